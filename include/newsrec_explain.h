/*
 * Exact per-click attribution of recommendation scores: which clicks of a user's history
 * produced a listed news' score (part of the C ABI of libnewsrec_hip.so; included by
 * newsrec.h's users next to it, same error model: NR_OK or a negative code, message in
 * nr_last_error()).
 *
 * Both poolers of nr_pool_score are linear in the per-news rows of hist_table, so a score
 * splits into one additive contribution per history click.  For user u the history is
 *   r_0 .. r_{H-1} = hist_idx[hist_off[u] .. hist_off[u+1])      rows of hist_table
 * (laid out as nr_pool_score documents) and the list is
 *   c_j = list_idx[u][j], j < K                                  rows of cand_table.
 * The share rows g_h [1024] are
 *   NR_POOL_FINAL   den_d = sum_h p[r_h][d],  g_h[d] = x[r_h][d] p[r_h][d] / (den_d + 1e-10)
 *   NR_POOL_MEAN    g_h = t[r_h] / H
 *   NR_POOL_LATENT  m = sum_h t[r_h] / H,     g_h = t[r_h] / (H max(|m|, 1e-12))
 * so that sum_h g_h = u, nr_pool_score's pooled user, and the contribution of click h to
 * list entry j is
 *   a[h][j] = (g_h . e_{c_j}) cand_inv_norm[c_j] / max(|u|, 1e-8);
 * sum_h a[h][j] is the evaluation path's score of (u, c_j).
 *
 * Operands.  The table entries are used as stored (NR_BF16 rows are upcast); nothing is
 *   rounded to bf16 on the way (x p of two bf16 values is exact in f32); every product and
 *   sum is f32.  Both dtypes run on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32): dtype only
 *   selects how the two tables are stored.
 * Pads.  A list entry outside [0, N) is a pad: never read from the table; its column of
 *   contrib_out is 0, its sum_out 0, its top_pos -1 and its top_val -inf.
 * History rows are not range-checked here, as in nr_pool_score.
 * Empty history (H = 0).  top_pos -1, top_val -inf, sum_out 0; nothing is written to
 *   contrib_out.
 * Top-T.  top_pos[u][j][0..T) holds the history positions h (0-based within the user's
 *   history) of the T largest a[h][j], value descending, equal values by ascending
 *   position; the tail is (-1, -inf) when H < T.  top_val holds the contributions
 *   themselves, bit for bit equal to contrib_out where both are requested.
 * Sums.  sum_out[u][j] = sum_h a[h][j], added in ascending position.
 * Position independence.  The bits of a[h][j] depend only on the user's history (as an
 *   ordered list), on the history row r_h and on the listed row c_j: not on h, j, K, T, U,
 *   on which outputs were requested or on the user's place in the grid.  A news that occurs
 *   twice in a history gets two bit-identical contributions, ordered by the tie rule.
 * Determinism.  No atomics; two runs give the same bits.
 * Inputs are finite.
 *
 * top_pos / top_val [U][K][T] go together (both or neither); sum_out [U][K] and
 * contrib_out [hist_off[U]][K] (row = CSR row of the click) are nullable; at least one
 * output is requested.
 *
 * Refused before any launch: dim != 1024 (NR_ERR_UNSUPPORTED); with NR_ERR_INVALID: a
 * pooler other than FINAL / LATENT / MEAN, a dtype that is not NR_F32 / NR_BF16, K outside
 * [1, NR_TOPK_MAX], T outside [1, NR_EXPLAIN_TOP_MAX] when the top outputs are given, one
 * of top_pos / top_val without the other, no output at all, U < 1 or U >= 2^31, N < 1 or
 * N >= 2^31, leading dimensions too small (hist_ld < 2 dim for FINAL), rows that are not
 * 16-byte aligned, null required pointers, pointers that are not device memory.
 * No workspace.
 */
#ifndef NEWSREC_EXPLAIN_H
#define NEWSREC_EXPLAIN_H

#include "newsrec.h"
#include "newsrec_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NR_EXPLAIN_TOP_MAX 8

int nr_explain_scores(int pooler, int dtype, int64_t dim, const void* hist_table, int64_t hist_ld, int64_t N,
                      const void* cand_table, int64_t cand_ld, const float* cand_inv_norm, int64_t U,
                      const int32_t* hist_idx, const int64_t* hist_off, const int32_t* list_idx, int64_t K, int64_t T,
                      int32_t* top_pos, float* top_val, float* sum_out, float* contrib_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_EXPLAIN_H */
