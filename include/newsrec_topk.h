/*
 * Top-K news retrieval over the whole news table (part of the C ABI of
 * libnewsrec_hip.so; included by newsrec.h's users next to it, same error model:
 * NR_OK or a negative code, message in nr_last_error()).
 *
 * users [U][1024] f32 are pooled user rows as nr_pool_score's pooling-only call
 * writes them; cand_table [N][cand_ld] (NR_F32 or NR_BF16) and cand_inv_norm [N]
 * are the evaluation path's candidate table and its 1 / max(|e_c|, 1e-8).
 *
 * Result.  top_idx[u][0..K) holds the rows of cand_table with the K largest cosine
 *   scores against users[u]; rows listed in excl_idx[excl_off[u] .. excl_off[u+1])
 *   (a nullable CSR over the U users) are left out.  Duplicates in that list are
 *   allowed; an entry outside [0, N) is ignored.
 * Order.  Score descending; equal scores go by ascending row.
 * Short rows.  If fewer than K rows are eligible the tail is idx = -1, score = -inf.
 * A zero user (|u| < 1e-8, an empty history) scores 0 everywhere and gets the first
 *   K eligible rows in row order.
 * Inputs are finite.
 * Returned scores are the evaluation path's, bit for bit: top_scores[u][j] equals
 *   what nr_score_users writes for user u and candidate top_idx[u][j] (the K
 *   survivors are re-scored by that kernel), and the final order is by these scores.
 * Selection scores.  Which K rows survive is decided on an MFMA product of the users
 *   with the table, scaled by cand_inv_norm[c] (the user's own norm is a common
 *   positive factor of its row and is left out):
 *     NR_F32   f32 users x f32 table on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32);
 *     NR_BF16  users rounded to bf16 (a pre-pass into the workspace) x the bf16
 *              table on v_mfma_f32_16x16x32_bf16, accumulated in f32.
 *   Consequence: a row whose evaluation-path score lies within the accumulation
 *   error (f32, <= 1e-4 on the cosine scale) or, in bf16, within the rounding error
 *   of the user row (DESIGN.md section 3.8 has the measured band) of the K-th best
 *   may be swapped for its neighbour.
 * Position independence.  The bits of a pair's selection score depend only on the
 *   two rows, not on U, N or the pair's place in a tile or chunk, so duplicate news
 *   rows tie exactly and the tie rule above decides between them.
 * Fixed order.  No float atomics; every merge has a fixed order; two runs give the
 *   same bits.
 *
 * Stage 1 walks the table in chunks of nr_topk_chunk_rows() rows and writes K
 * (score, row) pairs per (user, chunk) to the workspace -- the U x N scores never
 * reach memory.  Workspace: nr_topk_workspace_bytes(dtype, U, N, K) <=
 *   U (2 dim + 64) + U ceil(N / chunk) K 8 + 4096 bytes, 256-byte aligned.
 *
 * Refused before any launch: dim != 1024 (NR_ERR_UNSUPPORTED), N > 2^22
 * (NR_ERR_UNSUPPORTED: the merge keeps at most 256 chunk heads per user); with
 * NR_ERR_INVALID: a dtype that is not NR_F32 / NR_BF16, K outside [1, NR_TOPK_MAX],
 * U < 1 or U >= 2^31, N < 1, cand_ld < dim or rows that are not 16-byte aligned,
 * excl_idx without excl_off or the reverse, null pointers, a workspace that is too
 * small or misaligned, pointers that are not device memory.
 * nr_topk_workspace_bytes returns -1 for the same bad (dtype, U, N, K).
 */
#ifndef NEWSREC_TOPK_H
#define NEWSREC_TOPK_H

#include "newsrec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NR_TOPK_MAX 64

int64_t nr_topk_chunk_rows(void); /* news rows per stage-1 partial; a multiple of 256 */
int64_t nr_topk_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K);
int nr_topk_users(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                  int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                  int64_t K, int32_t* top_idx, float* top_scores, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_TOPK_H */
