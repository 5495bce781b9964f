/*
 * Diversity-aware re-ranking of retrieved news lists: greedy Maximal Marginal
 * Relevance (part of the C ABI of libnewsrec_hip.so; included by newsrec.h's users
 * next to it, same error model: NR_OK or a negative code, message in nr_last_error()).
 *
 * cand_table [N][cand_ld] (NR_F32 or NR_BF16) and cand_inv_norm [N] are the evaluation
 * path's candidate table and its 1 / max(|e_c|, 1e-8).  list_idx [U][M] / list_rel [U][M]
 * are M <= NR_RERANK_MAX retrieved rows per user and their relevance, e.g. the top_idx /
 * top_scores of nr_topk_users.  K of the M are picked one at a time; each pick maximises
 * lambda * relevance - (1 - lambda) * (largest similarity to anything already picked).
 *
 * Entries.  An entry is valid if 0 <= list_idx < N.  Every other entry is a pad: never
 *   read from the table, never chosen, wherever it sits in the list.
 * Similarity.  sim(i, j) = (e_i . e_j) cand_inv_norm[i] cand_inv_norm[j] over the entries'
 *   table rows, accumulated in f32:
 *     NR_F32   the f32 rows on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32);
 *     NR_BF16  the bf16 rows as stored on v_mfma_f32_32x32x16_bf16 (both operands are
 *              table rows: nothing is rounded).
 *   The product of a pair is computed once, for the lower position i < j, scaled as
 *   (dot * inv[i]) * inv[j], and used for (i, j) and (j, i): sim_out [U][M][M] is symmetric
 *   bit for bit.  Its diagonal and every pad row and column are written as 0.
 * Selection.  Round 0 picks the valid entry with the largest list_rel.  Round t >= 1
 *   picks, among the valid entries not yet chosen, the largest
 *     obj_i = lambda * rel_i - (1 - lambda) * ms_i,
 *   ms_i the maximum of sim(i, j) over the chosen j (it may be negative and is not clamped
 *   at 0).  Equal values go to the lower input position.  obj is evaluated in f32 without
 *   contraction: two rounded products and one rounded difference, (1 - lambda) rounded once.
 * lambda = 1.  The output is the input's valid entries stably sorted by list_rel
 *   descending; for a nr_topk_users list that is its first K entries unchanged.
 * Short lists.  With fewer than K valid entries the tail is idx -1, rel -inf, pos -1.
 * out_rel holds list_rel of the chosen entries, copied bit for bit; out_pos (nullable)
 *   their positions in the input list.
 * Diversity figures (out_ild, nullable, [U][2]).  [u][0] is the mean over pairs i < j of
 *   1 - sim(i, j) among the first min(K, valid) valid entries of the input, in input
 *   order; [u][1] the same over the chosen entries.  Both are 0 with fewer than two
 *   entries.  Both are f32, summed in a fixed order (each entry's pairs with the later
 *   positions in ascending position, then a fixed tree over the entries), from the same
 *   matrix the selection used.
 * Determinism.  No atomics; two runs give the same bits.  A user's outputs depend only
 *   on its own list, not on U or on its place in the grid.
 * Inputs are finite (list_rel of a pad may be anything).
 *
 * Refused before any launch: dim != 1024 (NR_ERR_UNSUPPORTED); with NR_ERR_INVALID: a
 * dtype that is not NR_F32 / NR_BF16, M outside [1, NR_RERANK_MAX], K outside [1, M],
 * lambda outside [0, 1] or NaN, U < 1 or U >= 2^31, N < 1 or N >= 2^31, cand_ld < dim or
 * rows that are not 16-byte aligned, null required pointers, pointers that are not
 * device memory.  No workspace.
 */
#ifndef NEWSREC_RERANK_H
#define NEWSREC_RERANK_H

#include "newsrec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NR_RERANK_MAX 64 /* == NR_TOPK_MAX */

int nr_rerank_mmr(int dtype, int64_t dim, int64_t U, int64_t N, const void* cand_table, int64_t cand_ld,
                  const float* cand_inv_norm, const int32_t* list_idx, const float* list_rel, int64_t M, int64_t K,
                  float lambda, int32_t* out_idx, float* out_rel, int32_t* out_pos, float* out_ild, float* sim_out,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_RERANK_H */
