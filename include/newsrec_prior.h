/*
 * A rank-one prior (popularity, recency) for top-K retrieval, the full-table ranks
 * and the sectioned top-K (part of the C ABI of libnewsrec_hip.so; same error model
 * as newsrec.h: NR_OK or a negative code, message in nr_last_error()).
 *
 * nr_topk_users_prior / nr_rank_targets_prior / nr_topk_sections_prior are
 * nr_topk_users_filtered / nr_rank_targets_filtered (newsrec_filter.h) /
 * nr_topk_sections (newsrec_sections.h) with a news selected and ordered by
 *
 *     key(u, c) = cos(u, c) + g_u * p_c
 *
 * instead of cos(u, c).  Every argument they share with those entries means what it
 * means there.
 *
 *   news_prior [N] f32, device   p_c, one value per table row
 *   user_gain  [U] f32, device   g_u, one value per user row
 *   top_keys   [U][K] f32 ([U][S][k] for sections), device, required
 *
 * g_u = beta is a static popularity prior; a g_u that falls with the history's length
 * is a stronger prior for thin histories; an exponential recency decay
 * 2^-(t_u - t_c)/h = 2^-(t_u - t0)/h * 2^(t_c - t0)/h is of this form too.  With
 * g_u = 0 nothing changes for that user.
 *
 * Pairing.  news_prior and user_gain go together: one without the other is refused
 *   (NR_ERR_INVALID) before any launch.  With both null the call runs the kernels of
 *   the filtered / sectioned entry and is that entry bit for bit; top_keys then
 *   equals top_scores.  Both must be device memory.  Inputs are finite.
 * Returned scores.  top_scores stay the evaluation path's cosines, nr_score_users'
 *   bits; the prior never touches them.
 * Returned keys, final order.  top_keys[u][j] = fl32(top_scores[u][j] + fl32(g_u * p_c))
 *   for c = top_idx[u][j]: two separately rounded f32 operations, never contracted
 *   into an fma, so a host recomputes them exactly.  Lists are ordered by key
 *   descending, ties by ascending row.  Short rows end in idx -1, score -inf,
 *   key -inf.
 * Selection keys.  Which rows survive is decided on sel(u, c) + gsel_u * p_c, where
 *   sel is the selection score of newsrec_topk.h bit for bit (the user's norm left
 *   out) and gsel_u = g_u * max(|u|, 1e-8), computed once per user in f32 in a fixed
 *   order by a pre-pass (one wave per user) into the workspace.  In real arithmetic
 *   gsel_u * p_c is g_u * p_c on the cosine scale times the positive factor that sel
 *   carries.  The product and the sum are again two separately rounded operations.
 *   Consequences: a user with g_u = 0 gets exactly the lists of the entry without a
 *   prior; a zero user (its row exactly 0) is ordered by p_c alone (descending for
 *   g_u > 0, ties by ascending row).  The swap band of newsrec_topk.h ("Selection
 *   scores") applies to keys as it does to scores.
 * Position independence, fixed order.  The bits of a pair's selection key depend only
 *   on the user row, g_u, the news row, cand_inv_norm[c] and p_c; not on U, N, the
 *   tile, the chunk or the user block.  No float atomics; two runs give the same bits.
 * Ranks.  nr_rank_targets_prior counts on selection keys; the target's own key comes
 *   from the same tile chain as the counted ones.  For K <= NR_TOPK_MAX,
 *   {t : rank(u, t) < K} is the row set of nr_topk_users_prior under the same
 *   arguments.  Ineligible targets keep rank -1.
 * Sections.  Section s of nr_topk_sections_prior equals nr_topk_users_prior with
 *   K = k and q_cat_mask[u] = sec_mask[s], bit for bit, keys included.
 *
 * Workspace: the ..._prior_workspace_bytes sibling of each entry: the base entry's
 *   layout plus U floats for the scaled gains; 256-byte aligned.  Each returns -1 for
 *   the shapes its base function refuses.
 *
 * Refused before any launch: whatever the base entries refuse, with the same codes
 * and messages; with NR_ERR_INVALID also news_prior without user_gain or the reverse,
 * a null top_keys, and a prior pointer or top_keys that is not device memory.
 */
#ifndef NEWSREC_PRIOR_H
#define NEWSREC_PRIOR_H

#include "newsrec_filter.h"
#include "newsrec_sections.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t nr_topk_users_prior_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K);
int nr_topk_users_prior(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                        int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                        const int32_t* news_time, const int32_t* q_time_lo, const int32_t* q_time_hi,
                        const uint8_t* news_cat, const uint64_t* q_cat_mask, const float* news_prior,
                        const float* user_gain, int64_t K, int32_t* top_idx, float* top_scores, float* top_keys,
                        void* ws, int64_t ws_bytes, void* stream);

int64_t nr_rank_targets_prior_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t T);
int nr_rank_targets_prior(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                          int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx,
                          const int64_t* excl_off, const int32_t* news_time, const int32_t* q_time_lo,
                          const int32_t* q_time_hi, const uint8_t* news_cat, const uint64_t* q_cat_mask,
                          const float* news_prior, const float* user_gain, int64_t T, const int32_t* tgt_idx,
                          const int64_t* tgt_off, int32_t* rank, void* ws, int64_t ws_bytes, void* stream);

int64_t nr_topk_sections_prior_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t S, int64_t k);
int nr_topk_sections_prior(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                           int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx,
                           const int64_t* excl_off, const int32_t* news_time, const int32_t* q_time_lo,
                           const int32_t* q_time_hi, const uint8_t* news_cat, const uint64_t* sec_mask,
                           const float* news_prior, const float* user_gain, int64_t S, int64_t k, int32_t* top_idx,
                           float* top_scores, float* top_keys, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_PRIOR_H */
