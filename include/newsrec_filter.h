/*
 * Catalogue filters (time window, category) for top-K retrieval and the full-table
 * ranks (part of the C ABI of libnewsrec_hip.so; same error model as newsrec.h:
 * NR_OK or a negative code, message in nr_last_error()).
 *
 * nr_topk_users_filtered / nr_rank_targets_filtered are nr_topk_users
 * (newsrec_topk.h) / nr_rank_targets (newsrec_fullrank.h) with a per-user
 * predicate over per-news attributes.  Every argument they share with those
 * entries means what it means there.
 *
 *   news_time  [N] int32   one time per table row (the unit is the caller's)
 *   q_time_lo  [U] int32   the user's window, both bounds inclusive;
 *   q_time_hi  [U] int32     lo > hi is an empty window
 *   news_cat   [N] uint8   one category per table row
 *   q_cat_mask [U] uint64  bit c set: category c is wanted
 *
 * Eligibility.  Row c is eligible for user row u when all of these hold:
 *   - c is not on u's exclusion list;
 *   - news_time is null, or q_time_lo[u] <= news_time[c] <= q_time_hi[u];
 *   - news_cat is null, or news_cat[c] < 64 and bit news_cat[c] of q_cat_mask[u] is set.
 *   A category of 64 or more is ineligible under every mask: no input is undefined.
 * Pairing.  news_time goes with q_time_lo and q_time_hi, news_cat with q_cat_mask:
 *   one half of a pair without the other is refused (NR_ERR_INVALID) before any
 *   launch.  Either pair may be null.  With both pairs null the call is
 *   nr_topk_users / nr_rank_targets bit for bit (the same kernels run).
 * Inherited contract, with "eligible" as above:
 *   score descending, ties by ascending row; a (-1, -inf) tail when fewer than K
 *   rows are eligible, all of it when none is; a zero user gets the first K
 *   eligible rows in row order; top_scores are nr_score_users' bit for bit; a
 *   target that is itself ineligible -- excluded, outside its user's window, of an
 *   unwanted category, or outside [0, N) -- gets rank -1; for K <= NR_TOPK_MAX
 *   {t : rank(u, t) < K} is the filtered top-K row set; no float atomics, a
 *   fixed merge order, the same bits on two runs.
 * Selection scores are those of the unfiltered entries, bit for bit: the predicate
 *   acts on the finished score tile, never on the product, so a filtered call equals
 *   the unfiltered call with the ineligible rows appended to the exclusion lists.
 *
 * Workspace: nr_topk_workspace_bytes / nr_rank_targets_workspace_bytes (the filter
 * needs none).
 *
 * Refused before any launch: whatever nr_topk_users / nr_rank_targets refuse, with
 * the same codes; with NR_ERR_INVALID also an unpaired filter pointer (above) and a
 * filter pointer that is not device memory.
 */
#ifndef NEWSREC_FILTER_H
#define NEWSREC_FILTER_H

#include "newsrec_fullrank.h"
#include "newsrec_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

int nr_topk_users_filtered(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                           int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx,
                           const int64_t* excl_off, const int32_t* news_time, const int32_t* q_time_lo,
                           const int32_t* q_time_hi, const uint8_t* news_cat, const uint64_t* q_cat_mask, int64_t K,
                           int32_t* top_idx, float* top_scores, void* ws, int64_t ws_bytes, void* stream);
int nr_rank_targets_filtered(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                             const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                             const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                             const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                             const uint64_t* q_cat_mask, int64_t T, const int32_t* tgt_idx, const int64_t* tgt_off,
                             int32_t* rank, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_FILTER_H */
