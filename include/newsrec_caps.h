/*
 * Per-group caps for top-K retrieval: at most `cap` news of one group in a list
 * (part of the C ABI of libnewsrec_hip.so; same error model as newsrec.h: NR_OK or
 * a negative code, message in nr_last_error()).
 *
 * nr_topk_users_capped is nr_topk_users_prior (newsrec_prior.h) under the rule "no
 * more than cap rows of one group".  Every argument it shares with that entry means
 * what it means there.
 *
 *   news_group [N] uint16, device   one group per table row, in [0, NR_CAP_GROUPS_MAX)
 *   cap                             in [1, NR_TOPK_MAX], the same for every group and user
 *
 * The rule.  Walk the eligible rows of a user (not excluded, inside the time window
 *   and the category mask) in the strict total order of newsrec_topk.h /
 *   newsrec_prior.h: selection key descending, ties by ascending row.  A row is taken
 *   if and only if fewer than cap rows of its group have been taken; the walk stops
 *   when K are taken.  That greedy list is the result (the optimum of a partition
 *   matroid truncated at K).  Without a prior the selection keys are the selection
 *   scores of newsrec_topk.h.
 * Inherited.  The time window, the category mask and the exclusion CSR compose.
 *   news_prior / user_gain are both present or both null.  top_keys [U][K] is
 *   required with a prior; without one it may be null, and if given equals
 *   top_scores.  top_scores are nr_score_users' bits.  The final order is by key
 *   descending, then row ascending.  Short lists end in (-1, -inf[, -inf]); a list is
 *   short when fewer than K rows are eligible UNDER THE CAPS (G groups can fill at
 *   most G * cap slots).  A zero user gets the first rows in row order that satisfy
 *   the caps (with a prior: in prior order).  Position independence holds: no float
 *   atomics, one running list per user in ascending row order, a fixed merge order;
 *   two runs give the same bits.
 * cap >= K.  The rule then never binds, and the call IS the base entry: it is
 *   dispatched to nr_topk_users_prior (with a prior or a top_keys) or
 *   nr_topk_users_filtered (without either) after this entry's own checks, so the
 *   outputs are those entries' bit for bit by construction.  The capped kernels run
 *   for cap < K only.
 * Groups are only ever compared; they never index memory.  A value >=
 *   NR_CAP_GROUPS_MAX is the caller's error: memory-safe, result unspecified (its
 *   high bits are dropped).  The Python layers refuse such labels on the host.
 *
 * Workspace: nr_topk_users_capped_workspace_bytes = that of nr_topk_users_prior
 *   (K pairs per user and chunk; the U scaled gains); 256-byte aligned.  It returns
 *   -1 for the shapes nr_topk_users_prior_workspace_bytes refuses.
 *
 * Refused before any launch: whatever nr_topk_users_prior refuses, with the same
 * codes (top_keys: only with a prior); with NR_ERR_INVALID also a null news_group, a
 * news_group that is not device memory, and cap outside [1, NR_TOPK_MAX].
 */
#ifndef NEWSREC_CAPS_H
#define NEWSREC_CAPS_H

#include "newsrec_prior.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NR_CAP_GROUPS_MAX 1024

int64_t nr_topk_users_capped_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K);
int nr_topk_users_capped(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                         int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                         const int32_t* news_time, const int32_t* q_time_lo, const int32_t* q_time_hi,
                         const uint8_t* news_cat, const uint64_t* q_cat_mask, const float* news_prior,
                         const float* user_gain, const uint16_t* news_group, int64_t cap, int64_t K, int32_t* top_idx,
                         float* top_scores, float* top_keys, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_CAPS_H */
