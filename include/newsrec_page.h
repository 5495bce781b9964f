/*
 * Cursors for top-K retrieval: continue a user's list past the first NR_TOPK_MAX rows
 * (part of the C ABI of libnewsrec_hip.so; same error model as newsrec.h: NR_OK or a
 * negative code, message in nr_last_error()).
 *
 * nr_topk_users_after is nr_topk_users_prior (newsrec_prior.h) restricted to the rows
 * that lie strictly behind a per-user position in the order every comparison of the
 * retrieval is made in -- selection key descending, row ascending -- and it returns the
 * position its own list ends at.  Feeding that position back gives the next K rows:
 * keyset pagination, to any depth, with two numbers of state per user.  Every argument
 * it shares with nr_topk_users_prior means what it means there; the filter pairs and
 * the prior pair may be null as there.
 *
 *   after_key [U] f32, after_row [U] int32, device   the cursor; both or neither
 *   next_key  [U] f32, next_row  [U] int32, device   the next cursor; both or neither
 *   top_keys  [U][K] f32, device                     may be null (not wanted)
 *
 * Eligibility.  With better(s, r, s2, r2) = s > s2 || (s == s2 && r < r2), a row r with
 *   selection key s is eligible for user u only if
 *       better(after_key[u], after_row[u], s, r)
 *   and the conditions of nr_topk_users_prior hold as well: not on the exclusion list,
 *   inside the filter, a finite key.  There are no special cases: (+inf, -1) is the start
 *   of the list, (-inf, INT32_MAX) is its end (nothing is eligible), and a NaN key makes
 *   nothing eligible.
 * The cursor is opaque.  The selection key is what stage 1 holds in its score tile: the
 *   MFMA product scaled by cand_inv_norm (newsrec_topk.h, "Selection scores": the user's
 *   norm left out), plus gsel_u * p_c under a prior (newsrec_prior.h, "Selection keys").
 *   It is NOT a returned score or key.  A cursor is therefore valid only with the user row,
 *   the table, cand_inv_norm, the dtype, news_prior and the user's gain it was made with;
 *   by "Position independence" of those two headers it does not depend on U, N's tiling,
 *   the chunk or the user block, so the users of a call may be regrouped between pages.
 *   Exclusion lists and filters may change between pages: they only take rows away.
 * The next cursor.  next_key[u], next_row[u] are the selection key and the row of the last
 *   survivor of user u in selection order (the K-th of the call).  When fewer than K rows
 *   were returned the end cursor (-inf, INT32_MAX) is written instead.  next_* may alias
 *   after_* (the cursors are read by stage 1 and written by stage 2).
 * Pages.  Repeated calls return consecutive, disjoint slices of one ordering of the eligible
 *   rows; each call is bit for bit reproducible from its cursor.  Everything else is
 *   nr_topk_users_prior's contract: returned scores are the evaluation path's (nr_score_users'
 *   bits), order inside the call is by score (by key under a prior), ties by ascending row,
 *   short rows end in idx -1, score -inf, key -inf.  A zero user (its row exactly 0) walks
 *   the eligible rows in row order (by p_c under a prior), from the cursor onward.
 * Across a page boundary.  Pages are slices of the SELECTION order; inside a page the order
 *   is by evaluation score.  The last score of one page and the first of the next may
 *   therefore be out of order by at most the selection band of newsrec_topk.h ("Selection
 *   scores"): the distance within which selection and evaluation may order two rows
 *   differently.  The union of the first P pages is exactly the row set of the best P K
 *   rows in selection order.
 * Without a cursor.  With after_* null and next_* null the call runs the kernels of
 *   nr_topk_users_prior / nr_topk_users_filtered / nr_topk_users (whichever the null pairs
 *   select) and is that entry bit for bit.  With after_* null and next_* given, the lists are
 *   still those, and the cursor behind them is returned.  A start cursor gives the same bits
 *   as no cursor.
 *
 * Workspace: nr_topk_users_after_workspace_bytes, the layout of
 *   nr_topk_users_prior_workspace_bytes (nothing is added); 256-byte aligned; -1 for the
 *   shapes that function refuses.
 *
 * Refused before any launch: whatever nr_topk_users_prior refuses, with the same codes and
 * messages (a null top_keys excepted); with NR_ERR_INVALID also after_key without after_row
 * or the reverse, next_key without next_row or the reverse, and any of the four that is not
 * device memory.
 */
#ifndef NEWSREC_PAGE_H
#define NEWSREC_PAGE_H

#include "newsrec_prior.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t nr_topk_users_after_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K);
int nr_topk_users_after(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                        int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                        const int32_t* news_time, const int32_t* q_time_lo, const int32_t* q_time_hi,
                        const uint8_t* news_cat, const uint64_t* q_cat_mask, const float* news_prior,
                        const float* user_gain, const float* after_key, const int32_t* after_row, float* next_key,
                        int32_t* next_row, int64_t K, int32_t* top_idx, float* top_scores, float* top_keys, void* ws,
                        int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_PAGE_H */
