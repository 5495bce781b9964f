/*
 * Sectioned top-K retrieval: the k best eligible news of each of S sections per
 * user, from one walk over the news table (part of the C ABI of
 * libnewsrec_hip.so; same error model as newsrec.h: NR_OK or a negative code,
 * message in nr_last_error()).
 *
 * A section is a set of categories, a 64-bit mask as q_cat_mask of
 * newsrec_filter.h.  The S masks are the same for every user of a call (they are
 * the page layout) and are read on the HOST:
 *
 *   sec_mask   [S] uint64, HOST memory   bit c set: category c belongs to section s
 *   news_cat   [N] uint8, device         one category per table row (required)
 *   news_time, q_time_lo, q_time_hi      the time window of newsrec_filter.h
 *                                        (all three, or all three null)
 *   top_idx, top_scores  [U][S][k]       section s of user u at [u][s][0..k)
 *
 * Every other argument means what it means to nr_topk_users (newsrec_topk.h).
 *
 * The contract.  For every section s, top_idx[u][s][0..k) and
 *   top_scores[u][s][0..k) equal, bit for bit, what nr_topk_users_filtered
 *   returns with K = k, the same users, table, exclusion lists and time window,
 *   the same news_cat, and q_cat_mask[u] = sec_mask[s] for every u.
 * What that entry promises therefore holds per section: score descending, ties by
 *   ascending row; a (-1, -inf) tail when fewer than k rows of the section are
 *   eligible, all of it when none is; a zero user gets the section's first k
 *   eligible rows in row order; top_scores are nr_score_users' bit for bit; a
 *   category of 64 or more belongs to no section; no float atomics, a fixed merge
 *   order, the same bits on two runs.
 * Sections are disjoint: a table row belongs to at most one of them, so a news
 *   appears once on a page.  A mask of 0 is allowed and gives an empty section.
 *
 * Workspace: nr_topk_sections_workspace_bytes(dtype, U, N, S, k), which equals
 *   nr_topk_workspace_bytes(dtype, U, N, S k); 256-byte aligned.
 *
 * Refused before any launch: whatever nr_topk_users_filtered refuses, with the same
 * codes; with NR_ERR_INVALID also S outside [1, NR_SECTIONS_MAX], k < 1,
 * S k > NR_TOPK_MAX (the list slots a user has), U S >= 2^31, a null news_cat or
 * sec_mask, two section masks that share a bit (the message names both sections),
 * an unpaired time pointer, a news_cat or time pointer that is not device memory.
 * nr_topk_sections_workspace_bytes returns -1 for the same bad (dtype, U, N, S, k).
 */
#ifndef NEWSREC_SECTIONS_H
#define NEWSREC_SECTIONS_H

#include "newsrec_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NR_SECTIONS_MAX 16

int64_t nr_topk_sections_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t S, int64_t k);
int nr_topk_sections(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                     int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                     const int32_t* news_time, const int32_t* q_time_lo, const int32_t* q_time_hi,
                     const uint8_t* news_cat, const uint64_t* sec_mask, int64_t S, int64_t k, int32_t* top_idx,
                     float* top_scores, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_SECTIONS_H */
