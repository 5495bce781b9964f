/*
 * Deep retrieval: up to NR_TOPK_DEEP_MAX rows per user from ONE walk over the table
 * (part of the C ABI of libnewsrec_hip.so; same error model as newsrec.h: NR_OK or a
 * negative code, message in nr_last_error()).
 *
 * nr_topk_users_deep is nr_topk_users_after (newsrec_page.h) with K allowed in
 * [1, NR_TOPK_DEEP_MAX]: the same argument list, every argument meaning what it means there,
 * the filter pairs, the prior pair, the cursor pairs and top_keys nullable as there.
 *
 * Eligibility, selection keys, order.  Exactly nr_topk_users_after's: a row is eligible for
 *   user u when it is not on the exclusion list, inside the filter, has a finite selection
 *   key s and lies strictly behind the cursor, better(after_key[u], after_row[u], s, r) with
 *   better(s, r, s2, r2) = s > s2 || (s == s2 && r < r2).  The selection key is what the shared
 *   score tile holds (newsrec_topk.h, "Selection scores"; newsrec_prior.h, "Selection keys"),
 *   so a cursor of one entry is a cursor of the other.  "Position independence", the fixed
 *   order of every comparison and the zero user are as stated there.
 * The list.  The row set of user u is exactly the K best eligible rows of the selection order:
 *   the union of the ceil(K / 64) cursor pages nr_topk_users_after would return from the same
 *   cursor, the last page asking for the remainder.  Returned scores are the evaluation
 *   path's (nr_score_users' bits: a re-score of the survivors); rows are ordered by score (by
 *   the key fl(score + fl(gain * prior)) under a prior) descending, ties by ascending row; a
 *   short list ends in idx -1, score -inf, key -inf.
 * The next cursor.  next_key[u], next_row[u] are the selection key and the row of the K-th
 *   survivor in selection order, the end cursor (-inf, INT32_MAX) when fewer than K rows
 *   survived: what the last of those pages would return.  next_* may alias after_*.
 * K <= NR_TOPK_MAX.  The call is forwarded to nr_topk_users_after behind this entry's own
 *   validation, and is that entry bit for bit; the deep kernels run for K > NR_TOPK_MAX only.
 * How the list is kept does not show: no result depends on U, on N's tiling, on the cut of the
 *   table into runs of chunks, or on when a user's candidate log was compacted.
 *
 * Workspace: nr_topk_users_deep_workspace_bytes; 256-byte aligned; -1 for the shapes
 *   nr_topk_users_after_workspace_bytes refuses and for K outside [1, NR_TOPK_DEEP_MAX].
 *   K <= NR_TOPK_MAX: nr_topk_users_after_workspace_bytes(dtype, U, N, K).  Otherwise, every
 *   term rounded up to 256 bytes, with C = nr_topk_chunk_rows() and R = the runs of chunks
 *   that walk side by side (1 once ceil(U / 128) >= 1024, else the fewest runs of equal
 *   length that bring ceil(U / 128) R to 1024, at most ceil(N / C)):
 *       (NR_BF16 ? 2048 U : 0) + 4 U + 4 U + 8 (U + 1) + 8 * 512 * U * R + 4 U
 *   the bf16 user rows, the list lengths, the re-score's user index and offsets, one log of
 *   512 (key, row) pairs per (user, run), the scaled gains: 4 KiB per user at R = 1.
 *
 * Refused before any launch: whatever nr_topk_users_after refuses, with the same codes and
 * message shapes (this entry's name in front), K outside [1, NR_TOPK_DEEP_MAX] where that
 * entry refuses K outside [1, NR_TOPK_MAX].  Not offered on deep lists: per-group caps,
 * sections (nr_topk_users_capped, nr_topk_sections stay at NR_TOPK_MAX).
 */
#ifndef NEWSREC_DEEP_H
#define NEWSREC_DEEP_H

#include "newsrec_page.h"

#define NR_TOPK_DEEP_MAX 256

#ifdef __cplusplus
extern "C" {
#endif

int64_t nr_topk_users_deep_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K);
int nr_topk_users_deep(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                       int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                       const int32_t* news_time, const int32_t* q_time_lo, const int32_t* q_time_hi,
                       const uint8_t* news_cat, const uint64_t* q_cat_mask, const float* news_prior,
                       const float* user_gain, const float* after_key, const int32_t* after_row, float* next_key,
                       int32_t* next_row, int64_t K, int32_t* top_idx, float* top_scores, float* top_keys, void* ws,
                       int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_DEEP_H */
