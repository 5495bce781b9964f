/*
 * The request path of top-K retrieval: nr_topk_users_after for at most NR_REQUEST_MAX_USERS
 * readers, at the cost of one read of the table (part of the C ABI of libnewsrec_hip.so; same
 * error model as newsrec.h: NR_OK or a negative code, message in nr_last_error()).
 *
 * nr_topk_request IS nr_topk_users_after (newsrec_page.h) for 1 <= U <= 32: the same arguments
 * with the same nullable pairs (exclusion CSR, time window and category mask, prior and gain,
 * cursor in, cursor out, top_keys), the same order (selection key descending, row ascending),
 * the same handling of short rows and zero users, and bit for bit the same top_idx, top_scores,
 * top_keys, next_key and next_row.  A cursor made by either entry is valid in the other.
 * K stays in [1, NR_TOPK_MAX].
 *
 * What differs is stage 1.  nr_topk_users_after multiplies blocks of 128 users with 128 news
 * rows, and at U <= 32 it keeps a handful of workgroups busy with tiles that are mostly padding.
 * Here the table is cut into R = ceil(N / nr_topk_request_run_rows(N)) <= 256 contiguous runs,
 * one workgroup per run; the <= 32 user rows stay in LDS as MFMA B fragments for the whole run
 * and the table rows stream from global memory straight into A fragments, every byte read once
 * device-wide.  The accumulation order of a (news, user) product is the bulk kernel's (32
 * v_mfma_f32_16x16x32_bf16 over ascending k in bf16; v_mfma_f32_32x32x2_f32 in the order
 * q = 0..3, t = 0..3 inside each ascending 32-deep slice in f32), so by "Position independence"
 * (newsrec_topk.h) the selection keys have the bulk kernel's bits.  Each (user, run) leaves K
 * rank-sorted pairs; stage 2 is nr_topk_users_after's, over R runs.
 *
 *   nr_topk_request_run_rows(N) = max(32, ceil(ceil(N / 256) / 32) * 32)
 *     288 at N = 72,023 (251 runs), 32 up to N = 8,192, 16,384 at N = 2^22.
 *
 * Exclusion lists may hold any number of rows of a run, duplicates, and entries outside [0, N)
 * (ignored), as in nr_topk_users_after.
 *
 * Workspace: nr_topk_request_workspace_bytes, with a256(b) = b rounded up to 256 and
 *   R = ceil(N / nr_topk_request_run_rows(N)):
 *     2 a256(4 U) + a256(8 (U + 1)) + a256(8 U R K) + a256(4 U)
 *   (cnt, uidx, coff, the partial lists, gsel: TopkLayout's arrays with R runs for its chunks; the
 *   bf16 user rows are rounded inside stage 1 and need no array).  At most about 4 MiB.
 *   256-byte aligned; -1 for a bad dtype, U outside [1, 32], N outside [1, 2^22], K outside
 *   [1, NR_TOPK_MAX].
 *
 * Refused before any launch: whatever nr_topk_users_after refuses, with the same codes and
 * messages under this entry's name; with NR_ERR_UNSUPPORTED also U > NR_REQUEST_MAX_USERS
 * (nr_topk_users_after is the entry for more users).
 */
#ifndef NEWSREC_REQUEST_H
#define NEWSREC_REQUEST_H

#include "newsrec_page.h"

#define NR_REQUEST_MAX_USERS 32

#ifdef __cplusplus
extern "C" {
#endif

int64_t nr_topk_request_run_rows(int64_t N);
int64_t nr_topk_request_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K);
int nr_topk_request(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                    int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                    const int32_t* news_time, const int32_t* q_time_lo, const int32_t* q_time_hi,
                    const uint8_t* news_cat, const uint64_t* q_cat_mask, const float* news_prior,
                    const float* user_gain, const float* after_key, const int32_t* after_row, float* next_key,
                    int32_t* next_row, int64_t K, int32_t* top_idx, float* top_scores, float* top_keys, void* ws,
                    int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_REQUEST_H */
