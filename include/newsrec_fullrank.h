/*
 * Full-table ranks of target news (part of the C ABI of libnewsrec_hip.so; included by
 * newsrec.h's users next to it, same error model: NR_OK or a negative code, message in
 * nr_last_error()).  Where nr_topk_users (newsrec_topk.h) returns the K best rows of the
 * table per user, this returns the exact position of given rows -- the clicked news of an
 * evaluation set -- among ALL eligible rows, which is what recall@K past NR_TOPK_MAX, MRR,
 * nDCG and the mean rank against the whole catalogue need.
 *
 * users, cand_table, cand_ld, cand_inv_norm, excl_idx and excl_off are as nr_topk_users
 * takes them.  tgt_idx[tgt_off[u] .. tgt_off[u + 1]) (int32 rows, int64 offsets of length
 * U + 1, tgt_off[0] = 0, ascending, T = tgt_off[U]) lists the target rows of user u: none,
 * or thousands; duplicates are allowed and each gets its own answer.
 *
 * Result.  rank[j] (int32, j in [0, T)), for target row t = tgt_idx[j] of user u, is the
 *   number of eligible rows c != t with better(sel(u, c), c, sel(u, t), t), where better is
 *   top-K's strict total order (selection score descending, then row ascending) and a row
 *   is eligible when it lies in [0, N) and is not on u's exclusion list.  The best row has
 *   rank 0.  A target that is itself excluded or outside [0, N) gets -1.
 * Selection scores sel(u, c) are newsrec_topk.h's, from the same code: the MFMA product of
 *   the user with the table row (NR_F32: exact-f32 MFMA; NR_BF16: users rounded to bf16 x
 *   the bf16 table on v_mfma_f32_16x16x32_bf16, f32 accumulation), scaled by
 *   cand_inv_norm[c]; their bits depend only on the two rows.  So
 *     - duplicate table rows tie exactly and the row rule decides between them;
 *     - a target never counts itself (its own threshold comes from the same MFMA chain);
 *     - for any K <= NR_TOPK_MAX, {t : rank(u, t) < K} is exactly the row set that
 *       nr_topk_users returns for u with the same exclusions.
 * Fixed result.  No float atomics; integer counts are summed with integer atomics into a
 *   zeroed output, so the result does not depend on their order and two runs give the
 *   same bits.  A zero user scores 0 everywhere: rank(t) = the number of eligible rows
 *   below t.
 * Inputs are finite.
 *
 * The U x N scores never reach memory.  Workspace:
 *   nr_rank_targets_workspace_bytes(dtype, U, N, T) = up256(NR_BF16 ? 2 dim U : 0) + up256(4 T)
 *   bytes (up256 rounds up to a multiple of 256; so <= 2 dim U + 4 T + 512), 256-byte
 *   aligned: the bf16 users and one f32 threshold per target.
 *
 * Refused before any launch: dim != 1024 (NR_ERR_UNSUPPORTED), N > 2^22
 * (NR_ERR_UNSUPPORTED, as nr_topk_users); with NR_ERR_INVALID: a dtype that is not
 * NR_F32 / NR_BF16, U < 1 or U >= 2^31, N < 1, T < 0 or T >= 2^31, cand_ld < dim or rows
 * that are not 16-byte aligned, excl_idx without excl_off or the reverse, null pointers
 * (tgt_idx and rank may be null when T = 0), a workspace that is too small or misaligned,
 * pointers that are not device memory.  nr_rank_targets_workspace_bytes returns -1 for the
 * same bad (dtype, U, N, T).
 */
#ifndef NEWSREC_FULLRANK_H
#define NEWSREC_FULLRANK_H

#include "newsrec.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t nr_rank_targets_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t T);
int nr_rank_targets(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                    int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx, const int64_t* excl_off,
                    int64_t T, const int32_t* tgt_idx, const int64_t* tgt_off, int32_t* rank, void* ws,
                    int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_FULLRANK_H */
