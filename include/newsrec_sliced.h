/* Column-sliced pool+score (csrc/pool_score.hip): nr_pool_score's scores from slice-major
 * images of the tables, so that an XCD's L2 holds a larger share of what is gathered.
 * Error model, dtype and pooler codes: include/newsrec.h. */
#ifndef NEWSREC_SLICED_H
#define NEWSREC_SLICED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Slice-major image of a row-major table for nr_pool_score_sliced:
 *   src [n_rows][parts * 1024] in `dtype` (row stride ld)  ->  dst [S][n_rows][parts * slice_w],
 * S = 1024 / slice_w, every slice dense.  Slice s of row r holds, part after part,
 * columns s * slice_w .. s * slice_w + slice_w - 1 of that part (parts = 1: an
 * embedding or latent table; parts = 2: FinalAttention's (x, exp(w)) rows).
 * slice_w is 64 or 128.  A bit-exact permutation; `inverse` != 0 runs it backwards
 * (src = the image, dst = the row-major table with row stride ld).
 */
int nr_slice_table(int dtype, int64_t n_rows, int parts, int slice_w, const void* src, int64_t ld, void* dst,
                   int inverse, void* stream);

/*
 * nr_pool_score's scores computed in column slices (three launches on `stream`):
 * per slice the chip gathers rows of slice_w columns from the slice images, so an
 * XCD's L2 holds 1024 / slice_w times as large a share of the table being gathered.
 *   pool    : per (slice, impression) the slice's pooled columns (f32) and their sum of squares
 *   score   : per (slice, impression) each candidate's partial dot over the slice's columns
 *   finalize: per candidate the partials added in slice order, then the same norm
 *             clamps (1e-12 latent, 1e-8 cosine) and cand_inv_norm as nr_pool_score
 * No atomics; the scores are the same bits from run to run.  They differ from
 * nr_pool_score's by f32 reassociation only (the history sum runs over 64 * 16 /
 * (slice_w * element size) row slots that are added in a tree, the dot is summed
 * per slice).
 * hist_image / cand_image: nr_slice_table images of the tables nr_pool_score takes
 * (hist parts = 2 for NR_POOL_FINAL), with n_hist_rows / n_cand_rows rows.
 * n_cand = cand_off[n_imp].  workspace: nr_pool_score_sliced_workspace_bytes(slice_w,
 * n_imp, n_cand) bytes, 16-byte aligned (f32 user rows [n_imp][1024], sums of squares
 * [S][n_imp], partial dots [S][n_cand]).  Same CSR, dim and index rules as nr_pool_score;
 * no `users` output and no hist_idx NULL form.
 */
int64_t nr_pool_score_sliced_workspace_bytes(int slice_w, int64_t n_imp, int64_t n_cand);
int nr_pool_score_sliced(int pooler, int dtype, int64_t dim, int slice_w, const void* hist_image,
                         int64_t n_hist_rows, const void* cand_image, int64_t n_cand_rows,
                         const float* cand_inv_norm, const int32_t* hist_idx, const int64_t* hist_off,
                         const int32_t* cand_idx, const int64_t* cand_off, int64_t n_imp, int64_t n_cand,
                         float* scores, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_SLICED_H */
