// Top-K news retrieval over the whole table (include/newsrec_topk.h): users x table
// as an MFMA GEMM whose U x N score matrix never reaches memory.
//
//   prep     NR_BF16 only: users f32 -> bf16 rows in the workspace (round to nearest even)
//   stage 1  grid (user blocks of 128, runs of chunks of kChunk news rows).  A workgroup walks its
//            chunks in 128-row score tiles (nr_score_tile.h, shared with fullrank.hip: the tile
//            main loop, the exclusion staging and the walk exist once).  Epilogue, per tile:
//            two threads per user scan the row against the user's running K-th best (-inf
//            until K are kept) and the first of them keeps the few that pass and are not
//            excluded in the user's list in LDS, a binary heap with the worst kept entry at
//            the root.  The list goes out rank-sorted as K (score, row) pairs per (user, run
//            of chunks).
//   stage 2  one wave per user: a K-round merge of the chunk lists' heads (ties by row),
//            the survivors' rows (0 in place of a missing one: never row -1) to top_idx;
//            the evaluation path's scoring kernel over them (score_users_dispatch) into
//            top_scores; a rank sort of each row's <= 64 (score, row) pairs.  The sectioned
//            top-K (sections.hip) runs the same three kernels over S lists per user.
//
// Every comparison is on the strict total order (score descending, row ascending), so no
// result depends on the order in which lanes or workgroups ran.
//
// nr_topk_users_filtered (include/newsrec_filter.h) is the same launch sequence with stage 1's
// filtered instantiation: the catalogue predicate is applied to the scan's survivors.
#include "nr_score_tile.h"

#include "../../include/newsrec_filter.h"
#include "../../include/newsrec_page.h"
#include "../../include/newsrec_prior.h"
#include "../../include/newsrec_topk.h"

namespace nr {
namespace tk {

constexpr int KMAX = NR_TOPK_MAX;

__global__ __launch_bounds__(256) void topk_bf16_users_kernel(int64_t n8, const float* __restrict__ x,
                                                              __bf16* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 a = reinterpret_cast<const float4*>(x)[2 * i], b = reinterpret_cast<const float4*>(x)[2 * i + 1];
  bf16x8 o;
  o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)a.z; o[3] = (__bf16)a.w;
  o[4] = (__bf16)b.x; o[5] = (__bf16)b.y; o[6] = (__bf16)b.z; o[7] = (__bf16)b.w;
  reinterpret_cast<bf16x8*>(y)[i] = o;
}

int bf16_users_launch(int64_t U, const float* users, __bf16* out, hipStream_t st, const char* fn) {
  const int64_t n8 = U * D / 8;
  hipLaunchKernelGGL(topk_bf16_users_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, n8, users, out);
  NR_CHECK_LAUNCH(fn);
  return NR_OK;
}

// gsel[u] = gain[u] * max(|users[u]|, 1e-8) (include/newsrec_prior.h): one wave per user.  Lane l
// adds the squares of elements 4 l + 256 i + (0 .. 3) in that order, the lanes' sums meet in a
// butterfly: a fixed order, so the bits depend on the user row and its gain alone.
__global__ __launch_bounds__(256) void prior_gains_kernel(int64_t U, const float* __restrict__ users,
                                                          const float* __restrict__ gain, float* __restrict__ gsel) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= U) return;  // wave-uniform
  const float4* row = reinterpret_cast<const float4*>(users + u * D) + lane;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < (int)D / 256; ++i) {
    const float4 v = row[64 * i];
    ss += v.x * v.x;
    ss += v.y * v.y;
    ss += v.z * v.z;
    ss += v.w * v.w;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
  if (lane == 0) gsel[u] = mul_rn(gain[u], fmaxf(sqrtf(ss), 1e-8f));
}

int prior_gains_launch(int64_t U, const float* users, const float* gain, float* gsel, hipStream_t st, const char* fn) {
  hipLaunchKernelGGL(prior_gains_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, st, U, users, gain, gsel);
  NR_CHECK_LAUNCH(fn);
  return NR_OK;
}

// FILT: the catalogue filter (include/newsrec_filter.h).  The predicate is ANDed into the scan's
// masks, so an ineligible row never reaches the serial drain: while fewer than K rows are kept
// every finite score passes the scan, and a selective filter would otherwise feed the heap loop
// all of them.  The unfiltered instantiation holds none of it.
// PRIOR: the rank-one prior (include/newsrec_prior.h).  The score tile then holds selection
// keys, and the scan, the heap and the partials below keep keys where they say scores.
// AFTER: the cursor (include/newsrec_page.h).  A row is kept only if it lies strictly behind
// (cur_key, cur_row) in the order of better(): `v <= cur_key` is ANDed into the scan's masks ahead
// of the filter, so the rows above the cursor never reach the serial drain, and the drain
// settles the tie on the row.  Both threads of a user hold its cursor in two registers; no LDS.
// The instantiations without a cursor hold none of it.
template <typename TI, bool FILT, bool PRIOR, bool AFTER>
__global__ __launch_bounds__(256) void topk_stage1_kernel(int64_t U, int64_t N, const TI* __restrict__ users,
                                                          const TI* __restrict__ tab, int64_t ldt,
                                                          const float* __restrict__ cinv,
                                                          const int32_t* __restrict__ excl_idx,
                                                          const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                          int K, int64_t span_rows, Pair* __restrict__ part,
                                                          PriorArgs pri, AfterArgs aft) {
  __shared__ __attribute__((aligned(16))) uint32_t smem[4 * TILE_WORDS];  // ring [2][news | users]; score tile
  __shared__ float ls[KMAX * TS];  // the users' sorted lists, [rank][user]
  __shared__ int32_t li[KMAX * TS];
  __shared__ __attribute__((aligned(16))) float cinv_s[TS];
  __shared__ int cnt_s[TS];
  __shared__ uint16_t ex_s[XCAP * TS];
  __shared__ uint32_t ov_mask[TS / 32];
  __shared__ __attribute__((aligned(16))) int32_t ft_s[FILT ? ATTR_TIME_WORDS : 4];  // the tile's news times
  __shared__ uint32_t fc_s[FILT ? ATTR_CAT_WORDS : 1];                                //   and categories
  __shared__ __attribute__((aligned(16))) float prior_s[PRIOR ? TS : 4];  // the tile's priors
  __shared__ float gsel_s[PRIOR ? TS : 1];                                //   and the block's scaled gains

  const int tid = threadIdx.x, lane = tid & 63;
  const float NINF = -__builtin_inff();
  // this workgroup's news rows: span_rows = a whole number of chunks, one running list over them
  ChunkWalk<TI, FILT, PRIOR> w(smem, cinv_s, ex_s, ov_mask, ft_s, fc_s, U, N, users, tab, ldt, cinv, excl_idx,
                               excl_off, flt, span_rows, prior_s, gsel_s, pri);
  // selection state: threads 2u and 2u + 1 serve user u of the block; 2u owns its list
  const int su = w.su, sh = w.sh;
  const int64_t m0 = w.m0;
  int cnt = 0;            // rows kept so far (a heap in LDS, the worst at slot 0)
  float thr = NINF;       // the worst's score once K are kept; -inf until then (every finite score passes)
  float cur_key = __builtin_inff();  // AFTER: the user's cursor; (+inf, -1) is the start of the list
  int32_t cur_row = -1;
  if constexpr (AFTER) {
    if (w.live) {
      cur_key = aft.key[m0 + su];
      cur_row = aft.row[m0 + su];
    }
  }

  w.run([&](int64_t n0, float* T) __attribute__((always_inline)) {
    // ---- scan against the running K-th best; what passes and is not excluded is kept (ascending row)
    uint32_t mlo = 0, mhi = 0;
    {
      const float* row = T + su * TLD + 64 * sh;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
        uint32_t b = (v.x > thr ? 1u : 0u) | (v.y > thr ? 2u : 0u) | (v.z > thr ? 4u : 0u) | (v.w > thr ? 8u : 0u);
        if constexpr (AFTER)  // (a NaN cursor passes nothing)
          b &= (v.x <= cur_key ? 1u : 0u) | (v.y <= cur_key ? 2u : 0u) | (v.z <= cur_key ? 4u : 0u) |
               (v.w <= cur_key ? 8u : 0u);
        if (i < 8) mlo |= b << (4 * i);
        else mhi |= b << (4 * (i - 8));
      }
    }
    if constexpr (FILT) w.el.keep_eligible(sh, mlo, mhi);
    const uint32_t plo = __shfl_down(mlo, 1, 64), phi = __shfl_down(mhi, 1, 64);
    if (sh == 0 && w.live) {
      // 32 columns of the row at a time, in ascending row order
      auto drain = [&](uint32_t bits, int col0) __attribute__((always_inline)) {
        while (bits) {
          const int col = col0 + __builtin_ctz(bits);
          bits &= bits - 1;
          const float s = T[su * TLD + col];
          const int32_t row = (int32_t)(n0 + col);
          // a later row never beats an equal score already kept, so the compare is strict
          if (!(s > thr) || w.ex.staged(row)) continue;  // (the threshold may have risen since the scan)
          if constexpr (AFTER) {
            if (s == cur_key && row <= cur_row) continue;  // at the cursor's key: only the rows behind its row
          }
          // the list is a binary heap with the WORST kept entry (lowest score, then highest
          // row) at slot 0: log2 K steps per kept row
          int i;
          if (cnt < K) {  // append, sift up while worse than the parent
            i = cnt++;
            while (i > 0) {
              const int p = (i - 1) >> 1;
              const float ps = ls[p * TS + su];
              const int32_t pr = li[p * TS + su];
              if (!better(ps, pr, s, row)) break;
              ls[i * TS + su] = ps;
              li[i * TS + su] = pr;
              i = p;
            }
          } else {  // a full list drops its worst: sift down from the root past every worse child
            i = 0;
            for (int c = 1; c < K; c = 2 * i + 1) {
              float cs = ls[c * TS + su];
              int32_t cr = li[c * TS + su];
              if (c + 1 < K) {
                const float ds = ls[(c + 1) * TS + su];
                const int32_t dr = li[(c + 1) * TS + su];
                if (better(cs, cr, ds, dr)) {
                  cs = ds;
                  cr = dr;
                  ++c;
                }
              }
              if (!better(s, row, cs, cr)) break;
              ls[i * TS + su] = cs;
              li[i * TS + su] = cr;
              i = c;
            }
          }
          ls[i * TS + su] = s;
          li[i * TS + su] = row;
          if (cnt == K) thr = ls[su];
        }
      };
      drain(mlo, 0);
      drain(mhi, 32);
      drain(plo, 64);
      drain(phi, 96);
    }
    thr = __shfl(thr, lane & ~1, 64);
  });
  // ---- K (score, row) pairs per (user, chunk), best first (a rank sort of the kept
  // list); a short list ends in (-inf, -1)
  if (sh == 0) cnt_s[su] = cnt;
  __syncthreads();
  for (int i = tid; i < TS * K; i += 256) {
    const int u = i / K, j = i - u * K;
    if (m0 + u >= U) break;
    const int n = cnt_s[u];
    Pair pr{NINF, -1};
    int at = j;
    if (j < n) {
      pr.s = ls[j * TS + u];
      pr.r = li[j * TS + u];
      at = 0;
      for (int t = 0; t < n; ++t) at += better(ls[t * TS + u], li[t * TS + u], pr.s, pr.r) ? 1 : 0;
    }
    part[((m0 + u) * gridDim.y + blockIdx.y) * K + at] = pr;
  }
}

// One wave per list (S lists per user, row u = user * S + list; S = 1: one per user): K rounds
// over the heads of its chunk lists (each sorted).  Lane l keeps the best head among chunks
// l, l + 64, ... and re-reads them only after it won.  The scoring pass behind it takes a
// user's S K rows as one list: uidx / coff are per user.  cnt_out may be null (topk_sort_kernel).
// next_key / next_row (null: not wanted; include/newsrec_page.h): the last round's winner, the
// list's last survivor in selection order, or the end cursor when fewer than K survived.
__global__ __launch_bounds__(256) void topk_merge_kernel(int64_t U, int S, int K, int nchunks,
                                                         const Pair* __restrict__ part, int32_t* __restrict__ top_idx,
                                                         int32_t* __restrict__ cnt_out, int32_t* __restrict__ uidx,
                                                         int64_t* __restrict__ coff, float* __restrict__ next_key,
                                                         int32_t* __restrict__ next_row) {
  __shared__ uint8_t head[4][kMaxChunks];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= U * S) return;  // wave-uniform; no block-wide barrier below
  const Pair* p = part + u * nchunks * K;
  for (int c = lane; c < nchunks; c += 64) head[wave][c] = 0;
  const float NINF = -__builtin_inff();
  float bs;
  int32_t br;
  int bc;
  auto refresh = [&]() {
    bs = NINF;
    br = INT32_MAX;
    bc = -1;
    for (int c = lane; c < nchunks; c += 64) {
      const int h = head[wave][c];
      if (h >= K) continue;
      const Pair e = p[(int64_t)c * K + h];
      if (e.r >= 0 && better(e.s, e.r, bs, br)) {
        bs = e.s;
        br = e.r;
        bc = c;
      }
    }
  };
  refresh();
  int32_t mine = 0;  // lane j: the j-th survivor
  int cnt = 0;
  float last_s = NINF;  // the latest winner (every lane holds the butterfly's result)
  int32_t last_r = INT32_MAX;
  for (int j = 0; j < K; ++j) {
    float ws = bs;
    int32_t wr = br;
    int wl = lane;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float os = __shfl_xor(ws, m, 64);
      const int32_t orow = __shfl_xor(wr, m, 64);
      const int ol = __shfl_xor(wl, m, 64);
      // rows are distinct across chunks, so (score, row) alone orders every live head;
      // two exhausted lanes (row INT32_MAX) tie and either may stand
      if (better(os, orow, ws, wr)) {
        ws = os;
        wr = orow;
        wl = ol;
      }
    }
    wl = __shfl(wl, 0, 64);
    wr = __shfl(wr, 0, 64);
    if (wr == INT32_MAX) break;  // every list is exhausted
    if (lane == j) mine = wr;
    last_s = ws;
    last_r = wr;
    ++cnt;
    if (lane == wl) {
      head[wave][bc] += 1;
      refresh();
    }
  }
  if (lane < K) top_idx[u * K + lane] = lane < cnt ? mine : 0;  // never row -1 to the scoring gather
  if (lane == 0) {
    if (cnt_out) cnt_out[u] = cnt;
    if (next_key) {
      next_key[u] = cnt == K ? last_s : NINF;
      next_row[u] = cnt == K ? last_r : INT32_MAX;
    }
    if (u % S == 0) {
      const int64_t user = u / S;
      uidx[user] = (int32_t)user;
      coff[user] = u * K;
      if (user == U - 1) coff[U] = U * S * K;
    }
  }
}

// One wave per list (R of them): order its <= 64 (evaluation score, row) pairs, pad the tail.
// The list's length is the merge's count, or, where that was not kept (cnt_in null), counted
// again: the rows of its runs, at most K.  L >= K: the lanes compared against -- lanes K and up
// hold (-inf, INT32_MAX) pads, which beat nothing and are never written (a pad in lane
// j < K still ranks j), so a short list does not pay for 64 rounds.
// PRIOR (include/newsrec_prior.h): the order is by the key fl(score + fl(gain[user] * prior[row])),
// list u belonging to user u / S, and the keys go to top_keys (null: not wanted, which
// nr_topk_users_after alone allows) beside the untouched scores.
struct SortPrior {
  const float* news_prior;
  const float* user_gain;
  float* top_keys;
  int S;
};
template <int L, bool PRIOR>
__global__ __launch_bounds__(256) void topk_sort_kernel(int64_t R, int K, const int32_t* __restrict__ cnt_in,
                                                        int nchunks, const Pair* __restrict__ part,
                                                        int32_t* __restrict__ top_idx, float* __restrict__ top_scores,
                                                        SortPrior sp) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= R) return;
  int n;
  if (cnt_in) {
    n = cnt_in[u];
  } else {
    const Pair* p = part + u * nchunks * K;
    n = 0;
    for (int i = lane; i < nchunks * K; i += 64) n += p[i].r >= 0 ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
    n = min(n, K);
  }
  const bool valid = lane < n;
  const float s = valid ? top_scores[u * K + lane] : -__builtin_inff();
  const int32_t r = valid ? top_idx[u * K + lane] : INT32_MAX;
  float key = s;  // what the list is ordered by
  if constexpr (PRIOR) {
    if (valid) key = add_rn(s, mul_rn(sp.user_gain[u / sp.S], sp.news_prior[r]));
  }
  int rank = 0;
  for (int l = 0; l < L; ++l) {
    const float os = __shfl(key, l, 64);
    const int32_t orow = __shfl(r, l, 64);
    rank += (better(os, orow, key, r) || (os == key && orow == r && l < lane)) ? 1 : 0;
  }
  // (the shuffles above consumed every lane's loads: the row is rewritten in place)
  if (rank < K) {
    top_idx[u * K + rank] = valid ? r : -1;
    top_scores[u * K + rank] = s;
    if constexpr (PRIOR) {
      if (sp.top_keys) sp.top_keys[u * K + rank] = key;
    }
  }
}

}  // namespace tk
}  // namespace nr

extern "C" int64_t nr_topk_chunk_rows(void) { return nr::tk::kChunk; }

extern "C" int64_t nr_topk_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || K < 1 || K > nr::tk::KMAX) return -1;
  return nr::tk::topk_layout(dtype, U, N, K).total;
}

namespace nr {
namespace tk {

int topk_stage2_launch(const char* fn, const ScanArgs& a, int64_t S, int64_t k, int nruns, const Pair* part,
                       int32_t* cnt, int32_t* uidx, int64_t* coff, int32_t* top_idx, float* top_scores,
                       float* top_keys, float* next_key, int32_t* next_row) {
  hipStream_t st = (hipStream_t)a.stream;
  const int64_t R = a.U * S;
  const dim3 gw((unsigned)((R + 3) / 4));
  if (S != 1) cnt = nullptr;
  hipLaunchKernelGGL(topk_merge_kernel, gw, dim3(256), 0, st, a.U, (int)S, (int)k, nruns, part, top_idx, cnt, uidx,
                     coff, next_key, next_row);
  NR_CHECK_LAUNCH(fn);
  return topk_stage2_finish(fn, a, S, k, nruns, part, cnt, uidx, coff, top_idx, top_scores, top_keys);
}

int topk_stage2_finish(const char* fn, const ScanArgs& a, int64_t S, int64_t k, int nruns, const Pair* part,
                       int32_t* cnt, int32_t* uidx, int64_t* coff, int32_t* top_idx, float* top_scores,
                       float* top_keys) {
  hipStream_t st = (hipStream_t)a.stream;
  const int64_t R = a.U * S;
  const dim3 gw((unsigned)((R + 3) / 4));
  if (S != 1) cnt = nullptr;
  const int rc = nr::score_users_dispatch(a.dtype, a.users, uidx, a.cand_table, a.cand_ld, a.cand_inv_norm, top_idx,
                                          coff, a.U, top_scores, st);
  if (rc) return rc;
  const int rc2 = nr::with_int<8, 16, 32, 64>(
      k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64, [&] { return nr::unvalidated_code("top-K list length", (int)k); },
      [&](auto lanes) {
        constexpr int L = decltype(lanes)::value;
        const SortPrior sp{a.news_prior, a.user_gain, top_keys, (int)S};
        if (a.prior())
          hipLaunchKernelGGL((topk_sort_kernel<L, true>), gw, dim3(256), 0, st, R, (int)k, (const int32_t*)cnt, nruns,
                             part, top_idx, top_scores, sp);
        else
          hipLaunchKernelGGL((topk_sort_kernel<L, false>), gw, dim3(256), 0, st, R, (int)k, (const int32_t*)cnt, nruns,
                             part, top_idx, top_scores, sp);
        return NR_OK;
      });
  if (rc2) return rc2;
  NR_CHECK_LAUNCH(fn);
  // without a prior the keys are the scores
  if (top_keys && !a.prior() &&
      hipMemcpyAsync(top_keys, top_scores, (size_t)(R * k) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    nr::set_error("%s: hipMemcpyAsync failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return NR_ERR_HIP;
  }
  return NR_OK;
}

// nr_topk_users, nr_topk_users_filtered, nr_topk_users_prior and nr_topk_users_after: one
// validation, one launch sequence.  A filter with both pairs null runs the unfiltered stage 1, a
// null prior the stage 1 without one, a null cursor the stage 1 without one.  keyed: the prior
// entry, whose top_keys is required.  paged: the cursor entry (include/newsrec_page.h), with the
// prior entry's workspace, a nullable top_keys and the next cursor's two arrays (`next`).
struct NextCursor {
  float* key = nullptr;
  int32_t* row = nullptr;
};
static int topk_run(const char* fn, const ScanArgs& a, int64_t K, int32_t* top_idx, float* top_scores, void* ws,
                    int64_t ws_bytes, bool keyed = false, float* top_keys = nullptr, bool paged = false,
                    NextCursor next = {}) {
  auto k_ok = [&] {
    NR_CHECK_ARG(K >= 1 && K <= KMAX, "%s: K = %lld outside [1, %d]", fn, (long long)K, KMAX);
    return NR_OK;
  };
  if (const int rc = check_scan(fn, a, k_ok, no_check)) return rc;
  NR_CHECK_ARG((a.after_key == nullptr) == (a.after_row == nullptr), "%s: after_key and after_row go together", fn);
  NR_CHECK_ARG((next.key == nullptr) == (next.row == nullptr), "%s: next_key and next_row go together", fn);
  NR_CHECK_ARG(top_idx && top_scores && ws && (top_keys || !keyed), "%s: null pointer", fn);
  const TopkLayout L = topk_layout(a.dtype, a.U, a.N, K, keyed || paged);
  NR_CHECK_ARG(ws_bytes >= L.total, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes,
               (long long)L.total);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  if (const int rc = keyed || paged ? check_scan_device(fn, a, "top_idx, top_scores, top_keys, ws",
                                                        {top_idx, top_scores, top_keys, ws})
                                    : check_scan_device(fn, a, "top_idx, top_scores, ws", {top_idx, top_scores, ws}))
    return rc;
  if (paged)
    if (const int rc = nr::check_device_ptrs(fn, "after_key, after_row, next_key, next_row",
                                             {a.after_key, a.after_row, next.key, next.row}))
      return rc;

  hipStream_t st = (hipStream_t)a.stream;
  const int64_t U = a.U;
  char* w = (char*)ws;
  int32_t* cnt = (int32_t*)(w + L.cnt);
  int32_t* uidx = (int32_t*)(w + L.uidx);
  int64_t* coff = (int64_t*)(w + L.coff);
  Pair* part = (Pair*)(w + L.part);
  ScanLaunch sl;
  float* gsel = (float*)(w + L.gsel);
  if (const int rc = scan_prepare(fn, a, w + L.ub, sl, gsel)) return rc;
  const int rc1 = with_scan_types(a, [&](auto ti, auto filt, auto prior, auto after) {
    using TI = typename decltype(ti)::type;
    hipLaunchKernelGGL(
        (topk_stage1_kernel<TI, decltype(filt)::value, decltype(prior)::value, decltype(after)::value>), sl.g1,
        dim3(256), 0, st, U, a.N, (const TI*)sl.urows, (const TI*)a.cand_table, a.cand_ld, a.cand_inv_norm, a.excl_idx,
        a.excl_off, a.flt, (int)K, sl.span_rows, part, PriorArgs{a.news_prior, gsel}, AfterArgs{a.after_key, a.after_row});
    return NR_OK;
  });
  if (rc1) return rc1;
  NR_CHECK_LAUNCH(fn);
  return topk_stage2_launch(fn, a, 1, K, (int)sl.g1.y, part, cnt, uidx, coff, top_idx, top_scores, top_keys, next.key,
                            next.row);
}

}  // namespace tk
}  // namespace nr

extern "C" int nr_topk_users(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                             int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx,
                             const int64_t* excl_off, int64_t K, int32_t* top_idx, float* top_scores, void* ws,
                             int64_t ws_bytes, void* stream) {
  return nr::tk::topk_run("nr_topk_users",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off, {}, stream}, K,
                          top_idx, top_scores, ws, ws_bytes);
}

extern "C" int nr_topk_users_filtered(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                      const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                      const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                      const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                      const uint64_t* q_cat_mask, int64_t K, int32_t* top_idx, float* top_scores,
                                      void* ws, int64_t ws_bytes, void* stream) {
  return nr::tk::topk_run("nr_topk_users_filtered",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                           {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream},
                          K, top_idx, top_scores, ws, ws_bytes);
}

extern "C" int64_t nr_topk_users_prior_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || K < 1 || K > nr::tk::KMAX) return -1;
  return nr::tk::topk_layout(dtype, U, N, K, true).total;
}

extern "C" int nr_topk_users_prior(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                   const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                   const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                   const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                   const uint64_t* q_cat_mask, const float* news_prior, const float* user_gain,
                                   int64_t K, int32_t* top_idx, float* top_scores, float* top_keys, void* ws,
                                   int64_t ws_bytes, void* stream) {
  return nr::tk::topk_run("nr_topk_users_prior",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                           {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream, news_prior, user_gain},
                          K, top_idx, top_scores, ws, ws_bytes, true, top_keys);
}

extern "C" int64_t nr_topk_users_after_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K) {
  return nr_topk_users_prior_workspace_bytes(dtype, U, N, K);
}

extern "C" int nr_topk_users_after(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                   const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                   const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                   const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                   const uint64_t* q_cat_mask, const float* news_prior, const float* user_gain,
                                   const float* after_key, const int32_t* after_row, float* next_key,
                                   int32_t* next_row, int64_t K, int32_t* top_idx, float* top_scores, float* top_keys,
                                   void* ws, int64_t ws_bytes, void* stream) {
  return nr::tk::topk_run("nr_topk_users_after",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                           {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream, news_prior, user_gain,
                           after_key, after_row},
                          K, top_idx, top_scores, ws, ws_bytes, false, top_keys, true, {next_key, next_row});
}
