// Full-table ranks of target news (include/newsrec_fullrank.h): the users x table product
// of top-K retrieval (topk.hip) with a counting epilogue in place of the heap.  The tile
// main loop, its fragment maps, accumulation order and scaling are nr_score_tile.h's, the one
// copy both features run, so a (user, news) selection score has the same bits here, in
// topk_stage1_kernel and in both kernels below.
//
//   prep        NR_BF16 only: users f32 -> bf16 rows in the workspace (topk.hip's kernel);
//               rank[] is zeroed
//   thresholds  grid (user blocks of 128).  The targets of a block's users are consecutive in
//               tgt_idx; they are GATHERED as the news operand of the shared tile, 128 target
//               rows per tile, in as many tiles as the block's targets need.  Entry (u, t) of
//               the score tile -- the target's own selection score, from the same MFMA chain
//               that the counting pass runs for row t -- goes to the workspace as the
//               target's threshold; a target outside [0, N) or on its user's exclusion list
//               gets a NaN threshold (nothing compares better than it, or equal) and rank -1.
//   count       grid (user blocks of 128, runs of chunks) as top-K's stage 1.  Per score tile:
//               -inf over the user's excluded rows in the tile (the per-chunk staged list, or
//               the whole-workgroup path past XCAP); then the two threads of a user hold its
//               128 scores in registers, 64 each, and count per target how many of them are
//               better than (threshold, target row): scores and thresholds as order-preserving
//               integer keys, so that is one compare and one add per score and target.  The
//               first TCAP targets of a user stay in LDS for the whole walk (key, row and a
//               counter that both threads add to); a user with more re-scans its scores for
//               the rest, thresholds re-read per tile, the two threads' counts summed with a
//               lane exchange and added to rank[] per tile.  No target count is refused or
//               truncated.  Counts of workgroups that ran side by side are summed by integer
//               atomics into the zeroed rank[]: the sum does not depend on their order.
//
// nr_rank_targets_filtered (include/newsrec_filter.h) runs both kernels' filtered instantiations:
// a target outside its user's window or mask gets the NaN threshold, and the counting pass
// writes -inf over such rows of every score tile.
#include "nr_score_tile.h"

#include "../../include/newsrec_filter.h"
#include "../../include/newsrec_fullrank.h"
#include "../../include/newsrec_prior.h"

namespace nr {
namespace tk {

constexpr int TCAP = 32;  // targets of a user whose thresholds and counters stay in LDS for the whole walk

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// FILT (here and in rank_count_kernel): the catalogue filter of include/newsrec_filter.h; the
// unfiltered instantiations hold none of it.  PRIOR (here and in rank_count_kernel): the
// rank-one prior of include/newsrec_prior.h; thresholds and counted scores are then selection
// keys from the same ScoreTile chain, the gathered rows' priors staged next to their cand_inv.
template <typename TI, bool FILT, bool PRIOR>
__global__ __launch_bounds__(256) void rank_thresholds_kernel(int64_t U, int64_t N, int64_t Tn,
                                                              const TI* __restrict__ users,
                                                              const TI* __restrict__ tab, int64_t ldt,
                                                              const float* __restrict__ cinv,
                                                              const int32_t* __restrict__ excl_idx,
                                                              const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                              const int32_t* __restrict__ tgt_idx,
                                                              const int64_t* __restrict__ tgt_off,
                                                              float* __restrict__ tsel, int32_t* __restrict__ rank,
                                                              PriorArgs pri) {
  __shared__ __attribute__((aligned(16))) uint32_t smem[4 * TILE_WORDS];  // ring [2][news | users]; score tile
  __shared__ __attribute__((aligned(16))) float cinv_s[TS];
  __shared__ int32_t grow_s[2][TS];  // table rows behind the current and the next tile's news rows
  __shared__ int toff_s[TS + 1];     // the block's target offsets, minus the first
  __shared__ __attribute__((aligned(16))) float prior_s[PRIOR ? TS : 4];  // the gathered rows' priors
  __shared__ float gsel_s[PRIOR ? TS : 1];                                //   and the block's scaled gains
  const float* T = reinterpret_cast<const float*>(smem);

  const int tid = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.x * TS;
  const int nu = (int)min((int64_t)TS, U - m0);
  // (offsets are clamped into [0, T]: a malformed list cannot index past the arrays)
  const int64_t tb0 = clamp64(tgt_off[m0], 0, Tn);
  const int64_t tb1 = clamp64(tgt_off[m0 + nu], tb0, Tn);
  const int ntiles = (int)((tb1 - tb0 + TS - 1) / TS);
  if (ntiles == 0) return;  // block-uniform: none of these users has a target
  if (tid <= nu) toff_s[tid] = (int)(clamp64(tgt_off[m0 + tid], tb0, tb1) - tb0);
  if constexpr (PRIOR) {
    if (tid < TS) gsel_s[tid] = tid < nu ? pri.gsel[m0 + tid] : 0.f;
  }

  ScoreTile<TI, PRIOR> st(smem, cinv_s, users, m0, U, prior_s, gsel_s);
  auto fill_rows = [&](int tile, int buf) __attribute__((always_inline)) {
    if (tid < TS) {
      const int64_t j = tb0 + (int64_t)tile * TS + tid;
      const int32_t t = j < tb1 ? tgt_idx[j] : 0;
      grow_s[buf][tid] = t >= 0 && t < N ? t : 0;  // (a target outside the table: any row, the score is dropped)
    }
  };
  auto rows_of = [&](int buf) __attribute__((always_inline)) {
    const int32_t* g = grow_s[buf];
    return [=](int r) __attribute__((always_inline)) { return (int64_t)g[r]; };
  };
  fill_rows(0, 0);
  __syncthreads();
  st.gload(tab, ldt, rows_of(0), 0);
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    // (the other row list was last read by the tile before this one, behind its closing barrier;
    // it is read again after this tile's first barrier)
    if (tile + 1 < ntiles) fill_rows(tile + 1, buf ^ 1);
    if (tid < TS) cinv_s[tid] = cinv[grow_s[buf][tid]];
    if constexpr (PRIOR) {
      if (tid < TS) prior_s[tid] = pri.news_prior[grow_s[buf][tid]];
    }
    st.scores(tab, ldt, rows_of(buf), tile + 1 < ntiles, rows_of(buf ^ 1), TS);
    const int64_t j = tb0 + (int64_t)tile * TS + tid;
    if (tid < TS && j < tb1) {
      // the target's user: the last one of the block whose offset is <= j
      const int jl = (int)(j - tb0);
      int lo = 0, hi = nu;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (toff_s[mid] <= jl) lo = mid;
        else hi = mid;
      }
      const int32_t t = tgt_idx[j];
      bool ok = t >= 0 && t < N;
      if (ok && excl_off) {
        const int64_t e1 = excl_off[m0 + lo + 1];
        for (int64_t e = excl_off[m0 + lo]; e < e1; ++e) ok &= excl_idx[e] != t;
      }
      if constexpr (FILT) {  // a target outside its user's window or mask: the NaN threshold of an excluded one
        if (ok && flt.news_time) ok = in_window(flt.news_time[t], flt.q_lo[m0 + lo], flt.q_hi[m0 + lo]);
        if (ok && flt.news_cat) ok = in_mask(flt.news_cat[t], flt.q_mask[m0 + lo]);
      }
      tsel[j] = ok ? T[lo * TLD + tid] : __builtin_nanf("");
      if (!ok) rank[j] = -1;
    }
    __syncthreads();  // the next tile's operands overwrite the score tile
  }
}

// Order-preserving integer key of a score: k(a) > k(b) <=> a > b and k(a) == k(b) <=> a == b
// for non-NaN floats (-0 is folded into +0 first), so "better" is ONE integer compare per
// score: better(v, c, thr, t) <=> key(v) > key(thr) - (c < t).
__device__ __forceinline__ int score_key(float f) {
  const int b = __float_as_int(f + 0.0f);
  return b ^ ((b >> 31) & 0x7fffffff);
}
// the key of a target's threshold; a NaN threshold (a missing or refused target) counts nothing
__device__ __forceinline__ int threshold_key(float thr) { return thr == thr ? score_key(thr) : INT32_MAX; }

// how many of the 64 score keys k (news rows first + i) are better than (threshold key K, row trow)
__device__ __forceinline__ int count_better(const int (&k)[64], int K, int32_t trow, int first) {
  const int64_t d = (int64_t)trow - first;  // rows below trow win a tie: the first d of the 64
  int c = 0;
  if (d <= 0 || d >= 64) {     // (all but 64 of the table's rows: the target is not among these scores)
    const int Kp = K - (d >= 64 ? 1 : 0);
#pragma unroll
    for (int i = 0; i < 64; ++i) c += k[i] > Kp ? 1 : 0;
  } else {
#pragma unroll
    for (int i = 0; i < 64; ++i) c += k[i] > K - (i < d ? 1 : 0) ? 1 : 0;
  }
  return c;
}

template <typename TI, bool FILT, bool PRIOR>
__global__ __launch_bounds__(256) void rank_count_kernel(int64_t U, int64_t N, int64_t Tn,
                                                         const TI* __restrict__ users, const TI* __restrict__ tab,
                                                         int64_t ldt, const float* __restrict__ cinv,
                                                         const int32_t* __restrict__ excl_idx,
                                                         const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                         const int32_t* __restrict__ tgt_idx,
                                                         const int64_t* __restrict__ tgt_off,
                                                         const float* __restrict__ tsel, int64_t span_rows,
                                                         int32_t* __restrict__ rank, PriorArgs pri) {
  __shared__ __attribute__((aligned(16))) uint32_t smem[4 * TILE_WORDS];  // ring [2][news | users]; score tile
  __shared__ __attribute__((aligned(16))) float cinv_s[TS];
  __shared__ uint16_t ex_s[XCAP * TS];
  __shared__ uint32_t ov_mask[TS / 32];
  __shared__ int tk_s[TCAP * TS];      // the users' first TCAP targets, [slot][user]: threshold keys,
  __shared__ int32_t tr_s[TCAP * TS];  //   rows,
  __shared__ int tc_s[TCAP * TS];      //   and counters (both threads of a user add to one)
  __shared__ __attribute__((aligned(16))) int32_t ft_s[FILT ? ATTR_TIME_WORDS : 4];  // the tile's news times
  __shared__ uint32_t fc_s[FILT ? ATTR_CAT_WORDS : 1];                                //   and categories
  __shared__ __attribute__((aligned(16))) float prior_s[PRIOR ? TS : 4];  // the tile's priors
  __shared__ float gsel_s[PRIOR ? TS : 1];                                //   and the block's scaled gains

  const float NINF = -__builtin_inff();
  ChunkWalk<TI, FILT, PRIOR> w(smem, cinv_s, ex_s, ov_mask, ft_s, fc_s, U, N, users, tab, ldt, cinv, excl_idx,
                               excl_off, flt, span_rows, prior_s, gsel_s, pri);
  // threads 2u and 2u + 1 serve user u of the block: 64 scores of a tile each
  const int su = w.su, sh = w.sh;
  int64_t t0 = 0, t1 = 0;  // the user's targets (clamped into [0, T])
  if (w.live) {
    t0 = clamp64(tgt_off[w.m0 + su], 0, Tn);
    t1 = clamp64(tgt_off[w.m0 + su + 1], t0, Tn);
  }
  // the first TCAP targets of the user stay in LDS for the whole walk (the two threads stage
  // alternate slots; read after the first tile's barriers)
  const int nl = (int)min((int64_t)TCAP, t1 - t0);
  for (int j = sh; j < nl; j += 2) {
    tk_s[j * TS + su] = threshold_key(tsel[t0 + j]);
    tr_s[j * TS + su] = tgt_idx[t0 + j];
    tc_s[j * TS + su] = 0;
  }

  // (the epilogue changes nothing it captures: by value, so its operands stay the kernel's own values)
  w.run([=, &w](int64_t n0, float* T) __attribute__((always_inline)) {
    // ---- -inf over the user's staged excluded rows that fall in this tile (idempotent under duplicates)
    if (sh == 0 && w.ex.xn <= XCAP) {
      const int base = (int)(n0 - w.ex.cb);
      for (int i = 0; i < w.ex.xn; ++i) {
        const int d = (int)ex_s[i * TS + su] - base;
        if (d >= 0 && d < TS) T[su * TLD + d] = NINF;
      }
    }
    // ---- -inf over the rows outside the user's window or mask: each of its two threads over its
    // own 64 columns (stores of -inf only, like the ones above: no store can undo another)
    if constexpr (FILT) {
      uint32_t elo, ehi;
      w.el.rows64(sh, elo, ehi);
      float* row = T + su * TLD + 64 * sh;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t out = ~(h ? ehi : elo);
        if (out == 0) continue;
#pragma unroll
        for (int i = 0; i < 32; ++i)
          if ((out >> i) & 1u) row[32 * h + i] = NINF;
      }
    }
    __syncthreads();
    // ---- count: this thread's 64 scores, as keys in registers, against the user's targets
    if (t1 > t0) {  // (the same for both threads of a user: the lane exchange below has its partner)
      int k[64];
      const float* row = T + su * TLD + 64 * sh;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
        k[4 * i] = score_key(v.x);
        k[4 * i + 1] = score_key(v.y);
        k[4 * i + 2] = score_key(v.z);
        k[4 * i + 3] = score_key(v.w);
      }
      const int first = (int)n0 + 64 * sh;
      for (int j = 0; j < nl; ++j) {
        const int c = count_better(k, tk_s[j * TS + su], tr_s[j * TS + su], first);
        if (c) atomicAdd(&tc_s[j * TS + su], c);
      }
      // a user with more than TCAP targets re-scans its scores for the rest: thresholds re-read
      // per tile, counts added to rank[] per tile
      for (int64_t j = t0 + TCAP; j < t1; ++j) {
        int c = count_better(k, threshold_key(tsel[j]), tgt_idx[j], first);
        c += __shfl_xor(c, 1, 64);
        if (sh == 0 && c) atomicAdd(&rank[j], c);
      }
    }
  });
  // (the closing barrier of the last tile is behind every LDS add)
  for (int j = sh; j < nl; j += 2) {
    const int c = tc_s[j * TS + su];
    if (c) atomicAdd(&rank[t0 + j], c);
  }
}

struct RankLayout {
  int64_t tsel, gsel, total;  // (the NR_BF16 users sit at offset 0; with a prior, U scaled gains at the end)
};
static RankLayout rank_layout(int dtype, int64_t U, int64_t T, bool prior = false) {
  RankLayout L{};
  L.tsel = align256(dtype == NR_BF16 ? U * D * 2 : 0);
  L.gsel = L.tsel + align256(T * 4);
  L.total = L.gsel + align256(prior ? U * 4 : 0);
  return L;
}

}  // namespace tk
}  // namespace nr

extern "C" int64_t nr_rank_targets_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t T) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || T < 0 || T >= (1ll << 31)) return -1;
  return nr::tk::rank_layout(dtype, U, T).total;
}

namespace nr {
namespace tk {

// nr_rank_targets, nr_rank_targets_filtered and nr_rank_targets_prior: one validation, one launch
// sequence.  A filter with both pairs null runs the unfiltered kernels, a null prior the kernels
// without one.  keyed: the prior entry (its workspace holds the scaled gains).
static int rank_run(const char* fn, const ScanArgs& a, int64_t T, const int32_t* tgt_idx, const int64_t* tgt_off,
                    int32_t* rank, void* ws, int64_t ws_bytes, bool keyed = false) {
  auto t_ok = [&] {
    NR_CHECK_ARG(T >= 0 && T < (1ll << 31), "%s: T = %lld outside [0, 2^31)", fn, (long long)T);
    return NR_OK;
  };
  if (const int rc = check_scan(fn, a, no_check, t_ok)) return rc;
  NR_CHECK_ARG(tgt_off && ws && (T == 0 || (tgt_idx && rank)), "%s: null pointer", fn);
  const RankLayout L = rank_layout(a.dtype, a.U, T, keyed);
  NR_CHECK_ARG(ws_bytes >= L.total, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes,
               (long long)L.total);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  if (const int rc = check_scan_device(fn, a, "tgt_idx, tgt_off, rank, ws", {tgt_idx, tgt_off, rank, ws})) return rc;
  if (T == 0) return NR_OK;

  hipStream_t st = (hipStream_t)a.stream;
  float* tsel = (float*)((char*)ws + L.tsel);
  if (hipMemsetAsync(rank, 0, (size_t)T * 4, st) != hipSuccess) {
    nr::set_error("%s: hipMemsetAsync failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return NR_ERR_HIP;
  }
  ScanLaunch sl;
  float* gsel = (float*)((char*)ws + L.gsel);
  if (const int rc = scan_prepare(fn, a, ws, sl, gsel)) return rc;
  const PriorArgs pri{a.news_prior, gsel};
  return with_scan_types(a, [&](auto ti, auto filt, auto prior) {
    using TI = typename decltype(ti)::type;
    constexpr bool F = decltype(filt)::value, P = decltype(prior)::value;
    hipLaunchKernelGGL((rank_thresholds_kernel<TI, F, P>), sl.g0, dim3(256), 0, st, a.U, a.N, T, (const TI*)sl.urows,
                       (const TI*)a.cand_table, a.cand_ld, a.cand_inv_norm, a.excl_idx, a.excl_off, a.flt, tgt_idx,
                       tgt_off, tsel, rank, pri);
    NR_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL((rank_count_kernel<TI, F, P>), sl.g1, dim3(256), 0, st, a.U, a.N, T, (const TI*)sl.urows,
                       (const TI*)a.cand_table, a.cand_ld, a.cand_inv_norm, a.excl_idx, a.excl_off, a.flt, tgt_idx,
                       tgt_off, (const float*)tsel, sl.span_rows, rank, pri);
    NR_CHECK_LAUNCH(fn);
    return NR_OK;
  });
}

}  // namespace tk
}  // namespace nr

extern "C" int nr_rank_targets(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                               const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                               const int32_t* excl_idx, const int64_t* excl_off, int64_t T, const int32_t* tgt_idx,
                               const int64_t* tgt_off, int32_t* rank, void* ws, int64_t ws_bytes, void* stream) {
  return nr::tk::rank_run("nr_rank_targets",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off, {}, stream}, T,
                          tgt_idx, tgt_off, rank, ws, ws_bytes);
}

extern "C" int nr_rank_targets_filtered(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                        const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                        const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                        const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                        const uint64_t* q_cat_mask, int64_t T, const int32_t* tgt_idx,
                                        const int64_t* tgt_off, int32_t* rank, void* ws, int64_t ws_bytes,
                                        void* stream) {
  return nr::tk::rank_run("nr_rank_targets_filtered",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                           {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream},
                          T, tgt_idx, tgt_off, rank, ws, ws_bytes);
}

extern "C" int64_t nr_rank_targets_prior_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t T) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || T < 0 || T >= (1ll << 31)) return -1;
  return nr::tk::rank_layout(dtype, U, T, true).total;
}

extern "C" int nr_rank_targets_prior(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                     const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                     const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                     const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                     const uint64_t* q_cat_mask, const float* news_prior, const float* user_gain,
                                     int64_t T, const int32_t* tgt_idx, const int64_t* tgt_off, int32_t* rank, void* ws,
                                     int64_t ws_bytes, void* stream) {
  return nr::tk::rank_run("nr_rank_targets_prior",
                          {dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                           {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream, news_prior, user_gain},
                          T, tgt_idx, tgt_off, rank, ws, ws_bytes, true);
}
