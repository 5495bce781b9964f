// Sectioned top-K (include/newsrec_sections.h): the k best eligible news of each of S sections
// (disjoint sets of categories) per user, from ONE walk over the table.
//
//   stage 1  topk.hip's walk (nr_score_tile.h: the same product, exclusion staging, overflow
//            knock-out and time window, so the selection bits are topk.hip's), with the user's
//            64 LDS list slots split into S binary heaps of k slots, heap s in slots
//            [s k, (s + 1) k), worst entry at its root; a count and a threshold per (user,
//            section) in LDS.  A table row's section comes from a 64-entry category -> section
//            map (255: none), staged as one byte per tile column; the scan tests a row against
//            the threshold of ITS OWN section, so a section that can never fill (threshold
//            -inf to the end) sends only its own rows through the serial drain, and rows of no
//            section or outside the time window never reach it.
//   stage 2  topk.hip's merge, re-score and sort over the U S lists (topk_stage2_launch).
//
// Every comparison is on the strict total order (score descending, row ascending) and a row
// belongs to at most one heap, so section s's k survivors are the set nr_topk_users_filtered
// keeps with K = k and the mask sec_mask[s]: the contract is an equality of bits.
#include "nr_score_tile.h"

#include "../../include/newsrec_prior.h"
#include "../../include/newsrec_sections.h"

namespace nr {
namespace tk {

constexpr int SMAX = NR_SECTIONS_MAX;
constexpr int SLOTS = NR_TOPK_MAX;  // list slots per user: S k of them are used
constexpr uint32_t NOSEC = 255;

struct SecMap {
  uint32_t w[16];  // byte c: the section of category c, NOSEC when no section wants it
};

// One kept row into the heap of `cap` slots at hs / hr (slot stride TS), the WORST kept entry
// (lowest score, then highest row) at slot 0; n: the rows it holds.  The caller has checked
// that (s, row) beats the root when the heap is full.
__device__ __forceinline__ void heap_keep(float* hs, int32_t* hr, int& n, int cap, float s, int32_t row) {
  int i;
  if (n < cap) {  // append, sift up while worse than the parent
    i = n++;
    while (i > 0) {
      const int p = (i - 1) >> 1;
      const float ps = hs[p * TS];
      const int32_t pr = hr[p * TS];
      if (!better(ps, pr, s, row)) break;
      hs[i * TS] = ps;
      hr[i * TS] = pr;
      i = p;
    }
  } else {  // a full heap drops its worst: sift down from the root past every worse child
    i = 0;
    for (int c = 1; c < cap; c = 2 * i + 1) {
      float cs = hs[c * TS];
      int32_t cr = hr[c * TS];
      if (c + 1 < cap) {
        const float ds = hs[(c + 1) * TS];
        const int32_t dr = hr[(c + 1) * TS];
        if (better(cs, cr, ds, dr)) {
          cs = ds;
          cr = dr;
          ++c;
        }
      }
      if (!better(s, row, cs, cr)) break;
      hs[i * TS] = cs;
      hr[i * TS] = cr;
      i = c;
    }
  }
  hs[i * TS] = s;
  hr[i * TS] = row;
}

// flt carries the time window only (its category pair is null: Eligible then stages category
// 0 against the full mask); the categories act through the section bytes.  PRIOR: the rank-one
// prior of include/newsrec_prior.h; the score tile, heaps and thresholds then hold selection keys.
template <typename TI, bool PRIOR>
__global__ __launch_bounds__(256) void sections_stage1_kernel(int64_t U, int64_t N, const TI* __restrict__ users,
                                                              const TI* __restrict__ tab, int64_t ldt,
                                                              const float* __restrict__ cinv,
                                                              const int32_t* __restrict__ excl_idx,
                                                              const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                              const uint8_t* __restrict__ news_cat, SecMap map, int S,
                                                              int k, int64_t span_rows, Pair* __restrict__ part,
                                                              PriorArgs pri) {
  __shared__ __attribute__((aligned(16))) uint32_t smem[4 * TILE_WORDS];  // ring [2][news | users]; score tile
  __shared__ float ls[SLOTS * TS];  // the users' heaps, [slot][user]
  __shared__ int32_t li[SLOTS * TS];
  __shared__ float thr_s[SMAX * TS];    // [section][user]: the heap's root once it is full, -inf until then
  __shared__ uint8_t cnt_s[SMAX * TS];  // [section][user]: rows kept
  __shared__ __attribute__((aligned(16))) float cinv_s[TS];
  __shared__ uint16_t ex_s[XCAP * TS];
  __shared__ uint32_t ov_mask[TS / 32];
  __shared__ __attribute__((aligned(16))) int32_t ft_s[ATTR_TIME_WORDS];  // the tile's news times
  __shared__ uint32_t fc_s[ATTR_CAT_WORDS];                               //   (Eligible's category bytes: zeros here)
  __shared__ uint32_t sec_s[TS / 4];  // the tile's section bytes, one per column
  __shared__ uint32_t map_s[16];
  __shared__ __attribute__((aligned(16))) float prior_s[PRIOR ? TS : 4];  // the tile's priors
  __shared__ float gsel_s[PRIOR ? TS : 1];                                //   and the block's scaled gains

  const int tid = threadIdx.x;
  const float NINF = -__builtin_inff();
  for (int i = tid; i < SMAX * TS; i += 256) {
    thr_s[i] = NINF;
    cnt_s[i] = 0;
  }
  if (tid < 16) map_s[tid] = map.w[tid];
  ChunkWalk<TI, true, PRIOR> w(smem, cinv_s, ex_s, ov_mask, ft_s, fc_s, U, N, users, tab, ldt, cinv, excl_idx,
                               excl_off, flt, span_rows, prior_s, gsel_s, pri);
  const int su = w.su, sh = w.sh;
  const int64_t m0 = w.m0;
  const bool windowed = flt.news_time != nullptr;
  // thread c < TS carries the category of column c of the NEXT tile: loaded one tile ahead, so
  // the load lands under that tile's product
  uint32_t cat_next = tid < TS ? news_cat[min(w.c0 + tid, N - 1)] : 0;
  // (the walk's barriers order the initial stores above before the first epilogue)

  w.run([&](int64_t n0, float* T) __attribute__((always_inline)) {
    if (tid < TS) {
      reinterpret_cast<uint8_t*>(sec_s)[tid] =
          (uint8_t)(cat_next < 64 ? reinterpret_cast<const uint8_t*>(map_s)[cat_next] : NOSEC);
      cat_next = news_cat[min(n0 + TS + tid, N - 1)];
    }
    __syncthreads();
    // ---- scan: each column against the threshold of its own section
    uint32_t mlo = 0, mhi = 0;
    {
      const float* row = T + su * TLD + 64 * sh;
      const uint32_t* sc = sec_s + 16 * sh;
      const float* th = thr_s + su;
      auto pass = [&](float v, uint32_t sec) __attribute__((always_inline)) {
        return sec != NOSEC && v > th[(sec & (SMAX - 1)) * TS];
      };
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
        const uint32_t cw = sc[i];
        const uint32_t b = (pass(v.x, cw & 255u) ? 1u : 0u) | (pass(v.y, (cw >> 8) & 255u) ? 2u : 0u) |
                           (pass(v.z, (cw >> 16) & 255u) ? 4u : 0u) | (pass(v.w, cw >> 24) ? 8u : 0u);
        if (i < 8) mlo |= b << (4 * i);
        else mhi |= b << (4 * (i - 8));
      }
    }
    if (windowed) w.el.keep_eligible(sh, mlo, mhi);
    const uint32_t plo = __shfl_down(mlo, 1, 64), phi = __shfl_down(mhi, 1, 64);
    if (sh == 0 && w.live) {
      // 32 columns of the row at a time, in ascending row order
      auto drain = [&](uint32_t bits, int col0) __attribute__((always_inline)) {
        while (bits) {
          const int col = col0 + __builtin_ctz(bits);
          bits &= bits - 1;
          const int sec = reinterpret_cast<const uint8_t*>(sec_s)[col];
          const int at = sec * TS + su;
          const float s = T[su * TLD + col];
          const int32_t row = (int32_t)(n0 + col);
          // a later row never beats an equal score already kept, so the compare is strict
          if (!(s > thr_s[at]) || w.ex.staged(row)) continue;  // (the threshold may have risen since the scan)
          int n = cnt_s[at];
          heap_keep(ls + sec * k * TS + su, li + sec * k * TS + su, n, k, s, row);
          cnt_s[at] = (uint8_t)n;
          if (n == k) thr_s[at] = ls[sec * k * TS + su];
        }
      };
      drain(mlo, 0);
      drain(mhi, 32);
      drain(plo, 64);
      drain(phi, 96);
    }
  });
  // ---- k (score, row) pairs per (user, section, run of chunks), best first (a rank sort of the
  // heap); a short list ends in (-inf, -1).  (user, section) is a row of U S rows.
  const int SK = S * k;
  for (int i = tid; i < TS * SK; i += 256) {
    const int u = i / SK, rem = i - u * SK, s = rem / k, j = rem - s * k;
    if (m0 + u >= U) break;
    const int n = cnt_s[s * TS + u];
    const float* hs = ls + s * k * TS + u;
    const int32_t* hr = li + s * k * TS + u;
    Pair pr{NINF, -1};
    int at = j;
    if (j < n) {
      pr.s = hs[j * TS];
      pr.r = hr[j * TS];
      at = 0;
      for (int t = 0; t < n; ++t) at += better(hs[t * TS], hr[t * TS], pr.s, pr.r) ? 1 : 0;
    }
    part[(((m0 + u) * S + s) * gridDim.y + blockIdx.y) * k + at] = pr;
  }
}

static bool sections_shape_ok(int64_t U, int64_t S, int64_t k) {
  return S >= 1 && S <= SMAX && k >= 1 && S * k <= SLOTS && U * S < (1ll << 31);
}

}  // namespace tk
}  // namespace nr

extern "C" int64_t nr_topk_sections_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t S, int64_t k) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || !nr::tk::sections_shape_ok(U, S, k)) return -1;
  return nr::tk::topk_layout(dtype, U, N, S * k).total;
}

namespace nr {
namespace tk {

// nr_topk_sections and nr_topk_sections_prior: one validation, one launch sequence.  A null
// prior runs the stage 1 without one.  keyed: the prior entry, whose top_keys is required.
static int sections_run(const char* fn, int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                        const void* cand_table, int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx,
                        const int64_t* excl_off, const int32_t* news_time, const int32_t* q_time_lo,
                        const int32_t* q_time_hi, const uint8_t* news_cat, const uint64_t* sec_mask,
                        const float* news_prior, const float* user_gain, int64_t S, int64_t k, int32_t* top_idx,
                        float* top_scores, float* top_keys, bool keyed, void* ws, int64_t ws_bytes, void* stream) {
  // the time window travels as the scan's filter; the categories act through the section map
  const ScanArgs a{dtype,    dim,      U, users, N, cand_table, cand_ld, cand_inv_norm,
                   excl_idx, excl_off, {news_time, q_time_lo, q_time_hi, nullptr, nullptr}, stream, news_prior,
                   user_gain};
  auto sk_ok = [&] {
    NR_CHECK_ARG(S >= 1 && S <= SMAX, "%s: S = %lld outside [1, %d]", fn, (long long)S, SMAX);
    NR_CHECK_ARG(k >= 1, "%s: k = %lld < 1", fn, (long long)k);
    NR_CHECK_ARG(S * k <= SLOTS, "%s: S * k = %lld exceeds the %d list slots of a user", fn, (long long)(S * k), SLOTS);
    return NR_OK;
  };
  auto us_ok = [&] {
    NR_CHECK_ARG(U * S < (1ll << 31), "%s: U * S = %lld outside [1, 2^31)", fn, (long long)(U * S));
    return NR_OK;
  };
  if (const int rc = check_scan(fn, a, sk_ok, us_ok)) return rc;
  NR_CHECK_ARG(news_cat && sec_mask, "%s: news_cat and sec_mask are required", fn);
  SecMap map;
  for (int i = 0; i < 16; ++i) map.w[i] = ~0u;  // NOSEC in every byte
  for (int64_t s = 0; s < S; ++s)
    for (int c = 0; c < 64; ++c) {
      if (!((sec_mask[s] >> c) & 1)) continue;
      const uint32_t owner = (map.w[c >> 2] >> (8 * (c & 3))) & 255u;
      NR_CHECK_ARG(owner == NOSEC, "%s: sections %u and %lld share category %d (sections are disjoint)", fn, owner,
                   (long long)s, c);
      map.w[c >> 2] = (map.w[c >> 2] & ~(255u << (8 * (c & 3)))) | ((uint32_t)s << (8 * (c & 3)));
    }
  NR_CHECK_ARG(top_idx && top_scores && ws && (top_keys || !keyed), "%s: null pointer", fn);
  const TopkLayout L = topk_layout(dtype, U, N, S * k, keyed);
  NR_CHECK_ARG(ws_bytes >= L.total, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes,
               (long long)L.total);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  if (const int rc = keyed ? check_scan_device(fn, a, "news_cat, top_idx, top_scores, top_keys, ws",
                                               {news_cat, top_idx, top_scores, top_keys, ws})
                           : check_scan_device(fn, a, "news_cat, top_idx, top_scores, ws",
                                               {news_cat, top_idx, top_scores, ws}))
    return rc;

  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  Pair* part = (Pair*)(w + L.part);
  float* gsel = (float*)(w + L.gsel);
  ScanLaunch sl;
  if (const int rc = scan_prepare(fn, a, w + L.ub, sl, gsel)) return rc;
  const int rc1 = nr::with_dtype(dtype, [&](auto ti) {
    using TI = typename decltype(ti)::type;
    auto launch = [&](auto prior) {
      hipLaunchKernelGGL((sections_stage1_kernel<TI, decltype(prior)::value>), sl.g1, dim3(256), 0, st, U, N,
                         (const TI*)sl.urows, (const TI*)cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off, a.flt,
                         news_cat, map, (int)S, (int)k, sl.span_rows, part, PriorArgs{news_prior, gsel});
      return NR_OK;
    };
    return a.prior() ? launch(std::true_type{}) : launch(std::false_type{});
  });
  if (rc1) return rc1;
  NR_CHECK_LAUNCH(fn);
  return topk_stage2_launch(fn, a, S, k, (int)sl.g1.y, part, (int32_t*)(w + L.cnt), (int32_t*)(w + L.uidx),
                            (int64_t*)(w + L.coff), top_idx, top_scores, top_keys);
}

}  // namespace tk
}  // namespace nr

extern "C" int nr_topk_sections(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                const uint64_t* sec_mask, int64_t S, int64_t k, int32_t* top_idx, float* top_scores,
                                void* ws, int64_t ws_bytes, void* stream) {
  return nr::tk::sections_run("nr_topk_sections", dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx,
                              excl_off, news_time, q_time_lo, q_time_hi, news_cat, sec_mask, nullptr, nullptr, S, k,
                              top_idx, top_scores, nullptr, false, ws, ws_bytes, stream);
}

extern "C" int64_t nr_topk_sections_prior_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t S, int64_t k) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || !nr::tk::sections_shape_ok(U, S, k)) return -1;
  return nr::tk::topk_layout(dtype, U, N, S * k, true).total;
}

extern "C" int nr_topk_sections_prior(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                      const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                      const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                      const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                      const uint64_t* sec_mask, const float* news_prior, const float* user_gain,
                                      int64_t S, int64_t k, int32_t* top_idx, float* top_scores, float* top_keys,
                                      void* ws, int64_t ws_bytes, void* stream) {
  return nr::tk::sections_run("nr_topk_sections_prior", dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm,
                              excl_idx, excl_off, news_time, q_time_lo, q_time_hi, news_cat, sec_mask, news_prior,
                              user_gain, S, k, top_idx, top_scores, top_keys, true, ws, ws_bytes, stream);
}
