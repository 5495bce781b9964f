// The request path of top-K retrieval (include/newsrec_request.h): nr_topk_users_after for at
// most 32 users, at the cost of one read of the table.
//
//   stage 1  one workgroup per run of run_rows consecutive news rows (<= 256 runs).  The <= 32
//            user rows are laid into LDS once, as the MFMA B fragments the lanes read (bf16
//            rounded here as topk_bf16_users_kernel rounds them), and stay for the whole run.
//            A wave streams a tile of 16 (bf16) / 32 (f32) table rows from global memory
//            straight into A fragments, two chunks of 16 loads per lane in flight, the next
//            tile's first chunks over the epilogue; the MFMA sequence per accumulator is
//            ScoreTile::compute's (nr_score_tile.h), so a (news, user) product has its bits.
//            Epilogue per round of 4 tiles: the raw products go to a small LDS tile; wave w
//            serves users w, w + 4, ...: lane l scales row l of a group of 64 as put4 does,
//            applies cursor, filter and exclusion list, and what beats the user's K-th best goes
//            into the wave-held sorted list (lane j = rank j; the position is a ballot of
//            better(), the tail moves up one lane).
//   stage 2  topk_stage2_launch (topk.hip) over R runs, unchanged.
//
// Every comparison is on the strict total order (key descending, row ascending), so no result
// depends on which wave or workgroup saw a row.
#include "nr_score_tile.h"

#include "../../include/newsrec_request.h"

namespace nr {
namespace tk {
namespace req {

constexpr int KMAX = NR_TOPK_MAX;
constexpr int UMAX = NR_REQUEST_MAX_USERS;
constexpr int UPW = UMAX / 4;  // users a wave serves in the epilogue
constexpr int LOADS = 16;      // 16-byte loads per lane and chunk

static inline int64_t run_rows(int64_t N) {
  const int64_t per = (N + kMaxChunks - 1) / kMaxChunks;
  return per < 32 ? 32 : (per + 31) / 32 * 32;
}
static inline int64_t runs_of(int64_t N) { return (N + run_rows(N) - 1) / run_rows(N); }

// TR: table rows per wave tile; NCH: chunks of LOADS loads per tile
template <typename TI> struct Geo { static constexpr int TR = 32, NCH = 8; };
template <> struct Geo<__bf16> { static constexpr int TR = 16, NCH = 2; };

// LDS: the users' B fragments, then the round's raw products [wave][user][row of the tile]
template <typename TI>
static inline int lds_bytes(int64_t U) {
  const int frag = sizeof(TI) == 4 ? (int)D * UMAX * 4 : (U > 16 ? 2 : 1) * (int)D * 16 * 2;
  return frag + 4 * UMAX * Geo<TI>::TR * 4;
}

template <typename TI>
__device__ __forceinline__ void load_chunk(u32x4 (&a)[LOADS], const u32x4* __restrict__ p, int c) {
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    if constexpr (sizeof(TI) == 4) a[i] = p[(4 * c + (i >> 2)) * 8 + (i & 3)];  // slice 4c + i/4, q = i % 4
    else a[i] = p[(LOADS * c + i) * 4];                                       // k step 16c + i
  }
}

template <typename TI, bool FILT, bool PRIOR, bool AFTER>
__global__ __launch_bounds__(256) void request_stage1_kernel(int U, int64_t N, const float* __restrict__ users,
                                                             const TI* __restrict__ tab, int64_t ldt,
                                                             const float* __restrict__ cinv,
                                                             const int32_t* __restrict__ excl_idx,
                                                             const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                             int K, int64_t rrows, Pair* __restrict__ part,
                                                             PriorArgs pri, AfterArgs aft) {
  constexpr int TR = Geo<TI>::TR, NCH = Geo<TI>::NCH, RR = 4 * TR, NG = RR / 64;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NINF = -__builtin_inff();
  const int nub = U > 16 ? 2 : 1;  // bf16: 16-user blocks in use
  const int frag_words = sizeof(TI) == 4 ? (int)D * UMAX : nub * (int)D * 16 / 2;
  float* S = reinterpret_cast<float*>(lds + frag_words);

  // ---- the users' B fragments, in the order the lanes read them (rows past U: zeros)
  if constexpr (sizeof(TI) == 4) {
    // fragment (slice s, q), lane (r, h): k = 32 s + 16 h + 4 q + (0 .. 3) of user r
    f32x4* UF = reinterpret_cast<f32x4*>(lds);
    for (int f = tid; f < 32 * 4 * 64; f += 256) {
      const int sq = f >> 6, l = f & 63, u = l & 31;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (u < U) v = *reinterpret_cast<const f32x4*>(users + (int64_t)u * D + 32 * (sq >> 2) + 16 * (l >> 5) + 4 * (sq & 3));
      UF[f] = v;
    }
  } else {
    // fragment (block j, step s), lane (r, g): k = 32 s + 8 g + (0 .. 7) of user 16 j + r
    bf16x8* UB = reinterpret_cast<bf16x8*>(lds);
    for (int f = tid; f < nub * 32 * 64; f += 256) {
      const int j = f >> 11, s = (f >> 6) & 31, l = f & 63, u = 16 * j + (l & 15);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (__bf16)0.f;
      if (u < U) {
        const float4* x = reinterpret_cast<const float4*>(users + (int64_t)u * D + 32 * s + 8 * (l >> 4));
        const float4 a = x[0], b = x[1];
        o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)a.z; o[3] = (__bf16)a.w;
        o[4] = (__bf16)b.x; o[5] = (__bf16)b.y; o[6] = (__bf16)b.z; o[7] = (__bf16)b.w;
      }
      UB[f] = o;
    }
  }

  // ---- this workgroup's rows [c0, c1)
  const int64_t c0 = (int64_t)blockIdx.x * rrows;
  const int64_t c1 = min(N, c0 + rrows);
  const int nrounds = (int)((c1 - c0 + RR - 1) / RR);

  // ---- per-user state of the epilogue: wave w serves users 4 i + w (wave-uniform values)
  float ls[UPW], gsel[UPW], cur_key[UPW];  // ls / lr: lane j holds rank j of the user's list
  int32_t lr[UPW], cur_row[UPW];
  uint32_t f_lo[UPW], f_span[UPW];
  uint64_t f_mask[UPW];
  int64_t e0[UPW], e1[UPW];
  int xcnt[UPW];  // the user's excluded rows inside this run
#pragma unroll
  for (int i = 0; i < UPW; ++i) {
    const int u = 4 * i + wave;
    ls[i] = NINF;
    lr[i] = INT32_MAX;
    gsel[i] = 0.f;
    cur_key[i] = __builtin_inff();
    cur_row[i] = -1;
    f_lo[i] = (uint32_t)INT32_MIN;
    f_span[i] = ~0u;
    f_mask[i] = ~0ull;
    e0[i] = e1[i] = 0;
    xcnt[i] = 0;
    if (u < U) {
      if constexpr (PRIOR) gsel[i] = pri.gsel[u];
      if constexpr (AFTER) {
        cur_key[i] = aft.key[u];
        cur_row[i] = aft.row[u];
      }
      if constexpr (FILT) {  // Eligible's window and mask (nr_score_tile.h)
        if (flt.news_cat) f_mask[i] = flt.q_mask[u];
        if (flt.news_time) {
          const int32_t a = flt.q_lo[u], b = flt.q_hi[u];
          f_lo[i] = (uint32_t)a;
          f_span[i] = (uint32_t)b - (uint32_t)a;
          if (a > b) {
            f_span[i] = 0;
            f_mask[i] = 0;
          }
        }
      }
      if (excl_off) {
        e0[i] = excl_off[u];
        e1[i] = excl_off[u + 1];
        for (int64_t e = e0[i]; e < e1[i]; e += 64) {
          const int64_t r = e + lane < e1[i] ? (int64_t)excl_idx[e + lane] : -1;
          xcnt[i] += __popcll(__ballot(r >= c0 && r < c1));
        }
      }
    }
  }
  __syncthreads();  // the fragments are in place

  // ---- the walk
  auto tile_ptr = [&](int64_t row0) __attribute__((always_inline)) {
    if constexpr (sizeof(TI) == 4)
      return reinterpret_cast<const u32x4*>(tab + min(row0 + (lane & 31), N - 1) * ldt + 16 * (lane >> 5));
    else
      return reinterpret_cast<const u32x4*>(tab + min(row0 + (lane & 15), N - 1) * ldt + 8 * (lane >> 4));
  };
  int64_t row0 = c0 + (int64_t)wave * TR;
  bool active = row0 < c1;
  const u32x4* p = tile_ptr(row0);
  u32x4 a0[LOADS], a1[LOADS];
  if (active) {
    load_chunk<TI>(a0, p, 0);
    load_chunk<TI>(a1, p, 1);
  }
  for (int round = 0; round < nrounds; ++round) {
    const int64_t g0 = c0 + (int64_t)round * RR;  // the round's first row
    // the rows' scales and attributes, lane l <-> row l of each group of 64 (they land over the MFMAs)
    float ci[NG], pr[NG];
    int32_t tm[NG];
    uint32_t ct[NG];
    if (wave < U) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int64_t r = g0 + 64 * g + lane;
        const bool in = r < c1;
        ci[g] = in ? cinv[r] : 0.f;
        pr[g] = 0.f;
        tm[g] = 0;
        ct[g] = 0;
        if constexpr (PRIOR) pr[g] = in ? pri.news_prior[r] : 0.f;
        if constexpr (FILT) {
          tm[g] = in && flt.news_time ? flt.news_time[r] : 0;
          ct[g] = in && flt.news_cat ? flt.news_cat[r] : 0u;
        }
      }
    }
    const int64_t nrow0 = row0 + RR;
    const bool nactive = nrow0 < c1;
    const u32x4* pn = tile_ptr(nrow0);
    if (active) {
      if constexpr (sizeof(TI) == 4) {
        const f32x4* UF = reinterpret_cast<const f32x4*>(lds) + lane;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        auto compute = [&](const u32x4(&a)[LOADS], int c) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < LOADS; ++i) {
            const f32x4 uf = UF[((4 * c + (i >> 2)) * 4 + (i & 3)) * 64];
            const f32x4 nf = __builtin_bit_cast(f32x4, a[i]);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(nf[t], uf[t], acc, 0, 0, 0);
          }
        };
#pragma unroll
        for (int c = 0; c < NCH; c += 2) {
          compute(a0, c);
          if (c + 2 < NCH) load_chunk<TI>(a0, p, c + 2);
          else if (nactive) load_chunk<TI>(a0, pn, 0);
          compute(a1, c + 1);
          if (c + 3 < NCH) load_chunk<TI>(a1, p, c + 3);
          else if (nactive) load_chunk<TI>(a1, pn, 1);
        }
        // C/D map: col (user) = lane & 31, row (news) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(S + (wave * UMAX + (lane & 31)) * TR + 8 * g + 4 * (lane >> 5)) =
              f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
      } else {
        const bf16x8* UB = reinterpret_cast<const bf16x8*>(lds) + lane;
        f32x4 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto compute = [&](const u32x4(&a)[LOADS], int c) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < LOADS; ++i) {
            const int s = LOADS * c + i;
            const bf16x8 nf = __builtin_bit_cast(bf16x8, a[i]);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf, UB[s * 64], acc[0], 0, 0, 0);
            if (nub > 1) acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf, UB[(32 + s) * 64], acc[1], 0, 0, 0);
          }
        };
        compute(a0, 0);
        if (nactive) load_chunk<TI>(a0, pn, 0);
        compute(a1, 1);
        if (nactive) load_chunk<TI>(a1, pn, 1);
        // C/D map: col (user) = lane & 15, row (news) = 4 (lane >> 4) + reg
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<f32x4*>(S + (wave * UMAX + 16 * j + (lane & 15)) * TR + 4 * (lane >> 4)) = acc[j];
      }
    }
    __syncthreads();
    // ---- epilogue: cursor, filter, exclusions, insertion
    if (wave < U) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int64_t n0 = g0 + 64 * g;
        if (n0 >= c1) break;  // (uniform)
        const int32_t row = (int32_t)(n0 + lane);
        const bool in = n0 + lane < c1;
        const int rr = 64 * g + lane;  // row of the round: tile rr / TR, its row rr % TR
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
          const int u = 4 * i + wave;
          if (u >= U) break;  // (uniform)
          const float raw = S[((rr / TR) * UMAX + u) * TR + rr % TR];
          float v;  // put4's scaling
          if constexpr (PRIOR) v = add_rn(mul_rn(raw, ci[g]), mul_rn(gsel[i], pr[g]));
          else v = mul_rn(raw, ci[g]);
          bool ok = in && v > NINF;
          if constexpr (AFTER) ok = ok && better(cur_key[i], cur_row[i], v, row);
          if constexpr (FILT)
            ok = ok && (uint32_t)tm[g] - f_lo[i] <= f_span[i] && ct[g] < 64 && ((f_mask[i] >> (ct[g] & 63)) & 1ull) != 0;
          if (xcnt[i] > 0) {  // (uniform) the user's list holds rows of this run: those of this group
            bool hit = false;
            for (int64_t e = e0[i]; e < e1[i]; e += 64) {
              const int64_t d64 = e + lane < e1[i] ? (int64_t)excl_idx[e + lane] - n0 : -1;
              const int d = d64 >= 0 && d64 < 64 ? (int)d64 : -1;
              uint64_t m = __ballot(d >= 0);
              while (m) {
                const int src = __builtin_ctzll(m);
                m &= m - 1;
                hit |= __shfl(d, src, 64) == lane;
              }
            }
            ok = ok && !hit;
          }
          float ks = __shfl(ls[i], K - 1, 64);  // the K-th best so far ((-inf, INT32_MAX): none yet)
          int32_t kr = __shfl(lr[i], K - 1, 64);
          for (;;) {
            const uint64_t m = __ballot(ok && better(v, row, ks, kr));
            if (!m) break;
            const int src = __builtin_ctzll(m);
            const float cs = __shfl(v, src, 64);
            const int32_t cr = (int32_t)(n0 + src);
            const int pos = __popcll(__ballot(better(ls[i], lr[i], cs, cr)));  // the list is sorted: a prefix
            const float us = __shfl_up(ls[i], 1, 64);
            const int32_t ur = __shfl_up(lr[i], 1, 64);
            if (lane > pos) {
              ls[i] = us;
              lr[i] = ur;
            } else if (lane == pos) {
              ls[i] = cs;
              lr[i] = cr;
            }
            ok = ok && lane != src;
            ks = __shfl(ls[i], K - 1, 64);
            kr = __shfl(lr[i], K - 1, 64);
          }
        }
      }
    }
    __syncthreads();  // the next round's products overwrite S
    row0 = nrow0;
    active = nactive;
    p = pn;
  }
  // ---- K (key, row) pairs per (user, run), best first; a short list ends in (-inf, -1)
#pragma unroll
  for (int i = 0; i < UPW; ++i) {
    const int u = 4 * i + wave;
    if (u < U && lane < K)
      part[((int64_t)u * gridDim.x + blockIdx.x) * K + lane] = Pair{ls[i], lr[i] == INT32_MAX ? -1 : lr[i]};
  }
}

struct Layout {
  int64_t runs, cnt, uidx, coff, part, gsel, total;
};
static inline Layout layout(int64_t U, int64_t N, int64_t K) {
  Layout L{};
  L.runs = runs_of(N);
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += align256(bytes);
    return at;
  };
  L.cnt = take(U * 4);
  L.uidx = take(U * 4);
  L.coff = take((U + 1) * 8);
  L.part = take(U * L.runs * K * (int64_t)sizeof(Pair));
  L.gsel = take(U * 4);
  L.total = o;
  return L;
}

}  // namespace req
}  // namespace tk
}  // namespace nr

extern "C" int64_t nr_topk_request_run_rows(int64_t N) { return nr::tk::req::run_rows(N); }

extern "C" int64_t nr_topk_request_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || U > nr::tk::req::UMAX || K < 1 || K > nr::tk::req::KMAX) return -1;
  return nr::tk::req::layout(U, N, K).total;
}

extern "C" int nr_topk_request(int dtype, int64_t dim, int64_t U, const float* users, int64_t N, const void* cand_table,
                               int64_t cand_ld, const float* cand_inv_norm, const int32_t* excl_idx,
                               const int64_t* excl_off, const int32_t* news_time, const int32_t* q_time_lo,
                               const int32_t* q_time_hi, const uint8_t* news_cat, const uint64_t* q_cat_mask,
                               const float* news_prior, const float* user_gain, const float* after_key,
                               const int32_t* after_row, float* next_key, int32_t* next_row, int64_t K,
                               int32_t* top_idx, float* top_scores, float* top_keys, void* ws, int64_t ws_bytes,
                               void* stream) {
  using namespace nr::tk;
  using namespace nr::tk::req;
  const char* fn = "nr_topk_request";
  const ScanArgs a{dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                   {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream, news_prior, user_gain,
                   after_key, after_row};
  // nr_topk_users_after's checks, in its order; the user limit where the shape is judged
  auto k_ok = [&] {
    NR_CHECK_ARG(K >= 1 && K <= KMAX, "%s: K = %lld outside [1, %d]", fn, (long long)K, KMAX);
    return NR_OK;
  };
  auto u_ok = [&] {
    if (U > UMAX) {
      nr::set_error("%s: U = %lld unsupported (at most %d users; nr_topk_users_after takes more)", fn, (long long)U,
                    UMAX);
      return NR_ERR_UNSUPPORTED;
    }
    return NR_OK;
  };
  if (const int rc = check_scan(fn, a, k_ok, u_ok)) return rc;
  NR_CHECK_ARG((after_key == nullptr) == (after_row == nullptr), "%s: after_key and after_row go together", fn);
  NR_CHECK_ARG((next_key == nullptr) == (next_row == nullptr), "%s: next_key and next_row go together", fn);
  NR_CHECK_ARG(top_idx && top_scores && ws, "%s: null pointer", fn);
  const Layout L = layout(U, N, K);
  NR_CHECK_ARG(ws_bytes >= L.total, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes,
               (long long)L.total);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  if (const int rc = check_scan_device(fn, a, "top_idx, top_scores, top_keys, ws", {top_idx, top_scores, top_keys, ws}))
    return rc;
  if (const int rc = nr::check_device_ptrs(fn, "after_key, after_row, next_key, next_row",
                                           {after_key, after_row, next_key, next_row}))
    return rc;

  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  int32_t* cnt = (int32_t*)(w + L.cnt);
  int32_t* uidx = (int32_t*)(w + L.uidx);
  int64_t* coff = (int64_t*)(w + L.coff);
  Pair* part = (Pair*)(w + L.part);
  float* gsel = (float*)(w + L.gsel);
  if (a.prior())
    if (const int rc = prior_gains_launch(U, users, user_gain, gsel, st, fn)) return rc;
  const int rc1 = with_scan_types(a, [&](auto ti, auto filt, auto prior, auto after) {
    using TI = typename decltype(ti)::type;
    auto kernel = request_stage1_kernel<TI, decltype(filt)::value, decltype(prior)::value, decltype(after)::value>;
    const int bytes = lds_bytes<TI>(U);
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
      nr::set_error("%s: hipFuncSetAttribute failed: %s", fn, hipGetErrorString(hipGetLastError()));
      return NR_ERR_HIP;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)L.runs), dim3(256), (size_t)bytes, st, (int)U, N, users,
                       (const TI*)cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off, a.flt, (int)K, run_rows(N),
                       part, PriorArgs{news_prior, gsel}, AfterArgs{after_key, after_row});
    return NR_OK;
  });
  if (rc1) return rc1;
  NR_CHECK_LAUNCH(fn);
  return topk_stage2_launch(fn, a, 1, K, (int)L.runs, part, cnt, uidx, coff, top_idx, top_scores, top_keys, next_key,
                            next_row);
}
