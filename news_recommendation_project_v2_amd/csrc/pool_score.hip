// Fused segmented history pooling + candidate cosine scoring (gfx950).
//
// Replaces, for every impression i of the eval set:
//   get_final_attention_eval   data_model_helper.py:112-131  (padded batches
//       through FinalAttention.forward modeling_utils.py:224-228, or
//       LatentAttentionModel.forward latent_attention.py:165-170)
//   get_cos_sim_scores loop    data_model_helper.py:199-230  (F.cosine_similarity)
//
// The per-item pooler transform is computed once per unique news by the GEMM
// chain (gemm.hip); this kernel only gathers table rows:
//   FINAL : u = sum_j x_j*p_j / (sum_j p_j + 1e-10)     (p = exp(w), per dim)
//   LATENT: u = normalize(sum_j h_j / h_i, eps 1e-12)
//   MEAN  : u = sum_j h_j / h_i            (average_pool, modeling_utils.py:55-59)
//   score_c = (u . e_c) / max(|u|, 1e-8) / max(|e_c|, 1e-8)
//
// Work decomposition: one wave (64 lanes) per impression, 4 impressions per
// 256-thread workgroup.  A table row is D=1024 elements = 16 per lane, read as
// 16-byte lane loads (1 KiB per wave instruction, fully coalesced within the
// row).  Row indices are loaded 64 at a time (one per lane) and broadcast with
// v_readlane, so row addresses are wave-uniform.  Several rows are kept in
// flight per wave (history: 2-4 rows, candidates: 4 rows) to cover gather
// latency; candidate dot products are reduced across the wave 4 at a time with
// a transpose-reduce (7 cross-lane steps for 4 dots instead of 24).
#include "nr_common.h"
#include "../../include/newsrec_sliced.h"

namespace nr {

template <typename T, int DIM>
struct RowFmt {
  static constexpr int VEC = 16 / (int)sizeof(T);  // elements per 16-B load
  static constexpr int NL = DIM / (64 * VEC);       // 16-B loads per lane per row
  static constexpr int EPL = DIM / 64;              // elements per lane
  static_assert(DIM % (64 * VEC) == 0, "DIM must be a multiple of 64*VEC");
};

template <typename T, int DIM>
__device__ __forceinline__ void load_row(const T* __restrict__ row, int lane,
                                         uint4 (&r)[RowFmt<T, DIM>::NL]) {
  const uint4* p = reinterpret_cast<const uint4*>(row) + lane;
#pragma unroll
  for (int j = 0; j < RowFmt<T, DIM>::NL; ++j) r[j] = p[j * 64];
}

template <typename T, int DIM>
__device__ __forceinline__ void unpack_row(const uint4 (&r)[RowFmt<T, DIM>::NL],
                                           float (&v)[RowFmt<T, DIM>::EPL]) {
  constexpr int NL = RowFmt<T, DIM>::NL;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      v[4 * j + 0] = __uint_as_float(r[j].x);
      v[4 * j + 1] = __uint_as_float(r[j].y);
      v[4 * j + 2] = __uint_as_float(r[j].z);
      v[4 * j + 3] = __uint_as_float(r[j].w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      v[8 * j + 0] = bf16_lo(r[j].x);
      v[8 * j + 1] = bf16_hi(r[j].x);
      v[8 * j + 2] = bf16_lo(r[j].y);
      v[8 * j + 3] = bf16_hi(r[j].y);
      v[8 * j + 4] = bf16_lo(r[j].z);
      v[8 * j + 5] = bf16_hi(r[j].z);
      v[8 * j + 6] = bf16_lo(r[j].w);
      v[8 * j + 7] = bf16_hi(r[j].w);
    }
  }
}

// Element index (within the row) of lane-local element i.
template <typename T, int DIM>
__device__ __forceinline__ int elem_pos(int i, int lane) {
  constexpr int VEC = RowFmt<T, DIM>::VEC;
  return (i / VEC) * (64 * VEC) + lane * VEC + (i % VEC);
}

template <typename T, int POOL>
struct PoolCfg;
// rows of history kept in flight per wave: ~16 x 16-B loads per lane
template <> struct PoolCfg<float, NR_POOL_FINAL> { static constexpr int R = 2; };
template <> struct PoolCfg<float, NR_POOL_LATENT> { static constexpr int R = 4; };
template <> struct PoolCfg<__bf16, NR_POOL_FINAL> { static constexpr int R = 4; };
template <> struct PoolCfg<__bf16, NR_POOL_LATENT> { static constexpr int R = 8; };
template <> struct PoolCfg<float, NR_POOL_MEAN> { static constexpr int R = 4; };
template <> struct PoolCfg<__bf16, NR_POOL_MEAN> { static constexpr int R = 8; };

// transpose-reduce of 4 per-lane partial dots; returns the total of dot q in
// lane 16*q (and its 15 neighbours).
__device__ __forceinline__ float reduce4(const float (&d)[4], int lane) {
  const bool hi = lane & 32;
  const float s0 = hi ? d[0] : d[2], s1 = hi ? d[1] : d[3];
  const float k0 = hi ? d[2] : d[0], k1 = hi ? d[3] : d[1];
  const float a0 = k0 + __shfl_xor(s0, 32, 64);
  const float a1 = k1 + __shfl_xor(s1, 32, 64);
  const bool m16 = lane & 16;
  float b = (m16 ? a1 : a0) + __shfl_xor(m16 ? a0 : a1, 16, 64);
  b += __shfl_xor(b, 8, 64);
  b += __shfl_xor(b, 4, 64);
  b += __shfl_xor(b, 2, 64);
  b += __shfl_xor(b, 1, 64);
  return b;
}

// FROM_USERS: the user vector of impression i is row uidx[i] of a table of
// user vectors this kernel wrote earlier (users output of a pooling-only
// launch over the distinct histories), instead of its own history gather; the
// candidate pass is the same code, so the scores are bit-identical.
template <typename T, int POOL, int DIM, bool FROM_USERS = false>
__global__ __launch_bounds__(256) void pool_score_kernel(
    const T* __restrict__ htab, int64_t hld, const T* __restrict__ ctab, int64_t cld,
    const float* __restrict__ cinv, const int32_t* __restrict__ hidx,
    const int64_t* __restrict__ hoff, const int32_t* __restrict__ cidx,
    const int64_t* __restrict__ coff, int64_t n_imp, float* __restrict__ scores,
    float* __restrict__ users, const int32_t* __restrict__ uidx) {
  using F = RowFmt<T, DIM>;
  constexpr int NL = F::NL, EPL = F::EPL;
  constexpr int R = PoolCfg<T, POOL>::R;
  constexpr int G = 4;

  const int lane = threadIdx.x & 63;
  const int64_t imp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (imp >= n_imp) return;  // wave-uniform

  float u[EPL];
  if constexpr (FROM_USERS) {
    const float* ur = users + (int64_t)uidx[imp] * DIM;
#pragma unroll
    for (int i = 0; i < EPL; ++i) u[i] = ur[elem_pos<T, DIM>(i, lane)];
  } else {
  float acc[EPL];
  float den[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) { acc[i] = 0.f; den[i] = 0.f; }

  // ---------------- history pooling ----------------
  const int64_t h0 = hoff[imp], h1 = hoff[imp + 1];
  for (int64_t base = h0; base < h1; base += 64) {
    const int cnt = (int)min((int64_t)64, h1 - base);
    // hidx == nullptr: the segment's rows are consecutive table rows (token pooling)
    const int myidx = lane < cnt ? (hidx ? hidx[base + lane] : (int)(base + lane)) : 0;
    int r = 0;
    for (; r + R <= cnt; r += R) {
      uint4 bx[R][NL];
      uint4 bp[(POOL == NR_POOL_FINAL) ? R : 1][NL];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int row = __builtin_amdgcn_readlane(myidx, r + q);
        const T* p = htab + (int64_t)row * hld;
        load_row<T, DIM>(p, lane, bx[q]);
        if constexpr (POOL == NR_POOL_FINAL) load_row<T, DIM>(p + DIM, lane, bp[q]);
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        float x[EPL];
        unpack_row<T, DIM>(bx[q], x);
        if constexpr (POOL == NR_POOL_FINAL) {
          float pw[EPL];
          unpack_row<T, DIM>(bp[q], pw);
#pragma unroll
          for (int i = 0; i < EPL; ++i) { acc[i] = fmaf(x[i], pw[i], acc[i]); den[i] += pw[i]; }
        } else {
#pragma unroll
          for (int i = 0; i < EPL; ++i) acc[i] += x[i];
        }
      }
    }
    for (; r < cnt; ++r) {
      const int row = __builtin_amdgcn_readlane(myidx, r);
      const T* p = htab + (int64_t)row * hld;
      uint4 bx[NL];
      load_row<T, DIM>(p, lane, bx);
      float x[EPL];
      unpack_row<T, DIM>(bx, x);
      if constexpr (POOL == NR_POOL_FINAL) {
        uint4 bp[NL];
        load_row<T, DIM>(p + DIM, lane, bp);
        float pw[EPL];
        unpack_row<T, DIM>(bp, pw);
#pragma unroll
        for (int i = 0; i < EPL; ++i) { acc[i] = fmaf(x[i], pw[i], acc[i]); den[i] += pw[i]; }
      } else {
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] += x[i];
      }
    }
  }

  // ---------------- user vector ----------------
  if constexpr (POOL == NR_POOL_FINAL) {
    // modeling_utils.py:224-228: w = exp(w)*m; w /= (sum w + 1e-10); sum x*w
#pragma unroll
    for (int i = 0; i < EPL; ++i) u[i] = acc[i] / (den[i] + 1e-10f);
  } else if constexpr (POOL == NR_POOL_MEAN) {
    const float d = (float)(h1 - h0);
#pragma unroll
    for (int i = 0; i < EPL; ++i) u[i] = acc[i] / d;
  } else {
    // latent_attention.py:166-170: s / d, then F.normalize(p=2, eps=1e-12)
    const float d = (float)(h1 - h0);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) { u[i] = acc[i] / d; ss = fmaf(u[i], u[i], ss); }
    const float nrm = sqrtf(wave_sum(ss));
    const float den1 = fmaxf(nrm, 1e-12f);
#pragma unroll
    for (int i = 0; i < EPL; ++i) u[i] = u[i] / den1;
  }
  if (users != nullptr) {
    float* ur = users + imp * DIM;
#pragma unroll
    for (int i = 0; i < EPL; ++i) ur[elem_pos<T, DIM>(i, lane)] = u[i];
  }
  }  // !FROM_USERS
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) ss = fmaf(u[i], u[i], ss);
  const float inv_u = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-8f);

  // ---------------- candidate scoring ----------------
  if (coff == nullptr) return;  // pooling only
  const int64_t c0 = coff[imp], c1 = coff[imp + 1];
  for (int64_t base = c0; base < c1; base += 64) {
    const int cnt = (int)min((int64_t)64, c1 - base);
    const int myidx = lane < cnt ? cidx[base + lane] : 0;
    const float myinv = lane < cnt ? cinv[myidx] : 0.f;
    float mydot = 0.f;
    for (int r = 0; r < cnt; r += G) {
      uint4 bc[G][NL];
#pragma unroll
      for (int q = 0; q < G; ++q) {
        const int rr = min(r + q, cnt - 1);
        const int row = __builtin_amdgcn_readlane(myidx, rr);
        load_row<T, DIM>(ctab + (int64_t)row * cld, lane, bc[q]);
      }
      float d[G];
#pragma unroll
      for (int q = 0; q < G; ++q) {
        float e[EPL];
        unpack_row<T, DIM>(bc[q], e);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < EPL; ++i) s = fmaf(u[i], e[i], s);
        d[q] = s;
      }
      const float b = reduce4(d, lane);
#pragma unroll
      for (int q = 0; q < G; ++q) {
        const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 16 * q));
        if (lane == r + q) mydot = t;
      }
    }
    if (lane < cnt) scores[base + lane] = mydot * inv_u * myinv;
  }
}

template <typename T, int POOL, bool FROM_USERS = false>
static int launch_pool_score(const void* ht, int64_t hld, const void* ct, int64_t cld,
                             const float* cinv, const int32_t* hidx, const int64_t* hoff,
                             const int32_t* cidx, const int64_t* coff, int64_t n_imp,
                             float* scores, float* users, hipStream_t s, const int32_t* uidx = nullptr) {
  const int64_t blocks = (n_imp + 3) / 4;
  hipLaunchKernelGGL((pool_score_kernel<T, POOL, 1024, FROM_USERS>), dim3((unsigned)blocks), dim3(256), 0, s,
                     (const T*)ht, hld, (const T*)ct, cld, cinv, hidx, hoff, cidx, coff, n_imp,
                     scores, users, uidx);
  NR_CHECK_LAUNCH("nr_pool_score");
  return NR_OK;
}

// Pooling only (no candidates) of consecutive rows: segment i = table rows
// off[i] .. off[i+1]-1, u written to users [n_seg][1024] f32.
int pool_rows_dispatch(int pooler, int dtype, const void* table, int64_t ld, const int64_t* off, int64_t n_seg,
                       float* users, hipStream_t s) {
  if (n_seg == 0) return NR_OK;
  return with_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    const auto miss = [&] { return unvalidated_code("pooler", pooler); };
    return with_int<NR_POOL_MEAN, NR_POOL_LATENT>(pooler, miss, [&](auto pool) -> int {
      return launch_pool_score<T, decltype(pool)::value>(table, ld, table, ld, nullptr, nullptr, off, nullptr, nullptr,
                                                         n_seg, nullptr, users, s);
    });
  });
}

// The evaluation path's candidate scoring over stored user rows (nr_score_users, and
// the exact re-score of nr_topk_users' survivors): impression i scores candidates
// cand_idx[cand_off[i] .. cand_off[i+1]) against users[user_idx[i]].
int score_users_dispatch(int dtype, const float* users, const int32_t* user_idx, const void* cand_table,
                         int64_t cand_ld, const float* cand_inv_norm, const int32_t* cand_idx,
                         const int64_t* cand_off, int64_t n_imp, float* scores, hipStream_t s) {
  // the pooler only shaped the stored user vectors; the scoring pass is pooler-independent
  return with_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    return launch_pool_score<T, NR_POOL_MEAN, true>(nullptr, 0, cand_table, cand_ld, cand_inv_norm, nullptr, nullptr,
                                                    cand_idx, cand_off, n_imp, scores, const_cast<float*>(users), s,
                                                    user_idx);
  });
}

}  // namespace nr

extern "C" int nr_pool_score(int pooler, int dtype, int64_t dim, const void* hist_table,
                             int64_t hist_ld, const void* cand_table, int64_t cand_ld,
                             const float* cand_inv_norm, const int32_t* hist_idx,
                             const int64_t* hist_off, const int32_t* cand_idx,
                             const int64_t* cand_off, int64_t n_imp, float* scores,
                             float* users, void* stream) {
  nr::clear_error();
  if (dim != 1024) {
    nr::set_error("nr_pool_score: dim %lld unsupported (1024 only)", (long long)dim);
    return NR_ERR_UNSUPPORTED;
  }
  NR_CHECK_ARG(pooler == NR_POOL_FINAL || pooler == NR_POOL_LATENT || pooler == NR_POOL_MEAN,
               "nr_pool_score: bad pooler %d", pooler);
  NR_CHECK_ARG(nr::ok_dtype(dtype), "nr_pool_score: bad dtype %d", dtype);
  NR_CHECK_ARG(n_imp >= 0, "nr_pool_score: n_imp < 0");
  if (n_imp == 0) return NR_OK;
  const bool score = cand_off != nullptr;
  NR_CHECK_ARG(hist_table && hist_off && (score || users), "nr_pool_score: null pointer");
  NR_CHECK_ARG(!score || (cand_table && cand_inv_norm && cand_idx && scores), "nr_pool_score: null candidate pointer");
  NR_CHECK_DEVICE("nr_pool_score", hist_table, cand_table, cand_inv_norm, hist_idx, hist_off, cand_idx, cand_off,
                  scores, users);
  if (!score) {
    cand_table = hist_table;
    cand_ld = hist_ld;
  }
  const int64_t min_hld = pooler == NR_POOL_FINAL ? 2 * dim : dim;
  NR_CHECK_ARG(hist_ld >= min_hld && cand_ld >= dim, "nr_pool_score: leading dimension too small");
  const int64_t align = dtype == NR_F32 ? 4 : 8;
  NR_CHECK_ARG(hist_ld % align == 0 && cand_ld % align == 0 &&
                   ((uintptr_t)hist_table & 15) == 0 && ((uintptr_t)cand_table & 15) == 0,
               "nr_pool_score: tables must be 16-byte aligned with 16-byte row strides");
  hipStream_t s = (hipStream_t)stream;
  return nr::with_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    const auto miss = [&] { return nr::unvalidated_code("pooler", pooler); };
    return nr::with_int<NR_POOL_MEAN, NR_POOL_FINAL, NR_POOL_LATENT>(pooler, miss, [&](auto pool) -> int {
      return nr::launch_pool_score<T, decltype(pool)::value>(hist_table, hist_ld, cand_table, cand_ld, cand_inv_norm,
                                                             hist_idx, hist_off, cand_idx, cand_off, n_imp, scores,
                                                             users, s);
    });
  });
}

extern "C" int nr_score_users(int dtype, int64_t dim, const float* users, const int32_t* user_idx,
                              const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                              const int32_t* cand_idx, const int64_t* cand_off, int64_t n_imp, float* scores,
                              void* stream) {
  nr::clear_error();
  if (dim != 1024) {
    nr::set_error("nr_score_users: dim %lld unsupported (1024 only)", (long long)dim);
    return NR_ERR_UNSUPPORTED;
  }
  NR_CHECK_ARG(nr::ok_dtype(dtype), "nr_score_users: bad dtype %d", dtype);
  NR_CHECK_ARG(n_imp >= 0, "nr_score_users: n_imp < 0");
  if (n_imp == 0) return NR_OK;
  NR_CHECK_ARG(users && user_idx && cand_table && cand_inv_norm && cand_idx && cand_off && scores,
               "nr_score_users: null pointer");
  NR_CHECK_DEVICE("nr_score_users", users, user_idx, cand_table, cand_inv_norm, cand_idx, cand_off, scores);
  NR_CHECK_ARG(cand_ld >= dim && cand_ld % (dtype == NR_F32 ? 4 : 8) == 0 && ((uintptr_t)cand_table & 15) == 0,
               "nr_score_users: cand_table must be 16-byte aligned with 16-byte row strides");
  return nr::score_users_dispatch(dtype, users, user_idx, cand_table, cand_ld, cand_inv_norm, cand_idx, cand_off, n_imp,
                                  scores, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// Column-sliced pool+score (nr_slice_table, nr_pool_score_sliced).
//
// Pooling is a per-column sum and a dot product is a sum over columns, so the
// pass can be cut by columns: the tables are kept as S = 1024 / W dense
// slice images [S][N][W] (nr_slice_table), and the whole chip works on about
// one slice at a time (slice-major blockIdx).  One slice of a table is N * W
// elements instead of N * 1024, so an XCD's L2 holds 1024 / W times as large
// a share of what is being gathered.
//
// A slice row is W * sizeof(T) bytes = L lanes of 16 bytes, so one wave
// instruction fetches 64 / L rows with per-lane addresses.  One wave works on
// one impression at a time (kSlicedIpw consecutive impressions per wave); the
// 64 / L row slots of an instruction hold different rows of that impression.
//   pool    : per (slice, impression) the W pooled columns, f32, into
//             u [I][1024], and the slice's sum of squares into usq [S][I]
//   score   : per (slice, impression) the partial dots into part [S][C]
//   finalize: per impression, the S partials of each candidate added in slice
//             order, the norm clamps of pool_score_kernel, cand_inv
// No atomics: every value has one writer and the sums have a fixed order.
namespace nr {

constexpr int kSlicedIpw = 8;  // consecutive impressions per wave

template <typename T, int W>
struct SliceFmt {
  static constexpr int VEC = 16 / (int)sizeof(T);  // elements per lane
  static constexpr int L = W / VEC;                // lanes per slice row
  static constexpr int RPI = 64 / L;               // rows per wave instruction
  // wave load instructions in flight: 32 rows (about a MIND history), 8 instructions at most
  static constexpr int R = RPI >= 4 ? 32 / RPI : 8;
  static_assert(W % VEC == 0 && 64 % L == 0 && L >= 1 && L <= 64, "slice width");
};

template <typename T>
__device__ __forceinline__ void unpack16(const uint4& r, float (&v)[16 / sizeof(T)]) {
  if constexpr (sizeof(T) == 4) {
    v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y);
    v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
  } else {
    v[0] = bf16_lo(r.x); v[1] = bf16_hi(r.x); v[2] = bf16_lo(r.y); v[3] = bf16_hi(r.y);
    v[4] = bf16_lo(r.z); v[5] = bf16_hi(r.z); v[6] = bf16_lo(r.w); v[7] = bf16_hi(r.w);
  }
}

// index / offset / partial streams: read once per slice, kept out of the slice's way in L2
template <typename V>
__device__ __forceinline__ V nt_load(const V* p) { return __builtin_nontemporal_load(p); }

// a wave-uniform value the compiler sees in vector registers, moved to scalar ones
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Row-major [n][parts * 1024] (row stride ld) <-> [S][n][parts * W]: 16 bytes per thread.
// Slice s of row r holds, part after part, columns s * W .. s * W + W - 1 of that part.
template <int ES>
__global__ __launch_bounds__(256) void slice_table_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          int64_t n, int64_t ld16, int parts, int W, bool inverse) {
  const int per_part = 1024 * ES / 16, per_w = W * ES / 16;
  const int per_row = parts * per_part;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * per_row) return;
  const int64_t r = t / per_row;
  const int c = (int)(t % per_row);
  const int p = c / per_part, cc = c % per_part;
  const int s = cc / per_w, w = cc % per_w;
  const int64_t rm = r * ld16 + c;
  const int64_t sm = ((int64_t)s * n + r) * (parts * per_w) + p * per_w + w;
  if (inverse) dst[rm] = src[sm];
  else dst[sm] = src[rm];
}

// The CSR offsets of a wave's n <= kSlicedIpw impressions, one vector load: lane l holds
// off[i0 + min(l, n)], read back with a wave-uniform lane number.
struct WaveOffsets {
  int64_t mine;
  __device__ __forceinline__ WaveOffsets(const int64_t* off, int64_t i0, int n, int lane)
      : mine(nt_load(off + i0 + min(lane, n))) {}
  __device__ __forceinline__ int64_t operator[](int k) const {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)mine, k);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)mine >> 32), k);
    return (int64_t)(((uint64_t)hi << 32) | lo);
  }
};

// The rows of the R instructions that start at `base` of a segment ending at `end`: an
// instruction wholly past the segment is skipped (wave-uniform); a lane past it in the
// last one reads the segment's last row again (and its value is dropped).
template <int R, int RPI>
__device__ __forceinline__ void load_rows_idx(const int32_t* __restrict__ idx, int64_t base, int64_t end, int g,
                                              int32_t (&row)[R]) {
#pragma unroll
  for (int q = 0; q < R; ++q) {
    row[q] = 0;
    if (base + q * RPI < end) row[q] = nt_load(idx + min(base + q * RPI + g, end - 1));
  }
}

template <typename T, int POOL, int W>
__global__ __launch_bounds__(256) void sliced_pool_kernel(const T* __restrict__ himg, int64_t n_rows,
                                                          const int32_t* __restrict__ hidx,
                                                          const int64_t* __restrict__ hoff, int64_t n_imp,
                                                          int64_t waves_per_slice, float* __restrict__ u_out,
                                                          float* __restrict__ usq) {
  using F = SliceFmt<T, W>;
  constexpr int VEC = F::VEC, L = F::L, RPI = F::RPI, R = F::R;
  constexpr bool FINAL = POOL == NR_POOL_FINAL;
  constexpr int RW = FINAL ? 2 * W : W;  // elements of one image row
  const int lane = threadIdx.x & 63;
  const int g = lane / L, c = lane % L;
  const int64_t wv = uniform64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
  const int64_t s = wv / waves_per_slice, w = wv % waves_per_slice;
  if (s >= 1024 / W) return;  // the last workgroup's spare waves
  const T* img = himg + s * n_rows * RW + c * VEC;
  const int64_t i0 = w * kSlicedIpw;
  const int n = (int)min((int64_t)kSlicedIpw, n_imp - i0);  // >= 1
  const WaveOffsets off(hoff, i0, n, lane);
  // the first instructions' rows of impression k + 1 are asked for before impression k's
  // rows are, so a wave's row loads do not wait for an index round trip per impression
  int32_t nxt[R];
  int64_t h0 = off[0];
  load_rows_idx<R, RPI>(hidx, h0, off[1], g, nxt);
  for (int k = 0; k < n; ++k) {  // wave-uniform
    const int64_t h1 = off[k + 1];
    int32_t row[R];
#pragma unroll
    for (int q = 0; q < R; ++q) row[q] = nxt[q];
    if (k + 1 < n) load_rows_idx<R, RPI>(hidx, h1, off[k + 2], g, nxt);
    float acc[VEC], den[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { acc[i] = 0.f; den[i] = 0.f; }
    for (int64_t base = h0; base < h1; base += RPI * R) {
      if (base != h0) load_rows_idx<R, RPI>(hidx, base, h1, g, row);
      uint4 bx[R], bp[FINAL ? R : 1];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        bx[q] = make_uint4(0, 0, 0, 0);
        if constexpr (FINAL) bp[q] = make_uint4(0, 0, 0, 0);
        if (base + q * RPI < h1) {
          const T* p = img + (int64_t)row[q] * RW;
          bx[q] = *reinterpret_cast<const uint4*>(p);
          if constexpr (FINAL) bp[q] = *reinterpret_cast<const uint4*>(p + W);
        }
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (base + q * RPI + g >= h1) {
          bx[q] = make_uint4(0, 0, 0, 0);
          if constexpr (FINAL) bp[q] = make_uint4(0, 0, 0, 0);
        }
        float x[VEC];
        unpack16<T>(bx[q], x);
        if constexpr (FINAL) {
          float pw[VEC];
          unpack16<T>(bp[q], pw);
#pragma unroll
          for (int i = 0; i < VEC; ++i) { acc[i] = fmaf(x[i], pw[i], acc[i]); den[i] += pw[i]; }
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += x[i];
        }
      }
    }
    // the row slots' sums, added in a fixed tree
#pragma unroll
    for (int m = L; m < 64; m <<= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        acc[i] += __shfl_xor(acc[i], m, 64);
        if constexpr (FINAL) den[i] += __shfl_xor(den[i], m, 64);
      }
    }
    float u[VEC], ss = 0.f;
    const float d = (float)(h1 - h0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      u[i] = FINAL ? acc[i] / (den[i] + 1e-10f) : acc[i] / d;
      ss = fmaf(u[i], u[i], ss);
    }
#pragma unroll
    for (int m = 1; m < L; m <<= 1) ss += __shfl_xor(ss, m, 64);
    if (g == 0) {
      const int64_t imp = i0 + k;
      float* up = u_out + imp * 1024 + s * W + c * VEC;
#pragma unroll
      for (int i = 0; i < VEC; i += 4) *reinterpret_cast<float4*>(up + i) = make_float4(u[i], u[i + 1], u[i + 2], u[i + 3]);
      if (c == 0) usq[s * n_imp + imp] = ss;
    }
    h0 = h1;
  }
}

template <typename T, int W>
__global__ __launch_bounds__(256) void sliced_score_kernel(const T* __restrict__ cimg, int64_t n_rows,
                                                           const int32_t* __restrict__ cidx,
                                                           const int64_t* __restrict__ coff, int64_t n_imp,
                                                           int64_t n_cand, int64_t waves_per_slice,
                                                           const float* __restrict__ u_in, float* __restrict__ part) {
  using F = SliceFmt<T, W>;
  constexpr int VEC = F::VEC, L = F::L, RPI = F::RPI, R = F::R;
  const int lane = threadIdx.x & 63;
  const int g = lane / L, c = lane % L;
  const int64_t wv = uniform64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
  const int64_t s = wv / waves_per_slice, w = wv % waves_per_slice;
  if (s >= 1024 / W) return;  // the last workgroup's spare waves
  const T* img = cimg + s * n_rows * W + c * VEC;
  float* out = part + s * n_cand;
  const int64_t i0 = w * kSlicedIpw;
  const int n = (int)min((int64_t)kSlicedIpw, n_imp - i0);  // >= 1
  const WaveOffsets off(coff, i0, n, lane);
  int32_t nxt[R];
  int64_t c0 = off[0];
  load_rows_idx<R, RPI>(cidx, c0, off[1], g, nxt);
  for (int k = 0; k < n; ++k) {  // wave-uniform
    const int64_t c1 = off[k + 1];
    int32_t row[R];
#pragma unroll
    for (int q = 0; q < R; ++q) row[q] = nxt[q];
    if (k + 1 < n) load_rows_idx<R, RPI>(cidx, c1, off[k + 2], g, nxt);
    float u[VEC];
    const float* up = u_in + (i0 + k) * 1024 + s * W + c * VEC;
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      const f32x4 v = nt_load(reinterpret_cast<const f32x4*>(up + i));
      u[i] = v[0]; u[i + 1] = v[1]; u[i + 2] = v[2]; u[i + 3] = v[3];
    }
    for (int64_t base = c0; base < c1; base += RPI * R) {
      if (base != c0) load_rows_idx<R, RPI>(cidx, base, c1, g, row);
      uint4 bc[R];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        bc[q] = make_uint4(0, 0, 0, 0);
        if (base + q * RPI < c1) bc[q] = *reinterpret_cast<const uint4*>(img + (int64_t)row[q] * W);
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (base + q * RPI >= c1) break;  // wave-uniform
        float e[VEC];
        unpack16<T>(bc[q], e);
        float dsum = 0.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) dsum = fmaf(u[i], e[i], dsum);
#pragma unroll
        for (int m = 1; m < L; m <<= 1) dsum += __shfl_xor(dsum, m, 64);
        const int64_t j = base + q * RPI + g;
        if (c == 0 && j < c1) out[j] = dsum;
      }
    }
    c0 = c1;
  }
}

template <int POOL, int S>
__global__ __launch_bounds__(256) void sliced_finalize_kernel(const float* __restrict__ part,
                                                              const float* __restrict__ usq,
                                                              const float* __restrict__ cinv,
                                                              const int32_t* __restrict__ cidx,
                                                              const int64_t* __restrict__ coff, int64_t n_imp,
                                                              int64_t n_cand, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t imp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (imp >= n_imp) return;  // wave-uniform
  const int64_t c0 = coff[imp], c1 = coff[imp + 1];
  if (c0 >= c1) return;
  // The S partials are added in f64 (16 or 8 adds per candidate, in slice order) and the
  // factors applied there, so the slicing adds one rounding to a score, not S of them.
  double ss = 0.0;
  float sq[S];
#pragma unroll
  for (int s = 0; s < S; ++s) sq[s] = usq[(int64_t)s * n_imp + imp];
#pragma unroll
  for (int s = 0; s < S; ++s) ss += (double)sq[s];
  double k;
  if constexpr (POOL == NR_POOL_LATENT) {
    // u_n = u / max(|u|, 1e-12); score = (u_n . e) / max(|u_n|, 1e-8)
    const double nrm = sqrt(ss), den1 = fmax(nrm, 1e-12);
    k = 1.0 / den1 / fmax(nrm / den1, 1e-8);
  } else {
    k = 1.0 / fmax(sqrt(ss), 1e-8);
  }
  for (int64_t j = c0 + lane; j < c1; j += 64) {
    float pd[S];
#pragma unroll
    for (int s = 0; s < S; ++s) pd[s] = nt_load(part + (int64_t)s * n_cand + j);
    double dsum = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) dsum += (double)pd[s];
    scores[j] = (float)(dsum * k * (double)cinv[cidx[j]]);
  }
}

static inline int64_t sliced_waves_per_slice(int64_t n_imp) { return (n_imp + kSlicedIpw - 1) / kSlicedIpw; }

// workspace: u f32 [I][1024] | usq f32 [S][I] | part f32 [S][C], each padded to 256 bytes
static inline int64_t sliced_ws_bytes(int W, int64_t n_imp, int64_t n_cand, int64_t* o_usq = nullptr,
                                      int64_t* o_part = nullptr) {
  const int64_t S = 1024 / W;
  const int64_t a = align256(n_imp * 1024 * 4), b = align256(S * n_imp * 4), c = align256(S * n_cand * 4);
  if (o_usq) *o_usq = a;
  if (o_part) *o_part = a + b;
  return a + b + c;
}

template <typename T, int POOL, int W>
static int launch_sliced(const void* himg, const void* cimg, int64_t n_hist_rows, int64_t n_cand_rows,
                         const float* cinv, const int32_t* hidx, const int64_t* hoff, const int32_t* cidx,
                         const int64_t* coff, int64_t n_imp, int64_t n_cand, float* scores, char* ws,
                         hipStream_t st) {
  constexpr int S = 1024 / W;
  int64_t o_usq, o_part;
  sliced_ws_bytes(W, n_imp, n_cand, &o_usq, &o_part);
  float* u = reinterpret_cast<float*>(ws);
  float* usq = reinterpret_cast<float*>(ws + o_usq);
  float* part = reinterpret_cast<float*>(ws + o_part);
  const int64_t wps = sliced_waves_per_slice(n_imp);
  const int64_t blocks = (wps * S + 3) / 4;
  NR_CHECK_ARG(blocks <= 0x7fffffff, "nr_pool_score_sliced: too many impressions");
  hipLaunchKernelGGL((sliced_pool_kernel<T, POOL, W>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)himg,
                     n_hist_rows, hidx, hoff, n_imp, wps, u, usq);
  NR_CHECK_LAUNCH("nr_pool_score_sliced");
  if (n_cand > 0) {
    hipLaunchKernelGGL((sliced_score_kernel<T, W>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)cimg,
                       n_cand_rows, cidx, coff, n_imp, n_cand, wps, u, part);
    NR_CHECK_LAUNCH("nr_pool_score_sliced");
    hipLaunchKernelGGL((sliced_finalize_kernel<POOL, S>), dim3((unsigned)((n_imp + 3) / 4)), dim3(256), 0, st, part, usq,
                       cinv, cidx, coff, n_imp, n_cand, scores);
    NR_CHECK_LAUNCH("nr_pool_score_sliced");
  }
  return NR_OK;
}

}  // namespace nr

extern "C" int nr_slice_table(int dtype, int64_t n_rows, int parts, int slice_w, const void* src, int64_t ld,
                              void* dst, int inverse, void* stream) {
  nr::clear_error();
  NR_CHECK_ARG(nr::ok_dtype(dtype), "nr_slice_table: bad dtype %d", dtype);
  NR_CHECK_ARG(parts == 1 || parts == 2, "nr_slice_table: parts %d (1 or 2)", parts);
  NR_CHECK_ARG(slice_w == 64 || slice_w == 128, "nr_slice_table: slice width %d (64 or 128)", slice_w);
  NR_CHECK_ARG(n_rows >= 0, "nr_slice_table: n_rows < 0");
  if (n_rows == 0) return NR_OK;
  NR_CHECK_ARG(src && dst, "nr_slice_table: null pointer");
  NR_CHECK_DEVICE("nr_slice_table", src, dst);
  // ld is the row stride of the ROW-MAJOR side: src, or dst with `inverse`
  const int64_t align = dtype == NR_F32 ? 4 : 8;
  NR_CHECK_ARG(ld >= (int64_t)parts * 1024 && ld % align == 0 && ((uintptr_t)src & 15) == 0 &&
                   ((uintptr_t)dst & 15) == 0,
               "nr_slice_table: tables must be 16-byte aligned, the row-major one with a 16-byte row stride of at "
               "least parts * 1024");
  const int es = dtype == NR_F32 ? 4 : 2;
  const int64_t total = n_rows * parts * (1024 * es / 16);
  const int64_t blocks = (total + 255) / 256;
  NR_CHECK_ARG(blocks <= 0x7fffffff, "nr_slice_table: table too large");
  hipStream_t s = (hipStream_t)stream;
  if (es == 4)
    hipLaunchKernelGGL((nr::slice_table_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint4*)src,
                       (uint4*)dst, n_rows, ld * es / 16, parts, slice_w, inverse != 0);
  else
    hipLaunchKernelGGL((nr::slice_table_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint4*)src,
                       (uint4*)dst, n_rows, ld * es / 16, parts, slice_w, inverse != 0);
  NR_CHECK_LAUNCH("nr_slice_table");
  return NR_OK;
}

extern "C" int64_t nr_pool_score_sliced_workspace_bytes(int slice_w, int64_t n_imp, int64_t n_cand) {
  nr::clear_error();
  if ((slice_w != 64 && slice_w != 128) || n_imp < 0 || n_cand < 0) {
    nr::set_error("nr_pool_score_sliced_workspace_bytes: slice width 64 or 128, n_imp and n_cand >= 0");
    return NR_ERR_INVALID;
  }
  return nr::sliced_ws_bytes(slice_w, n_imp, n_cand);
}

extern "C" int nr_pool_score_sliced(int pooler, int dtype, int64_t dim, int slice_w, const void* hist_image,
                                    int64_t n_hist_rows, const void* cand_image, int64_t n_cand_rows,
                                    const float* cand_inv_norm, const int32_t* hist_idx, const int64_t* hist_off,
                                    const int32_t* cand_idx, const int64_t* cand_off, int64_t n_imp, int64_t n_cand,
                                    float* scores, void* workspace, int64_t workspace_bytes, void* stream) {
  nr::clear_error();
  if (dim != 1024) {
    nr::set_error("nr_pool_score_sliced: dim %lld unsupported (1024 only)", (long long)dim);
    return NR_ERR_UNSUPPORTED;
  }
  NR_CHECK_ARG(pooler == NR_POOL_FINAL || pooler == NR_POOL_LATENT || pooler == NR_POOL_MEAN,
               "nr_pool_score_sliced: bad pooler %d", pooler);
  NR_CHECK_ARG(nr::ok_dtype(dtype), "nr_pool_score_sliced: bad dtype %d", dtype);
  NR_CHECK_ARG(slice_w == 64 || slice_w == 128, "nr_pool_score_sliced: slice width %d (64 or 128)", slice_w);
  NR_CHECK_ARG(n_imp >= 0 && n_cand >= 0, "nr_pool_score_sliced: n_imp or n_cand < 0");
  if (n_imp == 0) return NR_OK;
  NR_CHECK_ARG(hist_image && hist_idx && hist_off && cand_off && workspace, "nr_pool_score_sliced: null pointer");
  NR_CHECK_ARG(n_cand == 0 || (cand_image && cand_inv_norm && cand_idx && scores),
               "nr_pool_score_sliced: null candidate pointer");
  NR_CHECK_ARG(n_hist_rows > 0 && (n_cand == 0 || n_cand_rows > 0), "nr_pool_score_sliced: empty table");
  NR_CHECK_DEVICE("nr_pool_score_sliced", hist_image, cand_image, cand_inv_norm, hist_idx, hist_off, cand_idx,
                  cand_off, scores, workspace);
  NR_CHECK_ARG(((uintptr_t)hist_image & 15) == 0 && ((uintptr_t)cand_image & 15) == 0 &&
                   ((uintptr_t)workspace & 15) == 0,
               "nr_pool_score_sliced: images and workspace must be 16-byte aligned");
  NR_CHECK_ARG(workspace_bytes >= nr::sliced_ws_bytes(slice_w, n_imp, n_cand),
               "nr_pool_score_sliced: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)nr::sliced_ws_bytes(slice_w, n_imp, n_cand));
  hipStream_t s = (hipStream_t)stream;
  return nr::with_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    const auto miss = [&] { return nr::unvalidated_code("pooler", pooler); };
    return nr::with_int<NR_POOL_MEAN, NR_POOL_FINAL, NR_POOL_LATENT>(pooler, miss, [&](auto pool) -> int {
      const auto missw = [&] { return nr::unvalidated_code("slice width", slice_w); };
      return nr::with_int<64, 128>(slice_w, missw, [&](auto w) -> int {
        return nr::launch_sliced<T, decltype(pool)::value, decltype(w)::value>(
            hist_image, cand_image, n_hist_rows, n_cand_rows, cand_inv_norm, hist_idx, hist_off, cand_idx, cand_off,
            n_imp, n_cand, scores, (char*)workspace, s);
      });
    });
  });
}
