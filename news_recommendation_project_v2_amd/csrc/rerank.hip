// Greedy MMR re-ranking of retrieved news lists (include/newsrec_rerank.h): per user the
// M x M cosines between its M <= 64 listed table rows, then K dependent selection rounds.
//
//   grid     a fixed number of workgroups (3 per CU) walking users with a stride, 256 threads.
//   gather   the M rows in 256-byte column slices through a two-stage LDS ring (272-byte row
//            stride: conflict-free b128 fragment reads), 4 x 16 B per thread and slice, the next
//            slice's global loads in flight over the MFMAs; one barrier per slice.  A pad's
//            row is zeros in LDS and is never read from the table.
//   product  A and B fragments come from the SAME slice (the rows are loaded once).  Waves
//            1, 2, 3 accumulate the 32 x 32 quadrants (0,0), (0,1), (1,1) (f32 on
//            v_mfma_f32_32x32x2_f32, bf16 on v_mfma_f32_32x32x16_bf16: one f32x16 each);
//            quadrant (1,0) is the mirror of (0,1) and is not computed; (0,1) and (1,1) are
//            skipped when M <= 32.  A pair's value is taken from the position i < j, scaled
//            (dot * inv[i]) * inv[j] and written to S[i][j] and S[j][i] of a 64 x 65 f32
//            matrix in LDS: symmetric bit for bit, diagonal and pads 0.
//   select   wave 0 (it has no quadrant), lane i owning entry i: K rounds of a wave arg-max
//            (value descending, position ascending), then ms_i = max(ms_i, S[i][picked]);
//            the diversity figures from the same S.  The next user's lists and its first
//            slice are requested before the rounds start, so they land over them.
//
// 34 KiB ring + 16.25 KiB matrix + 0.5 KiB = 50.75 KiB of LDS: three workgroups per CU.
#include "nr_common.h"

#include "../../include/newsrec_rerank.h"

namespace nr {
namespace rr {

constexpr int64_t D = 1024;
constexpr int MMAX = NR_RERANK_MAX;
constexpr int ROWW = 68;                    // LDS words per staged 256-byte row slice (272 B)
constexpr int STAGE_WORDS = MMAX * ROWW;
constexpr int SLD = 65;                     // similarity matrix row stride, floats
constexpr int kWorkgroupsPerCU = 3;
static_assert((2 * STAGE_WORDS + MMAX * SLD + 2 * MMAX) * 4 * kWorkgroupsPerCU <= 160 * 1024, "three workgroups per CU");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename TI>
__global__ __launch_bounds__(256) void rerank_mmr_kernel(int64_t U, int64_t N, const TI* __restrict__ tab, int64_t ldt,
                                                         const float* __restrict__ cinv,
                                                         const int32_t* __restrict__ list_idx,
                                                         const float* __restrict__ list_rel, int M, int K, float lam,
                                                         float oml, int32_t* __restrict__ out_idx,
                                                         float* __restrict__ out_rel, int32_t* __restrict__ out_pos,
                                                         float* __restrict__ out_ild, float* __restrict__ sim_out) {
  // No contraction: obj = lam * rel - oml * ms is two rounded products and a rounded
  // difference wherever it is evaluated (include/newsrec_rerank.h, "Selection").
#pragma clang fp contract(off)
  constexpr int NKT = (int)(D * sizeof(TI) / 256);  // 256-byte slices per row (even: a user starts on ring stage 0)
  __shared__ __attribute__((aligned(16))) uint32_t ring[2 * STAGE_WORDS];
  __shared__ float S[MMAX * SLD];
  __shared__ float cinv_s[2][MMAX];  // by user parity: the next user's are written over this one's epilogue

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NINF = -__builtin_inff();
  // quadrant of this wave: (qi, qj) row blocks of 32; wave 0 has none
  const int qi = wave == 3 ? 1 : 0, qj = wave >= 2 ? 1 : 0;
  const bool has_quad = wave >= 1 && (M > 32 || wave == 1);

  // staging map: 4 chunks of 16 B per thread and slice; chunk (row, c) = (id >> 4, id & 15)
  const u32x4* g[4];
  u32x4 rg[4];
  int soff[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) soff[p] = ((tid >> 4) + 16 * p) * ROWW + (tid & 15) * 4;
  // wave 0, lane i: entry i of the user being prepared
  int32_t n_idx = -1;
  float n_rel = NINF;
  bool n_valid = false;

  auto prepare = [&](int64_t u, int par) __attribute__((always_inline)) {
    const int32_t* li = list_idx + u * M;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = (tid >> 4) + 16 * p;
      const int32_t ix = row < M ? li[row] : -1;
      g[p] = ix >= 0 && ix < N ? reinterpret_cast<const u32x4*>(tab + (int64_t)ix * ldt) + (tid & 15) : nullptr;
    }
    if (wave == 0) {
      n_idx = lane < M ? li[lane] : -1;
      n_valid = n_idx >= 0 && n_idx < N;
      n_rel = lane < M ? list_rel[u * M + lane] : NINF;
      cinv_s[par][lane] = n_valid ? cinv[n_idx] : 0.f;
    }
  };
  auto gload = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p) rg[p] = g[p] ? g[p][kt * 16] : (u32x4)0u;
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p) *reinterpret_cast<u32x4*>(ring + buf * STAGE_WORDS + soff[p]) = rg[p];
  };

  int par = 0;
  int64_t u = blockIdx.x;
  if (u < U) {
    prepare(u, par);
    gload(0);
  }
  for (; u < U; u += gridDim.x) {
    const int32_t idx = n_idx;
    const float rel = n_rel;
    const bool valid = n_valid;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int fr = lane & 31, fh = lane >> 5;
    for (int kt = 0; kt < NKT; ++kt) {
      const int cur = kt & 1;
      lstore(cur);
      __syncthreads();  // (the stage written next was last read before the previous barrier)
      if (kt + 1 < NKT) gload(kt + 1);
      if (has_quad) {
        const uint32_t* ra = ring + cur * STAGE_WORDS + (32 * qi + fr) * ROWW;
        const uint32_t* rb = ring + cur * STAGE_WORDS + (32 * qj + fr) * ROWW;
        if constexpr (sizeof(TI) == 4) {
          // lane (r, h) covers k = 32 h + 4 q + t of the 64-deep slice (both operands alike)
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(ra + 32 * fh + 4 * q);
            const f32x4 b = *reinterpret_cast<const f32x4*>(rb + 32 * fh + 4 * q);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
          }
        } else {
          // lane (r, h) holds k = 16 s + 8 h + j, j < 8, of row r (32x32x16 operand map)
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(ra + 8 * s + 4 * fh);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(rb + 8 * s + 4 * fh);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
          }
        }
      }
    }
    // ---- the scaled matrix.  C/D map: col (j) = lane & 31, row (i) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    if (has_quad) {
      const int j = 32 * qj + (lane & 31);
      const float cj = cinv_s[par][j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = 32 * qi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (i < j) {
          const float ci = cinv_s[par][i];
          const float v = ci == 0.f || cj == 0.f ? 0.f : (acc[r] * ci) * cj;  // a pad's inverse norm is 0
          S[i * SLD + j] = v;
          S[j * SLD + i] = v;
        } else if (i == j) {
          S[i * SLD + i] = 0.f;
        }
      }
    }
    // the next user's lists and first slice: in flight over the selection
    const int64_t un = u + gridDim.x;
    if (un < U) {
      prepare(un, par ^ 1);
      gload(0);
    }
    __syncthreads();
    if (sim_out) {
      float* so = sim_out + u * M * M;
      for (int e = tid; e < M * M; e += 256) {
        const int i = e / M;
        so[e] = S[i * SLD + (e - i * M)];
      }
    }
    if (wave == 0) {
      float ms = NINF;
      bool chosen = false;
      int32_t o_idx = -1, o_pos = -1;
      float o_rel = NINF;
      for (int t = 0; t < K; ++t) {
        const bool cand = valid && !chosen;
        const float key = t == 0 ? rel : lam * rel - oml * ms;
        float bv = cand ? key : NINF;
        int bp = cand ? lane : 127;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const float ov = __shfl_xor(bv, m, 64);
          const int op = __shfl_xor(bp, m, 64);
          if (ov > bv || (ov == bv && op < bp)) {
            bv = ov;
            bp = op;
          }
        }
        if (bp >= 64) break;  // no valid entry is left (wave-uniform)
        if (lane == bp) chosen = true;
        const int32_t pidx = __shfl(idx, bp, 64);
        const float prel = __shfl(rel, bp, 64);
        if (lane == t) {
          o_idx = pidx;
          o_pos = bp;
          o_rel = prel;
        }
        ms = fmaxf(ms, S[lane * SLD + bp]);
      }
      if (lane < K) {
        out_idx[u * K + lane] = o_idx;
        out_rel[u * K + lane] = o_rel;
        if (out_pos) out_pos[u * K + lane] = o_pos;
      }
      if (out_ild) {
        // mean of 1 - sim over the pairs of a set of positions: each member sums its pairs with
        // the later members in ascending position, then a fixed tree over the lanes
        auto ild = [&](uint64_t mask) __attribute__((always_inline)) {
          const int n = __builtin_popcountll(mask);
          float part = 0.f;
          if ((mask >> lane) & 1) {
            uint64_t later = mask & ~((2ull << lane) - 1);
            while (later) {
              const int j = __builtin_ctzll(later);
              later &= later - 1;
              part += 1.f - S[lane * SLD + j];
            }
          }
          const float tot = wave_sum(part);
          return n >= 2 ? tot / (float)(n * (n - 1) / 2) : 0.f;
        };
        const uint64_t vm = __ballot(valid);
        const bool head = valid && __builtin_popcountll(vm & ((1ull << lane) - 1)) < K;
        const float before = ild(__ballot(head));
        const float after = ild(__ballot(chosen));
        if (lane == 0) {
          out_ild[2 * u] = before;
          out_ild[2 * u + 1] = after;
        }
      }
    }
    par ^= 1;
  }
}

static int workgroups(int64_t U) {
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
    ncu = 256;
  return (int)(U < (int64_t)ncu * kWorkgroupsPerCU ? U : (int64_t)ncu * kWorkgroupsPerCU);
}

}  // namespace rr
}  // namespace nr

extern "C" int nr_rerank_mmr(int dtype, int64_t dim, int64_t U, int64_t N, const void* cand_table, int64_t cand_ld,
                             const float* cand_inv_norm, const int32_t* list_idx, const float* list_rel, int64_t M,
                             int64_t K, float lambda, int32_t* out_idx, float* out_rel, int32_t* out_pos,
                             float* out_ild, float* sim_out, void* stream) {
  using namespace nr::rr;
  constexpr const char* fn = "nr_rerank_mmr";
  nr::clear_error();
  if (dim != D) {
    nr::set_error("%s: dim %lld unsupported (1024 only)", fn, (long long)dim);
    return NR_ERR_UNSUPPORTED;
  }
  NR_CHECK_ARG(nr::ok_dtype(dtype), "%s: bad dtype %d", fn, dtype);
  NR_CHECK_ARG(M >= 1 && M <= MMAX, "%s: M = %lld outside [1, %d]", fn, (long long)M, MMAX);
  NR_CHECK_ARG(K >= 1 && K <= M, "%s: K = %lld outside [1, M = %lld]", fn, (long long)K, (long long)M);
  NR_CHECK_ARG(lambda >= 0.f && lambda <= 1.f, "%s: lambda = %g outside [0, 1]", fn, (double)lambda);  // NaN fails too
  NR_CHECK_ARG(U >= 1 && U < (1ll << 31), "%s: U = %lld outside [1, 2^31)", fn, (long long)U);
  NR_CHECK_ARG(N >= 1 && N < (1ll << 31), "%s: N = %lld outside [1, 2^31)", fn, (long long)N);
  NR_CHECK_ARG(cand_ld >= dim, "%s: cand_ld = %lld < dim", fn, (long long)cand_ld);
  NR_CHECK_ARG(cand_ld % (dtype == NR_F32 ? 4 : 8) == 0 && ((uintptr_t)cand_table & 15) == 0,
               "%s: cand_table must be 16-byte aligned with a 16-byte row stride", fn);
  NR_CHECK_ARG(cand_table && cand_inv_norm && list_idx && list_rel && out_idx && out_rel, "%s: null pointer", fn);
  NR_CHECK_DEVICE(fn, cand_table, cand_inv_norm, list_idx, list_rel, out_idx, out_rel, out_pos, out_ild, sim_out);

  hipStream_t st = (hipStream_t)stream;
  const float oml = 1.f - lambda;
  const dim3 grid((unsigned)workgroups(U));
  return nr::with_dtype(dtype, [&](auto tag) {
    using TI = typename decltype(tag)::type;
    hipLaunchKernelGGL(rerank_mmr_kernel<TI>, grid, dim3(256), 0, st, U, N, (const TI*)cand_table, cand_ld,
                       cand_inv_norm, list_idx, list_rel, (int)M, (int)K, lambda, oml, out_idx, out_rel, out_pos, out_ild,
                       sim_out);
    NR_CHECK_LAUNCH(fn);
    return (int)NR_OK;
  });
}
