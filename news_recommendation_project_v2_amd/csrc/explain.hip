// Exact per-click attribution of scores (include/newsrec_explain.h): per user the H x K
// contributions a[h][j] of its H history clicks to its K <= 64 listed news, their column
// sums (the scores) and the T <= 8 largest per column.
//
//   grid     a fixed number of workgroups (2 per CU) walking users with a stride, 256 threads.
//   scale    one pass over the user's history rows, thread t owning columns 4t .. 4t+3 and
//            adding the rows in ascending position (8 or 16 rows in flight): FINAL keeps
//            1 / (den_d + 1e-10) as 1024 f32 in LDS; every pooler gets |u| (LATENT |m| first)
//            from a fixed-order workgroup sum.  LATENT's and MEAN's per-user factor is applied
//            in the epilogue.
//   product  tiles of 64 history rows x the (up to 64) listed rows.  Both operands are
//            gathered in 64-element column slices through a two-stage LDS ring as f32
//            (bf16 rows are upcast on the way in; FINAL's share x p / (den + 1e-10) is formed
//            there, 272-byte row stride: conflict-free b128 fragment reads), the global loads
//            requested 4 slices at a time (f32 and FINAL: half as many each) once the previous
//            group is staged, a user's first group over its scale pass; one barrier per slice.
//            A pad's row is zeros in LDS and is never read from the table.  Wave w accumulates
//            history rows 16 w .. 16 w + 15 of the tile against each block of 16 listed rows on
//            v_mfma_f32_16x16x4_f32 (the f32 MFMA rate is the scarce one here: K = 10 costs one
//            block, and the four SIMDs share a tile's rows): per output one fmaf chain over the
//            1024 columns in a fixed order, whatever its place in the tile.
//   epilogue the scaled tile goes to a 64 x 65 f32 matrix in LDS (over ring stage 0, free
//            by then), from where it is stored to contrib_out, and wave 0, lane j owning
//            list entry j, adds it to the column sum and merges it into a sorted top-8 (value
//            descending, position ascending) in ascending position.  The first T are written.
//
// 68 KiB ring + 4 KiB + 0.3 KiB = 72.3 KiB of LDS: two workgroups per CU.
#include "nr_common.h"

#include "../../include/newsrec_explain.h"

namespace nr {
namespace ex {

constexpr int64_t D = 1024;
constexpr int KMAX = NR_TOPK_MAX;            // list entries (columns) per user
constexpr int HT = 64;                       // history rows per tile
constexpr int TOPN = NR_EXPLAIN_TOP_MAX;
constexpr int SL = 64;                       // elements per column slice
constexpr int NKT = (int)(D / SL);           // slices per row (even: a tile starts on ring stage 0)
constexpr int ROWW = 68;                     // LDS words per staged row slice (272 B)
constexpr int STAGE_WORDS = (HT + KMAX) * ROWW;
constexpr int CLD = 65;                      // contribution tile row stride, floats
constexpr int kWorkgroupsPerCU = 2;          // (also the waves per SIMD the register budget is held to)
static_assert(NKT % 2 == 0 && HT * CLD <= STAGE_WORDS, "the contribution tile lies over ring stage 0");
static_assert((2 * STAGE_WORDS + D + KMAX + 8) * 4 * kWorkgroupsPerCU <= 160 * 1024, "two workgroups per CU");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// four consecutive stored elements as f32
__device__ __forceinline__ f32x4 up4(u32x4 r) {
  return (f32x4){__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)};
}
__device__ __forceinline__ f32x4 up4(u32x2 r) { return (f32x4){bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y)}; }

template <typename TI, int POOL>
__global__ __launch_bounds__(256, kWorkgroupsPerCU) void explain_kernel(int64_t U, int64_t N, const TI* __restrict__ htab, int64_t hld,
                                                      const TI* __restrict__ ctab, int64_t cld,
                                                      const float* __restrict__ cinv, const int32_t* __restrict__ hidx,
                                                      const int64_t* __restrict__ hoff,
                                                      const int32_t* __restrict__ list_idx, int K, int T,
                                                      int32_t* __restrict__ top_pos, float* __restrict__ top_val,
                                                      float* __restrict__ sum_out, float* __restrict__ contrib_out) {
  // No contraction: every product and sum below is rounded as written (fmaf where one is meant).
#pragma clang fp contract(off)
  constexpr bool FINAL = POOL == NR_POOL_FINAL;
  using RAW = std::conditional_t<sizeof(TI) == 4, u32x4, u32x2>;  // 4 stored elements: the staging unit
  constexpr int PHALF = (int)(D / 4);                              // units from x to p of a FINAL row
  // Loads in flight per thread: PF slices of the product pass (x 8 units, 12 for FINAL), RS rows
  // of the scale pass (32 registers of them): as many as leave the kernel without spills at two
  // waves per SIMD.
  constexpr int PF = (sizeof(TI) == 4 ? 2 : 4) / (FINAL ? 2 : 1);
  constexpr int RS = (sizeof(TI) == 4 ? 8 : 16) / (FINAL ? 2 : 1);
  static_assert(NKT % PF == 0, "a slice keeps its register slot from tile to tile");
  __shared__ __attribute__((aligned(16))) float ring[2 * STAGE_WORDS];
  __shared__ __attribute__((aligned(16))) float rden_s[FINAL ? D : 4];
  __shared__ float cinv_s[KMAX];
  __shared__ float red_s[2][4];
  float* Cs = ring;  // [HT][CLD] over stage 0

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NINF = -__builtin_inff();
  const int fr = lane & 15, fg = lane >> 4;  // wave w: history rows 16 w .. 16 w + 15 of the tile, every column block

  // staging map: unit (row, c) = ((tid >> 4) + 16 p, tid & 15), p < 4, of the history rows and of the listed rows
  const int uc = tid & 15;
  int soff[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) soff[p] = ((tid >> 4) + 16 * p) * ROWW + uc * 4;

  auto block_sum = [&](float v, int slot) __attribute__((always_inline)) {
    v = wave_sum(v);
    if (lane == 0) red_s[slot][wave] = v;
    __syncthreads();
    return ((red_s[slot][0] + red_s[slot][1]) + red_s[slot][2]) + red_s[slot][3];
  };

  for (int64_t u = blockIdx.x; u < U; u += gridDim.x) {
    const int64_t h0 = hoff[u];
    const int H = (int)(hoff[u + 1] - h0);
    const int32_t* li = list_idx + u * K;
    if (H <= 0) {  // wave-uniform
      if (tid < K) {
        if (sum_out) sum_out[u * K + tid] = 0.f;
        if (top_pos)
          for (int t = 0; t < T; ++t) {
            top_pos[(u * K + tid) * T + t] = -1;
            top_val[(u * K + tid) * T + t] = NINF;
          }
      }
      continue;
    }

    // ---- the list: wave 0, lane j owns entry j
    const RAW* gc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = (tid >> 4) + 16 * p;
      const int32_t ix = row < K ? li[row] : -1;
      gc[p] = ix >= 0 && ix < N ? reinterpret_cast<const RAW*>(ctab + (int64_t)ix * cld) + uc : nullptr;
    }
    bool my_valid = false;
    if (wave == 0) {
      const int32_t ix = lane < K ? li[lane] : -1;
      my_valid = ix >= 0 && ix < N;
      cinv_s[lane] = my_valid ? cinv[ix] : 0.f;
    }

    // ---- the product pass's staging; its first slices are requested here, over the scale pass
    const RAW* gh[4];
    RAW rh[PF][4], rph[FINAL ? PF : 1][4], rc[PF][4];
    auto set_hist = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int i = tile * HT + (tid >> 4) + 16 * p;
        gh[p] = i < H ? reinterpret_cast<const RAW*>(htab + (int64_t)hidx[h0 + i] * hld) + uc : nullptr;
      }
    };
    auto gload = [&](int slot, int kt) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        rh[slot][p] = gh[p] ? gh[p][kt * 16] : (RAW)0u;
        if constexpr (FINAL) rph[slot][p] = gh[p] ? gh[p][kt * 16 + PHALF] : (RAW)0u;
        rc[slot][p] = gc[p] ? gc[p][kt * 16] : (RAW)0u;
      }
    };
    auto lstore = [&](int buf, int slot, int kt) __attribute__((always_inline)) {
      float* st = ring + buf * STAGE_WORDS;
      f32x4 rd = (f32x4)0.f;
      if constexpr (FINAL) rd = *reinterpret_cast<const f32x4*>(rden_s + kt * SL + 4 * uc);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f32x4 a = up4(rh[slot][p]);
        if constexpr (FINAL) a = (a * up4(rph[slot][p])) * rd;
        *reinterpret_cast<f32x4*>(st + soff[p]) = a;
        *reinterpret_cast<f32x4*>(st + HT * ROWW + soff[p]) = up4(rc[slot][p]);
      }
    };

    set_hist(0);
#pragma unroll
    for (int sl = 0; sl < PF; ++sl) gload(sl, sl);

    // ---- scale pass: column sums in ascending position, thread t owning columns 4t .. 4t+3
    float s[4] = {0.f, 0.f, 0.f, 0.f}, dn[4] = {0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < H; h += RS) {
      RAW rx[RS], rp[FINAL ? RS : 1];
#pragma unroll
      for (int q = 0; q < RS; ++q) {
        rx[q] = (RAW)0u;
        if constexpr (FINAL) rp[q] = (RAW)0u;
        if (h + q < H) {
          const RAW* p = reinterpret_cast<const RAW*>(htab + (int64_t)hidx[h0 + h + q] * hld) + tid;
          rx[q] = p[0];
          if constexpr (FINAL) rp[q] = p[PHALF];
        }
      }
#pragma unroll
      for (int q = 0; q < RS; ++q) {
        const f32x4 x = up4(rx[q]);
        if constexpr (FINAL) {
          const f32x4 pw = up4(rp[q]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            s[c] = fmaf(x[c], pw[c], s[c]);
            dn[c] += pw[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) s[c] += x[c];
        }
      }
    }
    const float Hf = (float)H;
    float s_g = 1.f, ss = 0.f;  // g_h = s_g * (staged row)
    if constexpr (FINAL) {
      f32x4 rd;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        rd[c] = 1.f / (dn[c] + 1e-10f);
        const float uu = s[c] * rd[c];
        ss = fmaf(uu, uu, ss);
      }
      *reinterpret_cast<f32x4*>(rden_s + 4 * tid) = rd;
    } else if constexpr (POOL == NR_POOL_MEAN) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float uu = s[c] / Hf;
        ss = fmaf(uu, uu, ss);
      }
      s_g = 1.f / Hf;
    } else {
      float ssm = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s[c] = s[c] / Hf;
        ssm = fmaf(s[c], s[c], ssm);
      }
      const float den1 = fmaxf(sqrtf(block_sum(ssm, 1)), 1e-12f);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float uu = s[c] / den1;
        ss = fmaf(uu, uu, ss);
      }
      s_g = 1.f / (Hf * den1);
    }
    const float inv_u = 1.f / fmaxf(sqrtf(block_sum(ss, 0)), 1e-8f);  // (its barrier also publishes rden_s, cinv_s)

    // ---- product pass
    float sum = 0.f, tv[TOPN];
    int32_t tp[TOPN];
#pragma unroll
    for (int t = 0; t < TOPN; ++t) {
      tv[t] = NINF;
      tp[t] = -1;
    }

    const int ntiles = (H + HT - 1) / HT;
    for (int tile = 0; tile < ntiles; ++tile) {
      const int cnt = min(HT, H - tile * HT);
      const bool has_rows = 16 * wave < cnt;
      const int ncb = (K + 15) >> 4;  // column blocks of 16 listed rows
      f32x4 acc[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[cb] = (f32x4)0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int cur = kt & 1, slot = kt % PF;
        lstore(cur, slot, kt);
        __syncthreads();  // (the stage written next was last read before the previous barrier)
        // Once a group of PF slices is staged its registers take the next PF slices, of this
        // tile or of the next one, all requested together: one exposed round trip per group.
        // (The loads sit under per-row conditions, so a staging step waits for every load in
        // flight; requesting slice by slice would expose one round trip per slice.)
        if (slot == PF - 1) {
          if (kt + 1 < NKT) {
#pragma unroll
            for (int sl = 0; sl < PF; ++sl) gload(sl, kt + 1 + sl);
          } else if (tile + 1 < ntiles) {
            set_hist(tile + 1);
#pragma unroll
            for (int sl = 0; sl < PF; ++sl) gload(sl, sl);
          }
        }
        if (has_rows) {
          // lane (r, g) covers k = 16 g + 4 q + t of the 64-deep slice (both operands alike)
          const float* ra = ring + cur * STAGE_WORDS + (16 * wave + fr) * ROWW + 16 * fg;
          const float* rb = ring + cur * STAGE_WORDS + (HT + fr) * ROWW + 16 * fg;
          f32x4 a[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) a[q] = *reinterpret_cast<const f32x4*>(ra + 4 * q);
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            if (cb < ncb) {  // wave-uniform
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(rb + cb * 16 * ROWW + 4 * q);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][t], b[t], acc[cb], 0, 0, 0);
              }
            }
          }
        }
      }
      // ---- the scaled tile.  C/D map of a 16 x 16 block: col (j) = lane & 15, row (i) = reg + 4 (lane >> 4).
      // The last slice sits in stage 1 and stage 0 was last read before that slice's barrier.
      if (has_rows) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          if (cb < ncb) {
            const int j = 16 * cb + fr;
            const float cj = cinv_s[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = 16 * wave + 4 * fg + r;
              Cs[i * CLD + j] = cj == 0.f ? 0.f : ((acc[cb][r] * s_g) * cj) * inv_u;  // a pad's inverse norm is 0
            }
          }
        }
      }
      __syncthreads();
      if (contrib_out) {
        float* co = contrib_out + (h0 + (int64_t)tile * HT) * K;
        for (int e = tid; e < cnt * K; e += 256) {
          const int i = e / K;
          co[e] = Cs[i * CLD + (e - i * K)];
        }
      }
      if (my_valid) {  // wave 0, lane j < K
        for (int i = 0; i < cnt; ++i) {
          const float v = Cs[i * CLD + lane];
          const int32_t pos = tile * HT + i;
          sum += v;
          if (v > tv[TOPN - 1]) {
            // positions come in ascending order, so an equal value stays behind the ones kept
#pragma unroll
            for (int t = TOPN - 1; t >= 1; --t) {
              const bool up = v > tv[t - 1], here = v > tv[t];
              tp[t] = up ? tp[t - 1] : here ? pos : tp[t];
              tv[t] = up ? tv[t - 1] : here ? v : tv[t];
            }
            if (v > tv[0]) {
              tv[0] = v;
              tp[0] = pos;
            }
          }
        }
      }
      __syncthreads();  // the next tile's first slice is written over the contribution tile
    }
    if (wave == 0 && lane < K) {
      if (sum_out) sum_out[u * K + lane] = sum;  // a pad's is still 0
      if (top_pos) {
#pragma unroll
        for (int t = 0; t < TOPN; ++t)
          if (t < T) {
            top_pos[(u * K + lane) * T + t] = tp[t];
            top_val[(u * K + lane) * T + t] = tv[t];
          }
      }
    }
  }
}

static int workgroups(int64_t U) {
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
    ncu = 256;
  return (int)(U < (int64_t)ncu * kWorkgroupsPerCU ? U : (int64_t)ncu * kWorkgroupsPerCU);
}

}  // namespace ex
}  // namespace nr

extern "C" int nr_explain_scores(int pooler, int dtype, int64_t dim, const void* hist_table, int64_t hist_ld, int64_t N,
                                 const void* cand_table, int64_t cand_ld, const float* cand_inv_norm, int64_t U,
                                 const int32_t* hist_idx, const int64_t* hist_off, const int32_t* list_idx, int64_t K,
                                 int64_t T, int32_t* top_pos, float* top_val, float* sum_out, float* contrib_out,
                                 void* stream) {
  using namespace nr::ex;
  constexpr const char* fn = "nr_explain_scores";
  nr::clear_error();
  if (dim != D) {
    nr::set_error("%s: dim %lld unsupported (1024 only)", fn, (long long)dim);
    return NR_ERR_UNSUPPORTED;
  }
  NR_CHECK_ARG(pooler == NR_POOL_FINAL || pooler == NR_POOL_LATENT || pooler == NR_POOL_MEAN, "%s: bad pooler %d", fn,
               pooler);
  NR_CHECK_ARG(nr::ok_dtype(dtype), "%s: bad dtype %d", fn, dtype);
  NR_CHECK_ARG(K >= 1 && K <= KMAX, "%s: K = %lld outside [1, %d]", fn, (long long)K, KMAX);
  NR_CHECK_ARG((top_pos == nullptr) == (top_val == nullptr), "%s: top_pos and top_val go together", fn);
  NR_CHECK_ARG(!top_pos || (T >= 1 && T <= TOPN), "%s: T = %lld outside [1, %d]", fn, (long long)T, TOPN);
  NR_CHECK_ARG(top_pos || sum_out || contrib_out, "%s: no output requested", fn);
  NR_CHECK_ARG(U >= 1 && U < (1ll << 31), "%s: U = %lld outside [1, 2^31)", fn, (long long)U);
  NR_CHECK_ARG(N >= 1 && N < (1ll << 31), "%s: N = %lld outside [1, 2^31)", fn, (long long)N);
  NR_CHECK_ARG(hist_ld >= (pooler == NR_POOL_FINAL ? 2 * dim : dim) && cand_ld >= dim,
               "%s: leading dimension too small", fn);
  const int64_t align = dtype == NR_F32 ? 4 : 8;
  NR_CHECK_ARG(hist_ld % align == 0 && cand_ld % align == 0 && ((uintptr_t)hist_table & 15) == 0 &&
                   ((uintptr_t)cand_table & 15) == 0,
               "%s: tables must be 16-byte aligned with 16-byte row strides", fn);
  NR_CHECK_ARG(hist_table && cand_table && cand_inv_norm && hist_idx && hist_off && list_idx, "%s: null pointer", fn);
  NR_CHECK_DEVICE(fn, hist_table, cand_table, cand_inv_norm, hist_idx, hist_off, list_idx, top_pos, top_val, sum_out,
                  contrib_out);

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)workgroups(U));
  return nr::with_dtype(dtype, [&](auto tag) -> int {
    using TI = typename decltype(tag)::type;
    const auto miss = [&] { return nr::unvalidated_code("pooler", pooler); };
    return nr::with_int<NR_POOL_MEAN, NR_POOL_FINAL, NR_POOL_LATENT>(pooler, miss, [&](auto pool) -> int {
      hipLaunchKernelGGL((explain_kernel<TI, decltype(pool)::value>), grid, dim3(256), 0, st, U, N,
                         (const TI*)hist_table, hist_ld, (const TI*)cand_table, cand_ld, cand_inv_norm, hist_idx,
                         hist_off, list_idx, (int)K, (int)T, top_pos, top_val, sum_out, contrib_out);
      NR_CHECK_LAUNCH(fn);
      return (int)NR_OK;
    });
  });
}
