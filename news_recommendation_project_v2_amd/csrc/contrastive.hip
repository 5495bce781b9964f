// InfoNCE loss with in-batch negatives (include/newsrec_contrastive.h): the loss
// stage of the contrastive config-5 steps and the stand-alone nr_cosine_infonce.
// The reference carries it as the commented loss of trainer.py:612-625 over the data
// of data_utils.py:275-334 / 512-578 / 794-817.  f32 throughout, in both step dtypes.
//
//   prep      one wave per row: unit vectors Uh [Bp][D], Eh [Cp][D] (zero rows for pads
//             and up to Bp = pad16(B), Cp = pad16(Cn)), inverse norms, clamp indicators;
//             from token states also the candidates' xhat rows (cn_prep_kernel)
//   S         = Uh Eh^T                 [B][Cn], K = 1024      (cn_gemm_kernel)
//   softmax   one wave per row: mask, max, sum exp, loss term; S <- G = (softmax -
//             onehot) inv_tau / B, zero where excluded and in the pad rows / columns
//   dUh       = G Eh                    [B][D],  K = Cp        (cn_gemm_kernel)
//   dEh       = G^T Uh                  [Cn][D], K = Bp        (cn_gemm_kernel)
//   norm bwd  one wave per row, in place: du = iu (dUh - cu (dUh . Uh) Uh), same for E
//   LN / loss the candidates' token LN parameter-grad partials (pair_ln_kernel's layout
//             over Cn rows) and the ordered sum of the loss terms (cn_ln_loss_kernel)
//
// The three products run on ONE small dedicated kernel rather than on gemm.hip's f32
// tile kernels: those take A [M][K] and W [N][K] with K contiguous and M, N, K in
// whole tiles, so dUh and dEh would each need a transposed copy of G and of Eh / Uh
// plus zero padding of B and Cn to 128 (at B = 5 a 25x larger product).  Here an
// operand is read either way round (K contiguous, or the output index contiguous),
// B and Cn are padded to 16 only, and the stage has no transposes.  64x64 output
// tile per workgroup, one 32x32 accumulator of v_mfma_f32_32x32x2_f32 (the exact-f32
// MFMA of gemm_kernel's f32 path) per wave, K in chunks of 16 through a two-stage LDS
// ring with the next chunk's global loads in flight over the MFMAs.  No split-K, no
// atomics: every output element is one fixed-order chain.
#include "nr_train.h"

#include "../../include/newsrec_contrastive.h"

#include <new>
#include <vector>

namespace nr {
namespace cn {

constexpr int64_t D = 1024;
static inline int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }

// ------------------------------------------------------------------ row preparation
// Rows r < Bp: users (zero rows past B); rows Bp + c, c < Cp: candidates (zero rows
// for pads and past Cn).  TT = void-like tag float with tok == nullptr: E table rows.
template <typename TT>
__global__ __launch_bounds__(256) void cn_prep_kernel(int64_t B, int64_t Bp, int64_t Cn, int64_t Cp,
                                                      const float* __restrict__ users, const float* __restrict__ E,
                                                      int64_t lde, const TT* __restrict__ tok,
                                                      const float* __restrict__ tg, const float* __restrict__ tb,
                                                      const int32_t* __restrict__ cand, float* __restrict__ Uh,
                                                      float* __restrict__ Eh, float* __restrict__ xh,
                                                      float* __restrict__ nrm /* [Bp + Cp][2]: inv, live */) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= Bp + Cp) return;
  const bool is_user = r < Bp;
  const int64_t c = r - Bp;
  int64_t src = -1;  // wave-uniform
  if (is_user) src = r < B ? r : -1;
  else if (c < Cn) src = cand[c];
  float v[4][4] = {};
  if (src >= 0) {
    if (is_user) {
#pragma unroll
      for (int j = 0; j < 4; ++j) ld4<float>(users + src * D + j * 256 + lane * 4, v[j]);
    } else if (tok) {
      tok_xhat<TT>(tok + src * D, lane, v);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) ld4<float>(E + src * lde + j * 256 + lane * 4, v[j]);
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = j * 256 + lane * 4;
    if (!is_user && tok) {
      // E = xhat gamma + beta, as slots_kernel / cos_pairs_kernel form it; xhat kept for the LN grads
      if (c < Cn) st4<float>(xh + c * D + e, v[j]);
      float gg[4], bb[4];
      ld4<float>(tg + e, gg);
      ld4<float>(tb + e, bb);
#pragma unroll
      for (int t = 0; t < 4; ++t) v[j][t] = src >= 0 ? fmaf(v[j][t], gg[t], bb[t]) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) ss = fmaf(v[j][t], v[j][t], ss);
  }
  ss = wave_sum(ss);
  CosUnit cu(ss);
  if (src < 0) { cu.inv = 0.f; cu.live = 0.f; }
  float* dst = is_user ? Uh + r * D : Eh + c * D;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = v[j][t] * cu.inv;
    st4<float>(dst + j * 256 + lane * 4, o);
  }
  if (lane == 0) { nrm[2 * r] = cu.inv; nrm[2 * r + 1] = cu.live; }
}

// ------------------------------------------------------------------ the products
// C[m][n] = sum_k A(m, k) B(n, k), m < M, n < N, K a multiple of 16.  An operand X is
// stored either [rows][K] (XK: K contiguous, X(i, k) = X[i ldx + k]) or [K][rows]
// (X(i, k) = X[k ldx + i]); rows at or past its limit (arows / brows, a multiple of 4
// in the second form) read as zero, so M and N need no padding.  ldx % 4 == 0.
constexpr int CT = 64, CK = 16;
template <bool XK>
struct CnOperand {
  static constexpr int LD = XK ? CT + 33 : CT + 32;  // LDS [k][row]; XK: scalar stores, else 16-B ones
  int64_t off;  // this thread's element offset at k0 = 0
  bool ok;
  int r, k;     // its 4 elements: XK: (row r, k .. k + 3), else (rows r .. r + 3, k)
  __device__ __forceinline__ CnOperand(int64_t row0, int64_t rows, int64_t ldx) {
    const int t = threadIdx.x;
    if constexpr (XK) { r = t >> 2; k = (t & 3) * 4; off = (row0 + r) * ldx + k; }
    else { k = t >> 4; r = (t & 15) * 4; off = (int64_t)k * ldx + row0 + r; }
    ok = row0 + r < rows;
  }
  __device__ __forceinline__ float4 load(const float* __restrict__ X, int64_t k0, int64_t ldx) const {
    if (!ok) return float4{0.f, 0.f, 0.f, 0.f};
    return *reinterpret_cast<const float4*>(X + off + (XK ? k0 : k0 * ldx));
  }
  __device__ __forceinline__ void store(float* tile, float4 v) const {
    if constexpr (XK) {
      tile[(k + 0) * LD + r] = v.x; tile[(k + 1) * LD + r] = v.y;
      tile[(k + 2) * LD + r] = v.z; tile[(k + 3) * LD + r] = v.w;
    } else {
      *reinterpret_cast<float4*>(tile + k * LD + r) = v;
    }
  }
};

template <bool AK, bool BK>
__global__ __launch_bounds__(256) void cn_gemm_kernel(int64_t M, int64_t N, int64_t K, const float* __restrict__ A,
                                                      int64_t lda, int64_t arows, const float* __restrict__ Bm,
                                                      int64_t ldb, int64_t brows, float* __restrict__ C,
                                                      int64_t ldc) {
  using OA = CnOperand<AK>;
  using OB = CnOperand<BK>;
  __shared__ __attribute__((aligned(16))) float sa[2][CK * OA::LD];
  __shared__ __attribute__((aligned(16))) float sb[2][CK * OB::LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // (M tiles on grid.x: M reaches 2^24 rows, N <= 2^20 columns stays within grid.y's 65,535)
  const int64_t m0 = (int64_t)blockIdx.x * CT, n0 = (int64_t)blockIdx.y * CT;
  const OA oa(m0, arows, lda);
  const OB ob(n0, brows, ldb);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;  // operand map: lane (r, h) holds k = h of row r
  const int64_t nk = K / CK;
  float4 ra = oa.load(A, 0, lda), rb = ob.load(Bm, 0, ldb);
  oa.store(sa[0], ra);
  ob.store(sb[0], rb);
  __syncthreads();
  for (int64_t kt = 0; kt < nk; ++kt) {
    const int cur = (int)(kt & 1);
    if (kt + 1 < nk) {
      ra = oa.load(A, (kt + 1) * CK, lda);
      rb = ob.load(Bm, (kt + 1) * CK, ldb);
    }
    const float* ta = sa[cur] + wm * 32 + fr;
    const float* tb = sb[cur] + wn * 32 + fr;
#pragma unroll
    for (int kk = 0; kk < CK / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[(2 * kk + fh) * OA::LD], tb[(2 * kk + fh) * OB::LD], acc, 0, 0, 0);
    if (kt + 1 < nk) {
      oa.store(sa[cur ^ 1], ra);
      ob.store(sb[cur ^ 1], rb);
    }
    __syncthreads();
  }
  // C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int64_t col = n0 + wn * 32 + fr;
  if (col < N) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t row = m0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * fh;
      if (row < M) C[row * ldc + col] = acc[reg];
    }
  }
}

// ------------------------------------------------------------------ row softmax + CE
// One wave per row b < Bp of S [Bp][Cp]: rows past B and columns past Cn become zero.
__global__ __launch_bounds__(256) void cn_softmax_kernel(int64_t B, int64_t Bp, int64_t Cn, int64_t Cp,
                                                         float* __restrict__ S, const int32_t* __restrict__ cand,
                                                         const int32_t* __restrict__ target,
                                                         const uint8_t* __restrict__ mask, float inv_tau,
                                                         float* __restrict__ logits_out, float* __restrict__ lrow) {
  // No contraction in this kernel: a logit is the ROUNDED product s inv_tau wherever it is
  // used (fused into z - m it would be the exact product there and the rounded one in the
  // maximum), so a row whose only column is its target has z - m = 0 and its loss term and
  // gradient are exactly 0.
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= Bp) return;
  float* s = S + b * Cp;
  if (b >= B) {
    for (int64_t c = lane; c < Cp; c += 64) s[c] = 0.f;
    return;
  }
  const float NINF = -__builtin_inff();
  const uint8_t* mk = mask ? mask + b * Cn : nullptr;
  const int64_t tcol = target[b];
  const float zt = s[tcol] * inv_tau;  // read before the row is rewritten below
  auto logit = [&](int64_t c) { return (cand[c] < 0 || (mk && mk[c])) ? NINF : s[c] * inv_tau; };
  float m = NINF;
  for (int64_t c = lane; c < Cn; c += 64) m = fmaxf(m, logit(c));
  m = wave_max(m);  // finite: the host checked that the target column is included
  float sum = 0.f;
  for (int64_t c = lane; c < Cn; c += 64) {
    const float z = logit(c);
    if (z != NINF) sum += expf(z - m);
  }
  sum = wave_sum(sum);
  const SoftmaxCE ce(m, sum, B);
  if (lane == 0) lrow[b] = ce.loss_term(zt);
  for (int64_t c = lane; c < Cp; c += 64) {
    float g = 0.f;
    if (c < Cn) {
      const float z = logit(c);
      if (logits_out) logits_out[b * Cn + c] = z;
      if (z != NINF) g = ce.dz(z, c == tcol) * inv_tau;
    }
    s[c] = g;
  }
}

// ------------------------------------------------------------------ normalisation backward
// In place over du [B][D] (rows r < B) and dE [Cn][D] (rows B + c): d = inv (dh - live (dh . h) h).
__global__ __launch_bounds__(256) void cn_norm_bwd_kernel(int64_t B, int64_t Bp, int64_t Cn,
                                                          const float* __restrict__ Uh, const float* __restrict__ Eh,
                                                          const float* __restrict__ nrm, float* __restrict__ du,
                                                          float* __restrict__ dE) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B + Cn) return;
  const bool is_user = r < B;
  const int64_t c = r - B;
  const float* h = is_user ? Uh + r * D : Eh + c * D;
  float* d = is_user ? du + r * D : dE + c * D;
  const int64_t ni = is_user ? r : Bp + c;
  const CosUnit cu(nrm[2 * ni], nrm[2 * ni + 1]);
  float hv[4][4], dv[4][4], dot = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ld4<float>(h + j * 256 + lane * 4, hv[j]);
    ld4<float>(d + j * 256 + lane * 4, dv[j]);
#pragma unroll
    for (int t = 0; t < 4; ++t) dot = fmaf(dv[j][t], hv[j][t], dot);
  }
  dot = wave_sum(dot);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = cu.bwd(dv[j][t], hv[j][t], dot);
    st4<float>(d + j * 256 + lane * 4, o);
  }
}

// ------------------------------------------------------------------ token LN grads + loss
// pair_ln_kernel (final_train.hip) over the Cn candidate rows: chunk k (rows k, k +
// kCnLnChunks, ...) -> part[k][0][c] = sum g xhat, part[k][1][c] = sum g.  Block = 64
// columns x 4 row groups; grid (D / 64, kCnLnChunks), or (1, 1) with part == nullptr
// for the loss alone.  Block (0, 0)'s first wave writes the loss as the ordered (fixed
// tree) sum of the per-row terms.
__global__ __launch_bounds__(256) void cn_ln_loss_kernel(int64_t B, int64_t Cn, const float* __restrict__ dE,
                                                         const float* __restrict__ xh, const float* __restrict__ lrow,
                                                         float* __restrict__ part, float* __restrict__ loss) {
  __shared__ float red[2][4][64];
  const int grp = threadIdx.x >> 6, cl = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  if (part) {
    const int64_t step = (int64_t)kCnLnChunks * 4;
    float sg = 0.f, sb = 0.f;
#pragma unroll 4
    for (int64_t r = (int64_t)blockIdx.y + kCnLnChunks * grp; r < Cn; r += step) {
      const float gv = dE[r * D + c];
      sg = fmaf(gv, xh[r * D + c], sg);
      sb += gv;
    }
    red[0][grp][cl] = sg;
    red[1][grp][cl] = sb;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    if (part) {
      part[(int64_t)blockIdx.y * 2 * D + c] = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
      part[(int64_t)blockIdx.y * 2 * D + D + c] = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {
      float l = 0.f;
      for (int64_t r = threadIdx.x; r < B; r += 64) l += lrow[r];
      l = wave_sum(l);
      if (threadIdx.x == 0) *loss = l;
    }
  }
}

// ------------------------------------------------------------------ host
struct Layout {
  int64_t Bp, Cp, Uh, Eh, S, nrm, lrow, xh, dE, total;
};
static Layout layout(int64_t B, int64_t Cn, bool from_tokens, bool own_dE) {
  Layout L{};
  L.Bp = pad16(B);
  L.Cp = pad16(Cn);
  WsCursor w;
  L.Uh = w.take(L.Bp * D * 4);
  L.Eh = w.take(L.Cp * D * 4);
  L.S = w.take(L.Bp * L.Cp * 4);
  L.nrm = w.take((L.Bp + L.Cp) * 2 * 4);
  L.lrow = w.take(L.Bp * 4);
  L.xh = w.take(from_tokens ? Cn * D * 4 : 0);
  L.dE = w.take(own_dE ? Cn * D * 4 : 0);
  L.total = w.o;
  return L;
}

template <bool AK, bool BK>
static int gemm(const char* fn, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, int64_t arows,
                const float* Bm, int64_t ldb, int64_t brows, float* C, int64_t ldc, hipStream_t st) {
  const dim3 grid((unsigned)((M + CT - 1) / CT), (unsigned)((N + CT - 1) / CT));
  hipLaunchKernelGGL((cn_gemm_kernel<AK, BK>), grid, dim3(256), 0, st, M, N, K, A, lda, arows, Bm, ldb, brows, C, ldc);
  NR_CHECK_LAUNCH(fn);
  return NR_OK;
}

}  // namespace cn

int64_t contrastive_ws_bytes(int64_t B, int64_t Cn, bool from_tokens, bool own_dE) {
  return cn::layout(B, Cn, from_tokens, own_dE).total;
}

int contrastive_check(const char* fn, const CnSpec& sp, hipStream_t st) {
  NR_CHECK_ARG(sp.B >= 1 && sp.B <= (1ll << 24), "%s: B = %lld outside [1, 2^24]", fn, (long long)sp.B);
  // (the three products' grids, and B Cn mask bytes read back per call)
  NR_CHECK_ARG(sp.Cn >= 1 && sp.Cn <= (1ll << 20), "%s: Cn = %lld outside [1, 2^20]", fn, (long long)sp.Cn);
  NR_CHECK_ARG(sp.B * sp.Cn <= (1ll << 31), "%s: B x Cn = %lld x %lld logits exceed 2^31", fn, (long long)sp.B,
               (long long)sp.Cn);
  NR_CHECK_ARG(sp.cand && sp.target, "%s: null cand / target", fn);
  NR_CHECK_ARG(sp.inv_tau > 0.f && sp.inv_tau < __builtin_inff(), "%s: inv_tau must be positive and finite", fn);
  NR_CHECK_DEVICE(fn, sp.cand, sp.target, sp.mask);
  std::vector<int32_t> cand, target;
  std::vector<uint8_t> mask;
  try {  // (no exception crosses the C ABI)
    cand.resize((size_t)sp.Cn);
    target.resize((size_t)sp.B);
    mask.resize(sp.mask ? (size_t)(sp.B * sp.Cn) : 0);
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory for the target check (%lld mask bytes)", fn, (long long)(sp.B * sp.Cn));
    return NR_ERR_INVALID;
  }
  // ordered after the uploads queued on st; the copies themselves block the host
  NR_TRY_HIP(hipStreamSynchronize(st), fn, "stream synchronize (target check)");
  NR_TRY_HIP(hipMemcpy(cand.data(), sp.cand, cand.size() * 4, hipMemcpyDeviceToHost), fn, "cand read-back");
  NR_TRY_HIP(hipMemcpy(target.data(), sp.target, target.size() * 4, hipMemcpyDeviceToHost), fn, "target read-back");
  if (sp.mask) NR_TRY_HIP(hipMemcpy(mask.data(), sp.mask, mask.size(), hipMemcpyDeviceToHost), fn, "mask read-back");
  if (sp.U > 0)
    for (int64_t c = 0; c < sp.Cn; ++c)
      NR_CHECK_ARG(cand[(size_t)c] < sp.U, "%s: cand[%lld] = %d outside the %lld news rows", fn, (long long)c,
                   cand[(size_t)c], (long long)sp.U);
  for (int64_t b = 0; b < sp.B; ++b) {
    const int64_t t = target[(size_t)b];
    NR_CHECK_ARG(t >= 0 && t < sp.Cn, "%s: target[%lld] = %lld out of range [0, %lld)", fn, (long long)b, (long long)t,
                 (long long)sp.Cn);
    NR_CHECK_ARG(cand[(size_t)t] >= 0, "%s: target[%lld] = %lld is a pad column", fn, (long long)b, (long long)t);
    NR_CHECK_ARG(!sp.mask || !mask[(size_t)(b * sp.Cn + t)], "%s: target[%lld] = %lld is masked for its own row", fn,
                 (long long)b, (long long)t);
  }
  return NR_OK;
}

int contrastive_stage(const char* fn, const CnSpec& sp, const float* users, const float* E, int64_t lde,
                      const void* tok, int tok_dtype, const float* tg, const float* tb, float* logits_out,
                      float* loss, float* du, float* dE_cols, float* ln_part, char* ws, hipStream_t st) {
  using namespace cn;
  const int64_t B = sp.B, Cn = sp.Cn;
  const Layout L = layout(B, Cn, tok != nullptr, dE_cols == nullptr);
  const int64_t Bp = L.Bp, Cp = L.Cp;
  float *Uh = (float*)(ws + L.Uh), *Eh = (float*)(ws + L.Eh), *S = (float*)(ws + L.S), *nrm = (float*)(ws + L.nrm);
  float *lrow = (float*)(ws + L.lrow), *xh = (float*)(ws + L.xh);
  float* dE = dE_cols ? dE_cols : (float*)(ws + L.dE);
  {
    const dim3 grid((unsigned)((Bp + Cp + 3) / 4));
    if (tok) {
      NR_TRY(with_tok_dtype(tok_dtype, [&](auto tt) -> int {
        using TT = typename decltype(tt)::type;
        hipLaunchKernelGGL((cn_prep_kernel<TT>), grid, dim3(256), 0, st, B, Bp, Cn, Cp, users, nullptr, (int64_t)0,
                           (const TT*)tok, tg, tb, sp.cand, Uh, Eh, xh, nrm);
        return NR_OK;
      }));
    } else {
      hipLaunchKernelGGL((cn_prep_kernel<float>), grid, dim3(256), 0, st, B, Bp, Cn, Cp, users, E, lde,
                         (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, sp.cand, Uh, Eh,
                         (float*)nullptr, nrm);
    }
    NR_CHECK_LAUNCH(fn);
  }
  // S = Uh Eh^T (both K-contiguous; rows past B / Cn are never stored)
  NR_TRY((gemm<true, true>(fn, B, Cn, D, Uh, D, Bp, Eh, D, Cp, S, Cp, st)));
  hipLaunchKernelGGL(cn_softmax_kernel, dim3((unsigned)((Bp + 3) / 4)), dim3(256), 0, st, B, Bp, Cn, Cp, S, sp.cand,
                     sp.target, sp.mask, sp.inv_tau, logits_out, lrow);
  NR_CHECK_LAUNCH(fn);
  // dUh = G Eh: A = G [B][Cp] (K = Cp contiguous), B(n = d, k = c) = Eh[c][d]
  NR_TRY((gemm<true, false>(fn, B, D, Cp, S, Cp, Bp, Eh, D, D, du, D, st)));
  // dEh = G^T Uh: A(m = c, k = b) = G[b][c], B(n = d, k = b) = Uh[b][d]
  NR_TRY((gemm<false, false>(fn, Cn, D, Bp, S, Cp, Cp, Uh, D, D, dE, D, st)));
  hipLaunchKernelGGL(cn_norm_bwd_kernel, dim3((unsigned)((B + Cn + 3) / 4)), dim3(256), 0, st, B, Bp, Cn, Uh, Eh, nrm,
                     du, dE);
  NR_CHECK_LAUNCH(fn);
  const dim3 lgrid = ln_part ? dim3((unsigned)(D / 64), kCnLnChunks) : dim3(1, 1);
  hipLaunchKernelGGL(cn_ln_loss_kernel, lgrid, dim3(256), 0, st, B, Cn, dE, xh, lrow, ln_part, loss);
  NR_CHECK_LAUNCH(fn);
  return NR_OK;
}

}  // namespace nr

extern "C" int64_t nr_cosine_infonce_workspace_bytes(int64_t B, int64_t Cn) {
  if (B < 1 || Cn < 1 || B > (1ll << 24) || Cn > (1ll << 20)) return -1;
  return nr::contrastive_ws_bytes(B, Cn, false, false);
}

extern "C" int nr_cosine_infonce(int64_t B, int64_t Cn, const float* users, const float* E, int64_t lde,
                                 const int32_t* cand, const int32_t* target, const uint8_t* mask, float inv_tau,
                                 float* logits_out, float* loss, float* du, float* dE_cols, void* ws, int64_t ws_bytes,
                                 void* stream) {
  constexpr const char* fn = "nr_cosine_infonce";
  nr::clear_error();
  NR_CHECK_ARG(lde >= 1024 && lde % 4 == 0, "%s: lde must be >= 1024 and a multiple of 4", fn);
  NR_CHECK_ARG(B >= 1 && Cn >= 1, "%s: B = %lld, Cn = %lld: both must be >= 1", fn, (long long)B, (long long)Cn);
  NR_CHECK_ARG(users && E && loss && du && dE_cols && ws, "%s: null pointer", fn);
  NR_CHECK_DEVICE(fn, users, E, logits_out, loss, du, dE_cols, ws);
  const nr::CnSpec sp{B, Cn, 0, cand, target, mask, inv_tau};
  hipStream_t st = (hipStream_t)stream;
  NR_TRY(nr::contrastive_check(fn, sp, st));
  const int64_t need = nr::contrastive_ws_bytes(B, Cn, false, false);
  NR_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes, (long long)need);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  return nr::contrastive_stage(fn, sp, users, E, lde, nullptr, NR_F32, nullptr, nullptr, logits_out, loss, du, dE_cols,
                               nullptr, (char*)ws, st);
}
