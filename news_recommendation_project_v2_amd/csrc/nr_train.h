// Helpers of the training kernels (train.hip and the two fused steps,
// final_train.hip / latent_train.hip): one copy of the cosine / margin loss and
// its gradient, the LayerNorm input gradient, the column fold of the LayerNorm
// parameter grads, the exact GELU derivative, the 64-group softmax backward and
// the 4-wave block sum; and the steps' host idioms (early returns, stream forks,
// token dtype dispatch, workspace cursor, shared argument checks).
#pragma once

#include "nr_common.h"
#include "nr_rows.h"

namespace nr {

template <typename T>
__device__ __forceinline__ float ldf(const T* p) {
  if constexpr (sizeof(T) == 4) return *p; else return (float)*p;
}
template <typename T>
__device__ __forceinline__ void stf(T* p, float v) {
  if constexpr (sizeof(T) == 4) *p = v; else *p = (T)v;
}

// sum of v over the 256 threads of the block (4 waves), returned to every thread
__device__ __forceinline__ float block_sum4(float v, float* scratch /* [4] */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// ----------------------------------------------------------------- cosine + margin loss
// F.cosine_similarity(u, e) = (u / max(|u|, 1e-8)) . (e / max(|e|, 1e-8))
// (data_model_helper.py / trainer.py:1058-1061), MarginRankingLoss(margin)(s_pos,
// s_neg, y=1) = mean(clamp_min(margin - (s_pos - s_neg), 0)) (trainer.py:1063-1066).
// CosDots: a thread's share of the five dot products of one batch row (user u,
// positive p, negative q); the kernel reduces the five sums (wave or block) and
// builds CosMargin from them.
struct CosDots {
  float uu = 0.f, pp = 0.f, nn = 0.f, up = 0.f, un = 0.f;
  __device__ __forceinline__ void add(float u, float p, float q) {
    uu = fmaf(u, u, uu);
    pp = fmaf(p, p, pp);
    nn = fmaf(q, q, nn);
    up = fmaf(u, p, up);
    un = fmaf(u, q, un);
  }
  template <typename Reduce>
  __device__ __forceinline__ void reduce(Reduce r) { uu = r(uu); pp = r(pp); nn = r(nn); up = r(up); un = r(un); }
};
struct CosMargin {
  float sp, sn, v, gsp, gsn, iu, ip, iq, cu, cp, cq, fB;
  __device__ __forceinline__ CosMargin(const CosDots& d, float margin, int64_t B) {
    constexpr float EPS = 1e-8f;
    const float nu = sqrtf(d.uu), np_ = sqrtf(d.pp), nq = sqrtf(d.nn);
    iu = 1.0f / fmaxf(nu, EPS); ip = 1.0f / fmaxf(np_, EPS); iq = 1.0f / fmaxf(nq, EPS);
    sp = d.up * iu * ip; sn = d.un * iu * iq;
    v = margin - (sp - sn);
    const float act = v >= 0.f ? 1.0f : 0.0f;  // clamp_min backward passes where input >= min
    fB = (float)B;
    gsp = -act / fB; gsn = act / fB;
    cu = nu > EPS ? 1.f : 0.f; cp = np_ > EPS ? 1.f : 0.f; cq = nq > EPS ? 1.f : 0.f;
  }
  __device__ __forceinline__ float loss_term() const { return fmaxf(v, 0.f) / fB; }
  // d cos(u, e) / du = (ê - [|u| > eps] cos û) / max(|u|, eps)   (û = u / max(|u|, eps))
  __device__ __forceinline__ float du(float u, float p, float q) const {
    const float uh = u * iu, ph = p * ip, qh = q * iq;
    return gsp * (ph - cu * sp * uh) * iu + gsn * (qh - cu * sn * uh) * iu;
  }
  __device__ __forceinline__ float dpos(float u, float p) const {
    const float uh = u * iu, ph = p * ip;
    return gsp * (uh - cp * sp * ph) * ip;
  }
  __device__ __forceinline__ float dneg(float u, float q) const {
    const float uh = u * iu, qh = q * iq;
    return gsn * (uh - cq * sn * qh) * iq;
  }
};

// ----------------------------------------------------------------- cosine + InfoNCE loss
// The contrastive stage (contrastive.hip) keeps the same cosine as CosMargin in
// factored form: a row v becomes its unit vector vh = v * inv with inv = 1 /
// max(|v|, 1e-8) and the clamp indicator live = [|v| > 1e-8] (CosMargin's iu / cu),
// the logits are products of unit vectors, and a gradient dvh into the unit vector
// goes back as dv = inv (dvh - live (dvh . vh) vh) -- CosMargin::du / dpos summed
// over the row's columns.
struct CosUnit {
  float inv, live;
  __device__ __forceinline__ explicit CosUnit(float sumsq) {
    constexpr float EPS = 1e-8f;
    const float n = sqrtf(sumsq);
    inv = 1.0f / fmaxf(n, EPS);
    live = n > EPS ? 1.f : 0.f;
  }
  __device__ __forceinline__ CosUnit(float inv_, float live_) : inv(inv_), live(live_) {}
  // dot = dvh . vh over the whole row
  __device__ __forceinline__ float bwd(float dvh, float vh, float dot) const { return inv * (dvh - live * dot * vh); }
};
// One row of CrossEntropyLoss (mean over B rows) over logits z with the row maximum
// m and s = sum exp(z - m) over the included columns: the row's loss term and
// dz = (softmax - onehot) / B.  A row whose only included column is its target has
// s = 1 and m = z_target: term 0 and dz 0 exactly.
struct SoftmaxCE {
  float m, inv_s, log_s, fB;
  __device__ __forceinline__ SoftmaxCE(float m_, float s, int64_t B) : m(m_), inv_s(1.0f / s), log_s(logf(s)), fB((float)B) {}
  __device__ __forceinline__ float loss_term(float z_target) const { return (log_s + (m - z_target)) / fB; }
  __device__ __forceinline__ float dz(float z, bool is_target) const {
    return (expf(z - m) * inv_s - (is_target ? 1.f : 0.f)) / fB;
  }
};

// The stage itself (contrastive.hip), shared by nr_cosine_infonce and the
// contrastive train steps.  Candidate rows E_c come either from an f32 table
// (E, lde) or, with tok, as the token LN of tok[cand[c]] (tok_dtype; tg / tb its
// affine), in which case the candidates' part of the token LN parameter grads is
// written as kCnLnChunks chunk partials [k][2][1024] into ln_part (pair_ln_kernel's
// layout: ln_reduce_kernel sums them).  loss, du [B][1024] and (nullable) dE_cols
// [Cn][1024], logits_out [B][Cn] are written whole.
constexpr int kCnLnChunks = 8;
struct CnSpec {
  int64_t B, Cn, U;  // U: rows the candidates index (0 = not known: cand is not range-checked)
  const int32_t* cand;
  const int32_t* target;
  const uint8_t* mask;
  float inv_tau;
};
int64_t contrastive_ws_bytes(int64_t B, int64_t Cn, bool from_tokens, bool own_dE);
// range checks of B / Cn, null and device checks of the spec's pointers, then target / cand /
// mask read back and every target (and, with U, every candidate) checked; no launch
int contrastive_check(const char* fn, const CnSpec& sp, hipStream_t st);
int contrastive_stage(const char* fn, const CnSpec& sp, const float* users, const float* E, int64_t lde,
                      const void* tok, int tok_dtype, const float* tg, const float* tb, float* logits_out,
                      float* loss, float* du, float* dE_cols, float* ln_part, char* ws, hipStream_t st);

// ----------------------------------------------------------------- LayerNorm backward
// dx = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)) of a row held as row_stats4
// holds it (one wave per row, NJ groups of 4 columns per lane), without the
// residual.  v: the row's x, turned into xhat in place; dxh = dy gamma;
// (layernorm_bwd_kernel, train.hip, keeps a copy of its own and says why.)  sink(j, dx) takes the lane's 4 columns 256 j + 4 lane .. + 3 (adds the kernel's
// residual, stores or accumulates).
template <int NJ, typename Sink>
__device__ __forceinline__ void ln_bwd_row(float (&v)[NJ][4], float mean, float rstd, const float (&dy)[NJ][4],
                                           const float (&gamma)[NJ][4], float dim, Sink sink) {
  float g[NJ][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[j][t] = (v[j][t] - mean) * rstd;  // xhat
      g[j][t] = dy[j][t] * gamma[j][t];   // dxhat
      s1 += g[j][t];
      s2 = fmaf(g[j][t], v[j][t], s2);
    }
  const float m1 = wave_sum(s1) / dim, m2 = wave_sum(s2) / dim;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    float dx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dx[t] = rstd * (g[j][t] - m1 - v[j][t] * m2);
    sink(j, dx);
  }
}

// LayerNorm parameter grads of a 4-wave block: each wave's per-lane register
// partials (columns 256 j + 4 lane + t) folded through LDS in a fixed order,
// then one atomic per column.  (A second fold through the same LDS needs a
// __syncthreads() before it.)
template <int NJ>
__device__ __forceinline__ void fold_cols_atomic(float (&sg)[4][NJ * 256], float (&sb)[4][NJ * 256],
                                                 const float (&ag)[NJ][4], const float (&ab)[NJ][4],
                                                 float* __restrict__ dg, float* __restrict__ db) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      sg[wave][j * 256 + lane * 4 + t] = ag[j][t];
      sb[wave][j * 256 + lane * 4 + t] = ab[j][t];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < NJ * 256; c += 256) {
    atomicAdd(dg + c, (sg[0][c] + sg[1][c]) + (sg[2][c] + sg[3][c]));
    atomicAdd(db + c, (sb[0][c] + sb[1][c]) + (sb[2][c] + sb[3][c]));
  }
}

// ----------------------------------------------------------------- GELU derivative
// gelu'(g) = Phi(g) + g phi(g) (the derivative torch's gelu backward uses): cdf =
// Phi and pdf = phi in exact f32 (erff / expf), as the forward's gelu_exact.
__device__ __forceinline__ void gelu_cdf_pdf(float g, float& cdf, float& pdf) {
  cdf = 0.5f * (1.0f + erff(g * 0.70710678118654752440f));
  pdf = 0.39894228040143267794f * expf(-0.5f * g * g);
}

// bf16 step only (the f32 step keeps erff / expf): for two values, h = erfc(|g| /
// sqrt 2) / 2 and e = exp(-g^2 / 2) with one packed polynomial and v_exp_f32, no
// branches -- the erfc form of gelu_erf2x2 (nr_common.h: erfc_poly2, its -1 folded
// in so 2^(P - s^2) = erfc / 2; relative error <= 2.2e-6 on erfc).  The divergent
// two-range erff plus expf made GEGLU's backward VALU-heavy (~65 instructions per
// element).
__device__ __forceinline__ void erfc_half2(f32x2v g, f32x2v& h, f32x2v& e) {
  const f32x2v s = g * kErfcS;
  const f32x2v c[1] = {{fminf(fabsf(s.x), kErfcSmax), fminf(fabsf(s.y), kErfcSmax)}};
  f32x2v q[1];
  erfc_poly2<1>(c, q);
  const f32x2v ns2 = -s * s, w = q[0] + ns2;
  e = (f32x2v){__builtin_amdgcn_exp2f(ns2.x), __builtin_amdgcn_exp2f(ns2.y)};
  h = (f32x2v){__builtin_amdgcn_exp2f(w.x), __builtin_amdgcn_exp2f(w.y)};
}

// ----------------------------------------------------------------- softmax64 backward
// dS = P * (dP - sum_group(P * dP)) over groups of 64 columns (one head's
// latents; SDPA softmax, latent_attention.py:72).  One wave per (row, group).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void softmax64_bwd_kernel(int64_t n_groups, int64_t groups_per_row,
                                                            const TI* __restrict__ p, int64_t ldp,
                                                            const TI* __restrict__ dp, int64_t lddp,
                                                            TO* __restrict__ ds, int64_t ldds) {
  const int lane = threadIdx.x & 63;
  for (int64_t gi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); gi < n_groups; gi += (int64_t)gridDim.x * 4) {
    const int64_t row = gi / groups_per_row, col = (gi % groups_per_row) * 64 + lane;
    const float pv = ldf<TI>(p + row * ldp + col), dv = ldf<TI>(dp + row * lddp + col);
    const float dot = wave_sum(pv * dv);
    stf<TO>(ds + row * ldds + col, pv * (dv - dot));
  }
}

// ----------------------------------------------------------------- host side of the steps
// a workspace layout: take(bytes) -> the next 256-aligned byte offset
struct WsCursor {
  int64_t o = 0;
  int64_t take(int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; }
};

// `to` goes on after everything queued on `from` so far
static inline int stream_fork(hipStream_t from, hipStream_t to, hipEvent_t ev, const char* fn, const char* what) {
  if (hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess) {
    set_error("%s: %s failed", fn, what);
    return NR_ERR_HIP;
  }
  return NR_OK;
}

// the argument checks nr_final_train_step and nr_latent_train_step share
static inline int check_step_args(const char* fn, int dtype, int tok_dtype, int64_t B, int64_t U, int64_t Hs) {
  NR_CHECK_ARG(ok_dtype(dtype), "%s: dtype must be NR_F32 or NR_BF16", fn);
  NR_CHECK_ARG(tok_dtype == NR_F32 || tok_dtype == NR_BF16 || tok_dtype == NR_F16, "%s: bad tok_dtype", fn);
  NR_CHECK_ARG(B >= 1 && U >= 1 && Hs >= 1, "%s: empty batch (B=%lld U=%lld Hs=%lld)", fn, (long long)B, (long long)U,
               (long long)Hs);
  NR_CHECK_ARG(Hs <= (1ll << 31) - 1024 && U <= (1ll << 31) && B <= (1ll << 24), "%s: batch too large", fn);
  return NR_OK;
}

// f(TypeTag<TA>, TypeTag<TT>): a step's activation / weight type and its token states' type
template <typename F>
int with_dtypes_tok(int dtype, int tok_dtype, F&& f) {
  return with_dtype(dtype, [&](auto ta) { return with_tok_dtype(tok_dtype, [&](auto tt) { return f(ta, tt); }); });
}

}  // namespace nr

// return the code of a failed internal call / report a failed HIP call of entry point fn
#define NR_TRY(...)                 \
  do {                              \
    const int rc_ = (__VA_ARGS__);  \
    if (rc_ != NR_OK) return rc_;   \
  } while (0)
#define NR_TRY_HIP(x, fn, what)                 \
  do {                                          \
    if ((x) != hipSuccess) {                    \
      nr::set_error("%s: %s failed", fn, what); \
      return NR_ERR_HIP;                        \
    }                                           \
  } while (0)
