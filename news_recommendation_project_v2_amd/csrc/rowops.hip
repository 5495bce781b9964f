// Row-wise wavefront kernels: LayerNorm, 64-wide softmax, inverse L2 norm.
// One wave per row (or per 64-group); 4 rows per 256-thread workgroup; the
// whole row lives in registers, so every element is read from HBM once and
// reductions are 64-lane butterflies (no LDS).
#include "nr_common.h"
#include "nr_rows.h"

namespace nr {

// torch.nn.LayerNorm semantics: biased variance, y = (x - mean) * rsqrt(var + eps) * g + b.
// One wave per row, rows grid-strided over a bounded grid (tiny per-row work
// would otherwise be dispatch-bound); each lane holds 16-byte chunks, so a
// wave instruction moves 1 KiB; the whole row stays in registers.
template <typename TI, typename TO, int DIM>
__global__ __launch_bounds__(256) void layernorm_kernel(int64_t rows, const TI* __restrict__ x,
                                                        int64_t ldx, const float* __restrict__ g,
                                                        const float* __restrict__ b, float eps,
                                                        TO* __restrict__ y, int64_t ldy) {
  constexpr int E = 16 / (int)sizeof(TI);           // elements per lane chunk
  constexpr int CH = DIM / E;                        // chunks per row
  constexpr int NJ = (CH + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  // affine parameters of this lane's chunks, loaded once per wave
  float gv[NJ][E], bv[NJ][E];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 64 + lane;
#pragma unroll
    for (int t = 0; t < E; ++t) {
      const bool ok = CH % 64 == 0 || c < CH;
      gv[j][t] = (g && ok) ? g[c * E + t] : 1.f;
      bv[j][t] = (b && ok) ? b[c * E + t] : 0.f;
    }
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nw) {
    float v[NJ][E];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      if (CH % 64 == 0 || c < CH) {
        if constexpr (E == 4) ld4<TI>(x + row * ldx + c * E, v[j]);
        else ld8<TI>(x + row * ldx + c * E, v[j]);
#pragma unroll
        for (int t = 0; t < E; ++t) s += v[j][t];
      }
    }
    const float mean = wave_sum(s) / (float)DIM;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      if (CH % 64 == 0 || c < CH) {
#pragma unroll
        for (int t = 0; t < E; ++t) {
          const float d = v[j][t] - mean;
          q = fmaf(d, d, q);
        }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)DIM + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      if (CH % 64 == 0 || c < CH) {
        float o[E];
#pragma unroll
        for (int t = 0; t < E; ++t) o[t] = (v[j][t] - mean) * rstd * gv[j][t] + bv[j][t];
        if constexpr (E == 4) st4<TO>(y + row * ldy + c * E, o);
        else st8<TO>(y + row * ldy + c * E, o);
      }
    }
  }
}

template <typename TO>
__global__ __launch_bounds__(256) void softmax64_kernel(int64_t items, int64_t groups,
                                                        const float* __restrict__ x, int64_t ldx,
                                                        TO* __restrict__ y, int64_t ldy) {
  const int lane = threadIdx.x & 63;
  const int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (it >= items) return;
  const int64_t row = it / groups, grp = it % groups;
  const float v = x[row * ldx + grp * 64 + lane];
  const float m = wave_max(v);
  const float e = expf(v - m);
  const float s = wave_sum(e);
  const float o = e / s;
  if constexpr (sizeof(TO) == 4) y[row * ldy + grp * 64 + lane] = o;
  else y[row * ldy + grp * 64 + lane] = (TO)o;
}

// Per-row LayerNorm statistics (mean, rstd) with the LayerNorm kernel's exact
// arithmetic (two passes over the register-resident row, biased variance):
// the bf16 latent transform applies LN inside the next GEMM's epilogue
// (gemm256t_kernel LNF) instead of writing the normalised rows.
template <typename T, int DIM>
__global__ __launch_bounds__(256) void row_stats_kernel(int64_t rows, const T* __restrict__ x, int64_t ldx,
                                                        float eps, float2* __restrict__ out) {
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int NJ = DIM / (64 * E);
  static_assert(DIM % (64 * E) == 0, "row_stats: DIM must be a multiple of 64 lanes x 16 B");
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nw) {
    float v[NJ][E];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if constexpr (E == 4) ld4<T>(x + row * ldx + (j * 64 + lane) * E, v[j]);
      else ld8<T>(x + row * ldx + (j * 64 + lane) * E, v[j]);
#pragma unroll
      for (int t = 0; t < E; ++t) s += v[j][t];
    }
    const float mean = wave_sum(s) / (float)DIM;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int t = 0; t < E; ++t) {
        const float d = v[j][t] - mean;
        q = fmaf(d, d, q);
      }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)DIM + eps);
    if (lane == 0) out[row] = make_float2(mean, rstd);
  }
}

template <typename T, int DIM>
__global__ __launch_bounds__(256) void inv_norm_kernel(int64_t rows, const T* __restrict__ x,
                                                       int64_t ldx, float eps,
                                                       float* __restrict__ out) {
  constexpr int NJ = DIM / 256;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    float v[4];
    ld4<T>(x + row * ldx + j * 256 + lane * 4, v);
#pragma unroll
    for (int t = 0; t < 4; ++t) q = fmaf(v[t], v[t], q);
  }
  q = wave_sum(q);
  if (lane == 0) out[row] = 1.0f / fmaxf(sqrtf(q), eps);
}

// the miss path of the row-width dispatch (with_int) of entry point fn
static int dim_unsupported(const char* fn, int64_t dim, int rc) {
  set_error("%s: dim %lld unsupported", fn, (long long)dim);
  return rc;
}

int layernorm_dispatch(int dti, int dto, int64_t rows, int64_t dim, const void* x, int64_t ldx,
                       const float* g, const float* b, float eps, void* y, int64_t ldy,
                       hipStream_t s) {
  NR_CHECK_ARG(ok_dtype(dti) && ok_dtype(dto), "nr_layernorm: bad dtype");
  NR_CHECK_ARG(rows >= 0 && ldx >= dim && ldy >= dim, "nr_layernorm: bad strides");
  NR_CHECK_ARG((ldx * (dti == NR_F32 ? 4 : 2)) % 16 == 0 && (ldy * (dto == NR_F32 ? 4 : 2)) % 16 == 0 &&
                   ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0,
               "nr_layernorm: rows must be 16-byte aligned");
  if (rows == 0) return NR_OK;
  NR_CHECK_ARG(x && y, "nr_layernorm: null pointer");
  const int64_t nb = (rows + 3) / 4;
  constexpr int64_t cap = 1024;  // grid cap (measured best for bf16 at 72k rows)
  const dim3 grid((unsigned)(cap > 0 && nb > cap ? cap : nb));  // rows grid-strided over <= cap blocks
  const auto miss = [&] { return dim_unsupported("nr_layernorm", dim, NR_ERR_UNSUPPORTED); };
  return with_dtypes(dti, dto, [&](auto ti, auto to) -> int {
    using TI = typename decltype(ti)::type;
    using TO = typename decltype(to)::type;
    return with_int<256, 512, 768, 1024, 2048>(dim, miss, [&](auto d) -> int {
      hipLaunchKernelGGL((layernorm_kernel<TI, TO, decltype(d)::value>), grid, dim3(256), 0, s, rows, (const TI*)x,
                         ldx, g, b, eps, (TO*)y, ldy);
      NR_CHECK_LAUNCH("nr_layernorm");
      return NR_OK;
    });
  });
}

int softmax64_dispatch(int64_t rows, int64_t groups, const float* x, int64_t ldx, int dto, void* y,
                       int64_t ldy, hipStream_t s) {
  NR_CHECK_ARG(rows >= 0 && groups > 0 && ldx >= groups * 64 && ldy >= groups * 64, "nr_softmax64: bad shape");
  NR_CHECK_ARG(ok_dtype(dto), "nr_softmax64: bad dtype");
  if (rows == 0) return NR_OK;
  NR_CHECK_ARG(x && y, "nr_softmax64: null pointer");
  const int64_t items = rows * groups;
  const dim3 grid((unsigned)((items + 3) / 4));
  return with_dtype(dto, [&](auto to) -> int {
    using TO = typename decltype(to)::type;
    hipLaunchKernelGGL((softmax64_kernel<TO>), grid, dim3(256), 0, s, items, groups, x, ldx, (TO*)y, ldy);
    NR_CHECK_LAUNCH("nr_softmax64");
    return NR_OK;
  });
}

int inv_norm_dispatch(int dtype, int64_t rows, int64_t dim, const void* x, int64_t ldx, float eps,
                      float* out, hipStream_t s) {
  NR_CHECK_ARG(ok_dtype(dtype), "nr_row_inv_norm: bad dtype");
  NR_CHECK_ARG(rows >= 0 && ldx >= dim && ldx % 4 == 0, "nr_row_inv_norm: bad strides");
  if (rows == 0) return NR_OK;
  NR_CHECK_ARG(x && out, "nr_row_inv_norm: null pointer");
  const dim3 grid((unsigned)((rows + 3) / 4));
  const auto miss = [&] { return dim_unsupported("nr_row_inv_norm", dim, NR_ERR_UNSUPPORTED); };
  return with_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    return with_int<256, 512, 768, 1024, 2048>(dim, miss, [&](auto d) -> int {
      hipLaunchKernelGGL((inv_norm_kernel<T, decltype(d)::value>), grid, dim3(256), 0, s, rows, (const T*)x, ldx,
                         eps, out);
      NR_CHECK_LAUNCH("nr_row_inv_norm");
      return NR_OK;
    });
  });
}

// Gathered chain of LayerNorms: out[i] = LN_{n-1}(...LN_0(x[row_idx[i]])...),
// f32 math and output.  The token-attention encoder's effective forward
// (attention.py:174-194 returns g_mlp_layernorm(hidden_states); the attention
// branch is dead) followed by last_token_pool (modeling_utils.py:37-48) is one
// such LN of the last valid token row, so only those rows are ever read.
template <typename TI, int DIM>
__global__ __launch_bounds__(256) void gather_ln_kernel(int64_t n, const TI* __restrict__ x, int64_t ldx,
                                                        const int64_t* __restrict__ row_idx, int n_ln,
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        float eps, float* __restrict__ y, int64_t ldy) {
  constexpr int NJ = DIM / 256;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t row = row_idx ? row_idx[i] : i;
  float v[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) ld4<TI>(x + row * ldx + j * 256 + lane * 4, v[j]);
  for (int l = 0; l < n_ln; ++l) {
    float mean, rstd;
    row_stats4<NJ>(v, (float)DIM, eps, mean, rstd);
    const float* gl = g ? g + (int64_t)l * DIM : nullptr;
    const float* bl = b ? b + (int64_t)l * DIM : nullptr;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int e = j * 256 + lane * 4 + t;
        v[j][t] = (v[j][t] - mean) * rstd * (gl ? gl[e] : 1.f) + (bl ? bl[e] : 0.f);
      }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) st4<float>(y + i * ldy + j * 256 + lane * 4, v[j]);
}

int gather_ln_dispatch(int dti, int64_t n, int64_t dim, const void* x, int64_t ldx, const int64_t* row_idx,
                       int n_ln, const float* g, const float* b, float eps, float* y, int64_t ldy,
                       hipStream_t s) {
  NR_CHECK_ARG(dti == NR_F32 || dti == NR_BF16 || dti == NR_F16, "nr_gather_layernorm: bad dtype");
  NR_CHECK_ARG(n >= 0 && n_ln >= 0 && ldx >= dim && ldy >= dim && ldx % 4 == 0 && ldy % 4 == 0,
               "nr_gather_layernorm: bad shape/strides");
  if (n == 0) return NR_OK;
  NR_CHECK_ARG(x && y, "nr_gather_layernorm: null pointer");
  const dim3 grid((unsigned)((n + 3) / 4));
  const auto miss = [&] { return dim_unsupported("nr_gather_layernorm", dim, NR_ERR_INVALID); };
  return with_tok_dtype(dti, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    return with_int<256, 512, 1024, 2048>(dim, miss, [&](auto d) -> int {
      hipLaunchKernelGGL((gather_ln_kernel<T, decltype(d)::value>), grid, dim3(256), 0, s, n, (const T*)x, ldx,
                         row_idx, n_ln, g, b, eps, y, ldy);
      NR_CHECK_LAUNCH("nr_gather_layernorm");
      return NR_OK;
    });
  });
}

int row_stats_dispatch(int dtype, int64_t rows, int64_t dim, const void* x, int64_t ldx, float eps, float* out,
                       hipStream_t s) {
  NR_CHECK_ARG(ok_dtype(dtype), "nr_row_stats: bad dtype");
  NR_CHECK_ARG(dim == 1024, "nr_row_stats: dim %lld unsupported (1024 only)", (long long)dim);
  NR_CHECK_ARG(rows >= 0 && ldx >= dim && (ldx * (dtype == NR_F32 ? 4 : 2)) % 16 == 0 && ((uintptr_t)x & 15) == 0 &&
                   ((uintptr_t)out & 7) == 0,
               "nr_row_stats: rows must be 16-byte aligned, out 8-byte aligned");
  if (rows == 0) return NR_OK;
  NR_CHECK_ARG(x && out, "nr_row_stats: null pointer");
  const int64_t nb = (rows + 3) / 4;
  const dim3 grid((unsigned)(nb > 2048 ? 2048 : nb));
  return with_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((row_stats_kernel<T, 1024>), grid, dim3(256), 0, s, rows, (const T*)x, ldx, eps, (float2*)out);
    NR_CHECK_LAUNCH("nr_row_stats");
    return NR_OK;
  });
}

}  // namespace nr

extern "C" int nr_gather_layernorm(int dtype_in, int64_t n, int64_t dim, const void* x, int64_t ldx,
                                   const int64_t* row_idx, int n_ln, const float* gammas, const float* betas,
                                   float eps, float* out, int64_t ldo, void* stream) {
  nr::clear_error();
  if (n > 0) NR_CHECK_DEVICE("nr_gather_layernorm", x, row_idx, gammas, betas, out);
  return nr::gather_ln_dispatch(dtype_in, n, dim, x, ldx, row_idx, n_ln, gammas, betas, eps, out, ldo,
                                (hipStream_t)stream);
}

extern "C" int nr_layernorm(int dtype_in, int dtype_out, int64_t rows, int64_t dim, const void* x,
                            int64_t ldx, const float* gamma, const float* beta, float eps, void* y,
                            int64_t ldy, void* stream) {
  nr::clear_error();
  if (rows > 0) NR_CHECK_DEVICE("nr_layernorm", x, gamma, beta, y);
  return nr::layernorm_dispatch(dtype_in, dtype_out, rows, dim, x, ldx, gamma, beta, eps, y, ldy,
                                (hipStream_t)stream);
}

extern "C" int nr_softmax64(int64_t rows, int64_t groups, const float* x, int64_t ldx,
                            int dtype_out, void* y, int64_t ldy, void* stream) {
  nr::clear_error();
  if (rows > 0) NR_CHECK_DEVICE("nr_softmax64", x, y);
  return nr::softmax64_dispatch(rows, groups, x, ldx, dtype_out, y, ldy, (hipStream_t)stream);
}

extern "C" int nr_row_inv_norm(int dtype, int64_t rows, int64_t dim, const void* x, int64_t ldx,
                               float eps, float* out, void* stream) {
  nr::clear_error();
  if (rows > 0) NR_CHECK_DEVICE("nr_row_inv_norm", x, out);
  return nr::inv_norm_dispatch(dtype, rows, dim, x, ldx, eps, out, (hipStream_t)stream);
}

extern "C" int nr_row_stats(int dtype, int64_t rows, int64_t dim, const void* x, int64_t ldx, float eps, float* out,
                            void* stream) {
  nr::clear_error();
  if (rows > 0) NR_CHECK_DEVICE("nr_row_stats", x, out);
  return nr::row_stats_dispatch(dtype, rows, dim, x, ldx, eps, out, (hipStream_t)stream);
}
