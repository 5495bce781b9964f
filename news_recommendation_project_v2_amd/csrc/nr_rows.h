// Device helpers shared by the row kernels (rowops.hip, train.hip and the two
// training steps): lane loads / stores of 4 and 8 consecutive elements, the
// pairwise LayerNorm row statistics and the token LayerNorm built on them, exact
// GELU, the sum-of-squares thread loop and the 64x64 transpose tile bodies.  One
// copy each, so the kernels that promise each other's bits share the arithmetic.
#pragma once

#include "nr_common.h"

#include <type_traits>

namespace nr {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {  // one v_cvt_pk_bf16_f32 (RNE)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

// 4 consecutive elements as one 8-B (16-bit types) / 16-B (f32) access; the
// callers keep p aligned to the access (bases, row strides and column offsets
// multiples of 4 elements).
template <typename T>
__device__ __forceinline__ void ld4(const T* p, float (&v)[4]) {
  if constexpr (std::is_same<T, _Float16>::value) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const h4 h = *reinterpret_cast<const h4*>(p);
    v[0] = (float)h[0]; v[1] = (float)h[1]; v[2] = (float)h[2]; v[3] = (float)h[3];
  } else if constexpr (sizeof(T) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v[0] = bf16_lo(u.x); v[1] = bf16_hi(u.x); v[2] = bf16_lo(u.y); v[3] = bf16_hi(u.y);
  }
}
template <typename T>
__device__ __forceinline__ void st4(T* p, const float (&v)[4]) {
  if constexpr (sizeof(T) == 4) *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], v[3]};
  else *reinterpret_cast<uint2*>(p) = uint2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}
template <typename T>
__device__ __forceinline__ void st4z(T* p) {
  const float z[4] = {0.f, 0.f, 0.f, 0.f};
  st4<T>(p, z);
}

// 8 consecutive elements: one 16-B access (bf16) or two (f32).
template <typename T>
__device__ __forceinline__ void ld8(const T* p, float (&v)[8]) {
  if constexpr (sizeof(T) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    v[0] = bf16_lo(u.x); v[1] = bf16_hi(u.x); v[2] = bf16_lo(u.y); v[3] = bf16_hi(u.y);
    v[4] = bf16_lo(u.z); v[5] = bf16_hi(u.z); v[6] = bf16_lo(u.w); v[7] = bf16_hi(u.w);
  }
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const float (&v)[8]) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<float4*>(p + 4) = float4{v[4], v[5], v[6], v[7]};
  } else {
    *reinterpret_cast<uint4*>(p) = uint4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                         pack_bf16x2(v[6], v[7])};
  }
}

// LayerNorm statistics of a row held as NJ groups of 4 columns per lane (one
// wave per row, biased variance, two passes over the registers): the per-group
// pairwise sum, then squared deviations chained in (j, t) order.  This order is
// the bits of nr_gather_layernorm, the training steps' token LN and every LN
// backward that recomputes its forward's statistics.
template <int NJ>
__device__ __forceinline__ void row_stats4(const float (&v)[NJ][4], float dim, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  mean = wave_sum(s) / dim;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float d = v[j][t] - mean;
      q = fmaf(d, d, q);
    }
  rstd = 1.0f / sqrtf(wave_sum(q) / dim + eps);
}

// The token model's output row (g_mlp_layernorm, 1024 columns, eps 1e-12)
// without its affine: lane's 4 x 4 columns 256 j + 4 lane .. +3 of xhat, the
// arithmetic of nr_gather_layernorm.  TT = the token states' type (f32 / bf16 / f16).
template <typename TT>
__device__ __forceinline__ void tok_xhat(const TT* row, int lane, float (&v)[4][4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) ld4<TT>(row + j * 256 + lane * 4, v[j]);
  float mean, rstd;
  row_stats4<4>(v, 1024.f, 1e-12f, mean, rstd);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) v[j][t] = (v[j][t] - mean) * rstd;
}

__device__ __forceinline__ float gelu_exact(float g) { return 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f)); }

// s + the squares of thread t's share of x[0 .. n) under a grid stride of gs
// threads: 16-B loads when x is 16-B aligned, four in flight per thread (one per
// iteration left the loop latency-bound), then a float4 tail and a scalar tail.
__device__ __forceinline__ float sumsq_range(const float* x, int64_t n, int64_t t, int64_t gs, float s = 0.f) {
  const int64_t n4 = ((uintptr_t)x & 15) == 0 ? n / 4 : 0;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  int64_t i = t;
  for (; i + 3 * gs < n4; i += 4 * gs) {
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x4[i + k * gs];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s = fmaf(v[k].x, v[k].x, s);
      s = fmaf(v[k].y, v[k].y, s);
      s = fmaf(v[k].z, v[k].z, s);
      s = fmaf(v[k].w, v[k].w, s);
    }
  }
  for (; i < n4; i += gs) {
    const float4 v = x4[i];
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  for (int64_t k = 4 * n4 + t; k < n; k += gs) s = fmaf(x[k], x[k], s);
  return s;
}

// dst[c][r] = load(r, c) for the 64x64 tile at (r0, c0) through a 64x65 f32 LDS
// tile (256 threads); dst gets zero columns [rows, rows_pad).  `load` is a
// by-value lambda over the kernel's source (a by-reference capture costs an
// address add per element).
template <typename TO, typename Load>
__device__ __forceinline__ void transpose_tile(Load load, TO* dst, int64_t ldd, int64_t rows, int64_t rows_pad,
                                               int64_t cols, int64_t r0, int64_t c0, float (&tile)[64][65]) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int rr = ty + 4 * k;
    const int64_t r = r0 + rr, c = c0 + tx;
    tile[rr][tx] = (r < rows && c < cols) ? load(r, c) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int cc = ty + 4 * k;
    const int64_t c = c0 + cc, r = r0 + tx;
    if (c < cols && r < rows_pad) dst[c * ldd + r] = (TO)tile[tx][cc];
  }
}

// 16-bit -> 16-bit transpose of a 64x64 tile with 16-B global accesses: each
// lane loads 8 consecutive columns of a row (2 per lane), the tile sits in LDS
// as u16 rows of pitch 66 (odd dword pitch: the column reads below are at most
// 2-way), and each lane writes 8 consecutive source rows of one column as one
// 16-B store (8 lanes = one 128-B output row segment).  Needs rows_pad, cols,
// strides multiple of 8 and 16-B aligned bases (checked by the caller).
constexpr int kT16Pitch = 66;
__device__ __forceinline__ void transpose_tile16(const uint16_t* src, int64_t lds, uint16_t* dst, int64_t ldd,
                                                 int64_t rows, int64_t rows_pad, int64_t cols, int64_t r0, int64_t c0,
                                                 uint16_t (&tile)[64 * kT16Pitch]) {
  constexpr int P = kT16Pitch;
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int rr = (t >> 3) + 32 * k, ch = t & 7;
    const int64_t r = r0 + rr, c = c0 + 8 * ch;
    uint4 u = make_uint4(0, 0, 0, 0);
    if (r < rows && c < cols) u = *reinterpret_cast<const uint4*>(src + r * lds + c);
    uint32_t* d = reinterpret_cast<uint32_t*>(tile + rr * P + 8 * ch);  // 4-B aligned (P even)
    d[0] = u.x; d[1] = u.y; d[2] = u.z; d[3] = u.w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int oc = (t >> 3) + 32 * k, rc = t & 7;
    const int64_t c = c0 + oc, r = r0 + 8 * rc;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = (uint32_t)tile[(8 * rc + 2 * j) * P + oc] | ((uint32_t)tile[(8 * rc + 2 * j + 1) * P + oc] << 16);
    if (c < cols && r < rows_pad) *reinterpret_cast<uint4*>(dst + c * ldd + r) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace nr
