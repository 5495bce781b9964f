// The users x news score tile that top-K retrieval (topk.hip) and the full-table ranks
// (fullrank.hip) share: ONE copy of the tile main loop, so that the bits of a (user, news)
// selection score are the same in both (include/newsrec_topk.h, "Selection scores" and
// "Position independence"; include/newsrec_fullrank.h rests its consistency contract on it).
//
//   ScoreTile<TI>  gemm_kernel's main loop (gemm.hip: 128 x 128 tile, K in 128-byte row slices
//                  through a two-stage LDS ring, the next slice's global loads in flight over
//                  the MFMAs; f32 on v_mfma_f32_32x32x2_f32, bf16 on v_mfma_f32_16x16x32_bf16)
//                  with the NEWS rows as the A operand, so a lane's accumulator registers are 4
//                  consecutive news of one user; then scale by cand_inv (-inf past the valid
//                  rows) and 16-byte stores into an LDS score tile [user][news] that aliases
//                  the operand ring.  Which table row feeds news row r of the tile is the
//                  caller's (a run of consecutive rows, or gathered rows).
//   Excluded       a user's excluded rows inside the current chunk, staged in LDS once per
//                  chunk as 16-bit offsets; a user with more than XCAP of them has its rows set
//                  to -inf in every score tile by the whole workgroup instead.
//   FilterOf<FILT> the catalogue filter (include/newsrec_filter.h): Eligible in the filtered
//                  instantiations, a predicate on the finished score tile, never on the product.
//   PRIOR          the rank-one prior (include/newsrec_prior.h): the PRIOR instantiations of
//                  ScoreTile add gsel[user] * prior[news] where the tile is scaled, from two
//                  small LDS arrays, so every epilogue sees selection KEYS in the score tile.
//   ChunkWalk      a workgroup's walk over its run of chunks with the three above: everything
//                  around the kernel's own epilogue over a finished score tile (a heap, a count).
//   ScanArgs       host side: what nr_topk_users* and nr_rank_targets* take alike, with its
//                  validation, launch preparation and (dtype, filtered) -> <TI, FILT> dispatch.
//   TopkLayout     host side: the workspace of a top-K and its stage 2 (topk.hip), which the
//                  sectioned top-K (sections.hip) runs over S lists per user.
#pragma once

#include "nr_common.h"

namespace nr {
namespace tk {

constexpr int64_t D = 1024;
constexpr int64_t kChunk = 16384;  // news rows per stage-1 partial (< 2^16: exclusions are staged as 16-bit offsets)
constexpr int kMaxChunks = 256;   // chunk heads the merge keeps per user (N <= 2^22)
constexpr int kFillWorkgroups = 1024;  // workgroups wanted before chunks are walked in sequence
constexpr int XCAP = 32;          // excluded rows of one chunk staged in LDS per user (more: the global list is searched)
constexpr int TS = 128;           // tile side: users and news rows per tile
constexpr int ROWW = 36;          // LDS words per staged 128-byte row slice (144 B: conflict-free b128 reads)
constexpr int TILE_WORDS = TS * ROWW;
constexpr int TLD = 132;          // score tile row stride, floats
static_assert(kChunk % 256 == 0 && kChunk <= 65536 && TS * TLD <= 4 * TILE_WORDS, "score tile must fit the operand ring");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// (score descending, row ascending)
__device__ __forceinline__ bool better(float s, int32_t r, float s2, int32_t r2) {
  return s > s2 || (s == s2 && r < r2);
}

// NR_BF16: users f32 -> bf16 rows (round to nearest even), U * D / 8 groups of 8 (topk.hip)
int bf16_users_launch(int64_t U, const float* users, __bf16* out, hipStream_t st, const char* fn);
// the prior's scaled gains, gsel[u] = gain[u] * max(|users[u]|, 1e-8): one wave per user (topk.hip)
int prior_gains_launch(int64_t U, const float* users, const float* gain, float* gsel, hipStream_t st, const char* fn);

// How many chunks one workgroup walks in sequence: chunks only run side by side while the
// user blocks alone do not fill the device.
static inline int64_t chunk_span(int64_t U, int64_t nchunks) {
  const int64_t ublocks = (U + TS - 1) / TS;
  int64_t span = nchunks;
  while (span > 1 && ublocks * ((nchunks + span - 1) / span) < kFillWorkgroups) --span;
  return span;
}

template <typename TI> struct Acc { typedef f32x16 type[2][2]; };  // [news 32-block][user 32-block]
template <> struct Acc<__bf16> { typedef f32x4 type[4][4]; };      // [news 16-block][user 16-block]

// The two operations of a key (include/newsrec_prior.h), each rounded on its own: never
// contracted into an fma, whatever the translation unit's default, so a host can recompute
// the bits with two f32 operations.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// The prior as the kernels take it: news_prior [N] and gsel [U], the scaled gains that the
// pre-pass left in the workspace.  The PRIOR = false instantiations never read it.
struct PriorArgs {
  const float* news_prior = nullptr;
  const float* gsel = nullptr;
};

// The cursor as the stage-1 kernels with one take it (include/newsrec_page.h): [U] and [U].  The
// AFTER = false instantiations never read it.
struct AfterArgs {
  const float* key = nullptr;
  const int32_t* row = nullptr;
};

template <typename TI, bool PRIOR = false>
struct ScoreTile {
  static constexpr int BK = 128 / (int)sizeof(TI);
  static constexpr int NKT = (int)D / BK;  // K tiles per product (even: a tile starts on ring stage 0)

  uint32_t* smem;  // ring [2][news | users], 4 * TILE_WORDS words, 16-byte aligned; the score tile aliases it
  float* cinv_s;   // [TS] cand_inv of the tile's news rows, 16-byte aligned (the caller fills it before scores())
  float* prior_s;  // PRIOR: [TS] the priors of the tile's news rows, 16-byte aligned (filled where cinv_s is)
  float* gsel_s;   // PRIOR: [TS] the scaled gains of the block's users (filled once, before the first scores())
  int tid, lane, wm, wn;  // wm: news half, wn: user half
  // global -> register staging map: 4 chunks of 16 B per operand per thread; rows past U
  // are clamped for the loads (their scores are never selected)
  int soff[4];
  const u32x4* gu[4];
  u32x4 rn[4], ru[4];
  typename Acc<TI>::type acc;

  __device__ __forceinline__ ScoreTile(uint32_t* smem_, float* cinv_s_, const TI* users, int64_t m0, int64_t U,
                                       float* prior_s_ = nullptr, float* gsel_s_ = nullptr)
      : smem(smem_), cinv_s(cinv_s_), prior_s(prior_s_), gsel_s(gsel_s_) {
    tid = threadIdx.x;
    lane = tid & 63;
    const int wave = tid >> 6;
    wm = wave >> 1;
    wn = wave & 1;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int id = tid + 256 * p;
      soff[p] = (id >> 3) * ROWW + (id & 7) * 4;
      gu[p] = reinterpret_cast<const u32x4*>(users + min(m0 + (id >> 3), U - 1) * D) + (id & 7);
    }
  }

  __device__ __forceinline__ float* tile() const { return reinterpret_cast<float*>(smem); }

  // rows(r): the table row (int64, inside the table) behind news row r of the tile
  template <typename Rows>
  __device__ __forceinline__ void gload(const TI* __restrict__ tab, int64_t ldt, Rows rows, int kt) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int id = tid + 256 * p;
      rn[p] = (reinterpret_cast<const u32x4*>(tab + rows(id >> 3) * ldt) + (id & 7))[kt * 8];
      ru[p] = gu[p][kt * 8];
    }
  }
  __device__ __forceinline__ void lstore(int buf) {
    uint32_t* Ns = smem + buf * 2 * TILE_WORDS;
    uint32_t* Us = Ns + TILE_WORDS;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *reinterpret_cast<u32x4*>(Ns + soff[p]) = rn[p];
      *reinterpret_cast<u32x4*>(Us + soff[p]) = ru[p];
    }
  }
  __device__ __forceinline__ void compute(int buf) {
    const uint32_t* Ns = smem + buf * 2 * TILE_WORDS;
    const uint32_t* Us = Ns + TILE_WORDS;
    if constexpr (sizeof(TI) == 4) {
      // lane (r, h) covers k = 16h + 4q + t of the 32-deep slice (news and users alike)
      const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 nf[2], uf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          nf[i] = *reinterpret_cast<const f32x4*>(Ns + (wm * 64 + 32 * i + fr) * ROWW + 16 * fh + 4 * q);
          uf[i] = *reinterpret_cast<const f32x4*>(Us + (wn * 64 + 32 * i + fr) * ROWW + 16 * fh + 4 * q);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(nf[i][t], uf[j][t], acc[i][j], 0, 0, 0);
      }
    } else {
      // lane (r, g) holds k = 32 ks + 8 g + j, j < 8, of row r (16x16x32 operand map)
      const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 nf[4], uf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          nf[i] = *reinterpret_cast<const bf16x8*>(Ns + (wm * 64 + 16 * i + fr) * ROWW + 16 * ks + 4 * fg);
          uf[i] = *reinterpret_cast<const bf16x8*>(Us + (wn * 64 + 16 * i + fr) * ROWW + 16 * ks + 4 * fg);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf[i], uf[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  // one group of 4 consecutive news of one user: scaled, -inf past the valid rows, into the score tile
  __device__ __forceinline__ void put4(int ul, int nl, float a0, float a1, float a2, float a3, int nvalid) {
    const float NINF = -__builtin_inff();
    const float4 ci = *reinterpret_cast<const float4*>(cinv_s + nl);
    float4 v;
    if constexpr (PRIOR) {
      // sel + gsel * prior; the scaled score inside it has the PRIOR = false bits
      const float4 pr = *reinterpret_cast<const float4*>(prior_s + nl);
      const float g = gsel_s[ul];
      v.x = nl + 0 < nvalid ? add_rn(mul_rn(a0, ci.x), mul_rn(g, pr.x)) : NINF;
      v.y = nl + 1 < nvalid ? add_rn(mul_rn(a1, ci.y), mul_rn(g, pr.y)) : NINF;
      v.z = nl + 2 < nvalid ? add_rn(mul_rn(a2, ci.z), mul_rn(g, pr.z)) : NINF;
      v.w = nl + 3 < nvalid ? add_rn(mul_rn(a3, ci.w), mul_rn(g, pr.w)) : NINF;
    } else {
      v.x = nl + 0 < nvalid ? a0 * ci.x : NINF;
      v.y = nl + 1 < nvalid ? a1 * ci.y : NINF;
      v.z = nl + 2 < nvalid ? a2 * ci.z : NINF;
      v.w = nl + 3 < nvalid ? a3 * ci.w : NINF;
    }
    *reinterpret_cast<float4*>(tile() + ul * TLD + nl) = v;
  }

  // One score tile.  On entry the tile's first K slice is in rn / ru (a gload(.., rows, 0))
  // and cinv_s is written; on return the score tile tile()[user * TLD + news] is complete and
  // visible to the workgroup, and, if `more`, the first slice of the tile behind `next` is
  // in flight (it lands over the caller's epilogue).  The caller ends its epilogue with a
  // barrier before the next call: the operands overwrite the score tile.
  template <typename Rows, typename Next>
  __device__ __forceinline__ void scores(const TI* __restrict__ tab, int64_t ldt, Rows rows, bool more, Next next,
                                         int nvalid) {
    lstore(0);
    __syncthreads();
    if constexpr (sizeof(TI) == 4) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    }
    for (int kt = 0; kt < NKT; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < NKT) gload(tab, ldt, rows, kt + 1);
      else if (more) gload(tab, ldt, next, 0);  // lands over the epilogue
      compute(cur);
      if (kt + 1 < NKT) lstore(cur ^ 1);
      __syncthreads();
    }
    // ---- score tile (aliases the ring: every wave is past its last fragment read)
    if constexpr (sizeof(TI) == 4) {
      // C/D map: col (user) = lane & 31, row (news) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            put4(wn * 64 + 32 * j + (lane & 31), wm * 64 + 32 * i + 8 * g + 4 * (lane >> 5), acc[i][j][4 * g],
                 acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], nvalid);
    } else {
      // C/D map: col (user) = lane & 15, row (news) = 4 (lane >> 4) + reg
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          put4(wn * 64 + 16 * j + (lane & 15), wm * 64 + 16 * i + 4 * (lane >> 4), acc[i][j][0], acc[i][j][1],
               acc[i][j][2], acc[i][j][3], nvalid);
    }
    __syncthreads();
  }
};

// Threads 2u and 2u + 1 serve user u of the block; 2u (sh == 0) owns its staged list.
struct Excluded {
  uint16_t* ex_s;     // [XCAP * TS] the users' excluded rows inside the current chunk, [slot][user], minus its first row
  uint32_t* ov_mask;  // [TS / 32] users with more than XCAP of them: knocked out of every score tile instead
  const int32_t* excl_idx;
  const int64_t* excl_off;
  int su;
  int64_t e0, e1;
  int xn;      // the owner's excluded rows inside the current chunk (all of them; XCAP are staged)
  int64_t cb;  // the current chunk's first row

  __device__ __forceinline__ Excluded(uint16_t* ex_s_, uint32_t* ov_mask_, const int32_t* excl_idx_,
                                      const int64_t* excl_off_, int64_t m0, bool live, int64_t c0)
      : ex_s(ex_s_), ov_mask(ov_mask_), excl_idx(excl_idx_), excl_off(excl_off_), su(threadIdx.x >> 1), e0(0), e1(0),
        xn(0), cb(c0) {
    if (excl_off && live) {
      e0 = excl_off[m0 + su];
      e1 = excl_off[m0 + su + 1];
    }
  }
  // A chunk starts at row n0: clear the overflow mask, barrier, the owners stage their rows
  // (read after the tile's first barrier).  Called by every thread.
  __device__ __forceinline__ void chunk_start(int64_t n0) {
    cb = n0;
    if (threadIdx.x < TS / 32) ov_mask[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 1) == 0) {
      xn = 0;
#pragma unroll 4
      for (int64_t e = e0; e < e1; ++e) {
        const int64_t d = (int64_t)excl_idx[e] - cb;
        if (d >= 0 && d < kChunk) {
          if (xn < XCAP) ex_s[xn * TS + su] = (uint16_t)d;
          ++xn;
        }
      }
      if (xn > XCAP) atomicOr(&ov_mask[su >> 5], 1u << (su & 31));
    }
  }
  // owner only: is `row` (of the current chunk) on the staged list?
  __device__ __forceinline__ bool staged(int32_t row) const {
    if (xn > XCAP) return false;  // such a user's excluded rows are -inf in the score tile already
    const int d = (int)(row - cb);
    bool hit = false;
    for (int i = 0; i < xn; ++i) hit |= ex_s[i * TS + su] == d;
    return hit;
  }
  // users with too many excluded rows for the staged list: every thread walks their lists and
  // writes -inf into the score tile T of news rows [n0, n0 + TS).  Called by every thread.
  __device__ __forceinline__ void knock_out_overflow(float* T, int64_t m0, int64_t n0) {
    const float NINF = -__builtin_inff();
    bool any = false;
#pragma unroll
    for (int w = 0; w < TS / 32; ++w) {
      uint32_t bits = ov_mask[w];  // block-uniform
      while (bits) {
        const int u = 32 * w + __builtin_ctz(bits);
        bits &= bits - 1;
        any = true;
        const int64_t b = excl_off[m0 + u + 1];
        for (int64_t e = excl_off[m0 + u] + threadIdx.x; e < b; e += 256) {
          const int64_t d = (int64_t)excl_idx[e] - n0;
          if (d >= 0 && d < TS) T[u * TLD + (int)d] = NINF;
        }
      }
    }
    if (any) __syncthreads();
  }
};

// The catalogue filter of include/newsrec_filter.h: per-news attributes, per-user window and
// category mask.  A null pair passes every row.
struct FilterArgs {
  const int32_t* news_time = nullptr;
  const int32_t* q_lo = nullptr;
  const int32_t* q_hi = nullptr;
  const uint8_t* news_cat = nullptr;
  const uint64_t* q_mask = nullptr;
  bool any() const { return news_time || news_cat; }
};

constexpr int ATTR_HALF = TS / 2 + 4;  // words between the two 64-row halves of the staged times (see Eligible)
constexpr int ATTR_TIME_WORDS = ATTR_HALF + TS / 2;
constexpr int ATTR_CAT_WORDS = TS / 4;

// the predicate as include/newsrec_filter.h states it (one target at a time: rank_thresholds_kernel)
__device__ __forceinline__ bool in_window(int32_t t, int32_t lo, int32_t hi) { return t >= lo && t <= hi; }
__device__ __forceinline__ bool in_mask(uint32_t cat, uint64_t mask) { return cat < 64 && ((mask >> (cat & 63)) & 1) != 0; }

// Threads 2u and 2u + 1 serve user u of the block: its window and mask live in their registers,
// the tile's 128 times and 128 categories in LDS (staged once per tile next to cinv_s).  Thread
// half sh reads rows [64 sh, 64 sh + 64): every lane of a half reads one address (a broadcast),
// and the second half of the times sits 4 words past a whole number of bank rows, so the two
// b128 addresses of a wave never meet in a bank.  A null pair is staged as zeros against the
// widest window / the full mask, so the test has no branch on it.  The window test is one
// unsigned compare, (t - lo) <= (hi - lo) in 32-bit wrap-around arithmetic (exact for every
// lo <= hi); an empty window (lo > hi) is held as the mask 0 instead.
struct Eligible {
  static constexpr int SPARSE_MAX = 8;  // scan survivors per thread up to which only they are tested
  int32_t* t_s;   // [ATTR_TIME_WORDS]
  uint32_t* c_s;  // [ATTR_CAT_WORDS], one byte per news row
  const int32_t* news_time;
  const uint8_t* news_cat;
  uint32_t lo, span, mask_lo, mask_hi;

  __device__ __forceinline__ Eligible(int32_t* t_s_, uint32_t* c_s_, const FilterArgs& f, int64_t m0, bool live)
      : t_s(t_s_), c_s(c_s_), news_time(f.news_time), news_cat(f.news_cat), lo((uint32_t)INT32_MIN), span(~0u),
        mask_lo(~0u), mask_hi(~0u) {
    const int su = threadIdx.x >> 1;
    if (live && f.news_cat) {
      const uint64_t m = f.q_mask[m0 + su];
      mask_lo = (uint32_t)m;
      mask_hi = (uint32_t)(m >> 32);
    }
    if (live && f.news_time) {
      const int32_t a = f.q_lo[m0 + su], b = f.q_hi[m0 + su];
      lo = (uint32_t)a;
      span = (uint32_t)b - (uint32_t)a;
      if (a > b) span = mask_lo = mask_hi = 0;
    }
  }
  __device__ __forceinline__ bool row_ok(int32_t t, uint32_t cat) const {
    return (uint32_t)t - lo <= span && cat < 64 && ((((cat & 32) ? mask_hi : mask_lo) >> (cat & 31)) & 1u) != 0;
  }
  // the attributes of news rows [n0, n0 + TS), clamped past the table as the row loads are
  // (those rows' scores are -inf already).  Called by every thread, before ScoreTile::scores:
  // its barriers order these stores before the reads below, the tile's closing barrier orders
  // the reads before the next tile's stores.
  __device__ __forceinline__ void stage(int64_t n0, int64_t N) {
    const int t = threadIdx.x;
    if (t < TS) {
      const int64_t r = min(n0 + t, N - 1);
      t_s[t + (t >> 6) * (ATTR_HALF - TS / 2)] = news_time ? news_time[r] : 0;
      reinterpret_cast<uint8_t*>(c_s)[t] = news_cat ? news_cat[r] : (uint8_t)0;
    }
  }
  // bit i of (elo | ehi << 32): tile row 64 sh + i is inside the user's window and mask
  __device__ __forceinline__ void rows64(int sh, uint32_t& elo, uint32_t& ehi) const {
    const int32_t* t = t_s + ATTR_HALF * sh;
    const uint32_t* c = c_s + (TS / 8) * sh;
    elo = ehi = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int4 tv = *reinterpret_cast<const int4*>(t + 4 * i);
      const uint32_t cw = c[i];
      const uint32_t b = (row_ok(tv.x, cw & 255u) ? 1u : 0u) | (row_ok(tv.y, (cw >> 8) & 255u) ? 2u : 0u) |
                         (row_ok(tv.z, (cw >> 16) & 255u) ? 4u : 0u) | (row_ok(tv.w, cw >> 24) ? 8u : 0u);
      if (i < 8) elo |= b << (4 * i);
      else ehi |= b << (4 * (i - 8));
    }
  }
  // Top-K's scan: clear the bits of (mlo | mhi << 32) -- the rows of this thread's half that beat
  // the running K-th best -- whose rows are not eligible.  Once K rows are kept few rows pass
  // the scan (K (1 + ln(rows / K)) over a whole walk), so only they are tested, one at a time;
  // while a thread of the wave still has many (the list is filling: every finite score passes),
  // all 64 rows are.  Both ways apply the same test.  Called by every thread.
  __device__ __forceinline__ void keep_eligible(int sh, uint32_t& mlo, uint32_t& mhi) const {
    if (__any(__popc(mlo) + __popc(mhi) > SPARSE_MAX)) {
      uint32_t elo, ehi;
      rows64(sh, elo, ehi);
      mlo &= elo;
      mhi &= ehi;
      return;
    }
    const int32_t* t = t_s + ATTR_HALF * sh;
    const uint8_t* c = reinterpret_cast<const uint8_t*>(c_s) + (TS / 2) * sh;
    for (uint32_t b = mlo; b; b &= b - 1) {
      const int i = __builtin_ctz(b);
      if (!row_ok(t[i], c[i])) mlo &= ~(1u << i);
    }
    for (uint32_t b = mhi; b; b &= b - 1) {
      const int i = __builtin_ctz(b);
      if (!row_ok(t[32 + i], c[32 + i])) mhi &= ~(1u << i);
    }
  }
};

// what the unfiltered instantiations construct in its place: nothing
struct NoFilter {
  __device__ __forceinline__ NoFilter(int32_t*, uint32_t*, const FilterArgs&, int64_t, bool) {}
};
template <bool FILT> using FilterOf = std::conditional_t<FILT, Eligible, NoFilter>;

// One workgroup's walk over news rows [c0, min(N, c0 + span_rows)) of the table against users
// [m0, m0 + TS).  The kernel declares the __shared__ arrays and hands them in; run() calls
// epilogue(n0, T) once per finished score tile T of rows [n0, n0 + TS) and closes the tile with
// the barrier behind which the next tile's operands overwrite T.  Threads 2 su and 2 su + 1
// (sh = 0, 1) serve user su of the block, which exists if `live`.  PRIOR: T holds selection
// keys; the block's scaled gains are staged once, a tile's priors where its cand_inv is.
template <typename TI, bool FILT, bool PRIOR = false>
struct ChunkWalk {
  int64_t U, N, m0, c0, ldt;
  int ntiles, su, sh;
  bool live;
  const TI* tab;
  const float* cinv;
  PriorArgs pri;
  ScoreTile<TI, PRIOR> st;
  Excluded ex;
  FilterOf<FILT> el;

  __device__ __forceinline__ ChunkWalk(uint32_t* smem, float* cinv_s, uint16_t* ex_s, uint32_t* ov_mask, int32_t* ft_s,
                                       uint32_t* fc_s, int64_t U_, int64_t N_, const TI* users, const TI* tab_,
                                       int64_t ldt_, const float* cinv_, const int32_t* excl_idx,
                                       const int64_t* excl_off, const FilterArgs& flt, int64_t span_rows,
                                       float* prior_s = nullptr, float* gsel_s = nullptr, PriorArgs pri_ = {})
      : U(U_), N(N_), m0((int64_t)blockIdx.x * TS), c0((int64_t)blockIdx.y * span_rows), ldt(ldt_),
        ntiles((int)((min(N_, c0 + span_rows) - c0 + TS - 1) / TS)), su(threadIdx.x >> 1), sh(threadIdx.x & 1),
        live(m0 + su < U_), tab(tab_), cinv(cinv_), pri(pri_), st(smem, cinv_s, users, m0, U_, prior_s, gsel_s),
        ex(ex_s, ov_mask, excl_idx, excl_off, m0, live, c0), el(ft_s, fc_s, flt, m0, live) {}

  template <typename Epilogue>
  __device__ __forceinline__ void run(Epilogue epilogue) {
    const int tid = threadIdx.x;
    // a run of consecutive table rows from n0, clamped past the table (their scores are -inf)
    auto rows_from = [&](int64_t n0) __attribute__((always_inline)) {
      return [n0, last = N - 1](int r) __attribute__((always_inline)) { return min(n0 + r, last); };
    };
    st.gload(tab, ldt, rows_from(c0), 0);
    if constexpr (PRIOR) {  // (read behind the first tile's barriers)
      if (tid < TS) st.gsel_s[tid] = m0 + tid < U ? pri.gsel[m0 + tid] : 0.f;
    }
    for (int tile = 0; tile < ntiles; ++tile) {
      const int64_t n0 = c0 + (int64_t)tile * TS;
      if (tile == 0 || n0 == ex.cb + kChunk) ex.chunk_start(n0);
      const int nvalid = (int)min((int64_t)TS, N - n0);
      if (tid < TS) st.cinv_s[tid] = tid < nvalid ? cinv[n0 + tid] : 0.f;
      if constexpr (PRIOR) {
        if (tid < TS) st.prior_s[tid] = tid < nvalid ? pri.news_prior[n0 + tid] : 0.f;
      }
      if constexpr (FILT) el.stage(n0, N);
      st.scores(tab, ldt, rows_from(n0), tile + 1 < ntiles, rows_from(n0 + TS), nvalid);
      ex.knock_out_overflow(st.tile(), m0, n0);
      epilogue(n0, st.tile());
      __syncthreads();  // the next tile's operands overwrite the score tile
    }
  }
};

// ---- host side: what the entries over the whole table (nr_topk_users*, nr_rank_targets*) share
struct ScanArgs {
  int dtype;
  int64_t dim, U;
  const float* users;
  int64_t N;
  const void* cand_table;
  int64_t cand_ld;
  const float* cand_inv_norm;
  const int32_t* excl_idx;
  const int64_t* excl_off;
  FilterArgs flt;
  void* stream;
  const float* news_prior = nullptr;  // the rank-one prior (include/newsrec_prior.h): [N] and
  const float* user_gain = nullptr;   //   [U], both or neither
  const float* after_key = nullptr;    // the cursor (include/newsrec_page.h): [U] and [U], both or
  const int32_t* after_row = nullptr;  //   neither; nr_topk_users_after alone sets it
  bool prior() const { return news_prior != nullptr; }
  bool after() const { return after_key != nullptr; }
};

static inline int64_t chunks_of(int64_t N) { return (N + kChunk - 1) / kChunk; }
static inline bool scan_shape_ok(int dtype, int64_t U, int64_t N) {
  return ok_dtype(dtype) && U >= 1 && U < (1ll << 31) && N >= 1 && N <= kChunk * kMaxChunks;
}
static inline int no_check() { return NR_OK; }

// The shared validation.  A feature's own size check (K, T) runs where that feature has always
// had it, behind the dtype check or behind those of N; its output and workspace checks follow.
template <typename AfterDtype, typename AfterN>
static int check_scan(const char* fn, const ScanArgs& a, AfterDtype after_dtype, AfterN after_n) {
  nr::clear_error();
  if (a.dim != 1024) {
    nr::set_error("%s: dim %lld unsupported (1024 only)", fn, (long long)a.dim);
    return NR_ERR_UNSUPPORTED;
  }
  NR_CHECK_ARG(nr::ok_dtype(a.dtype), "%s: bad dtype %d", fn, a.dtype);
  if (const int rc = after_dtype()) return rc;
  NR_CHECK_ARG(a.U >= 1 && a.U < (1ll << 31), "%s: U = %lld outside [1, 2^31)", fn, (long long)a.U);
  NR_CHECK_ARG(a.N >= 1, "%s: N = %lld < 1", fn, (long long)a.N);
  if (a.N > kChunk * kMaxChunks) {
    nr::set_error("%s: N = %lld unsupported (at most %lld rows)", fn, (long long)a.N, (long long)(kChunk * kMaxChunks));
    return NR_ERR_UNSUPPORTED;
  }
  if (const int rc = after_n()) return rc;
  NR_CHECK_ARG(a.cand_ld >= a.dim, "%s: cand_ld = %lld < dim", fn, (long long)a.cand_ld);
  NR_CHECK_ARG(a.cand_ld % (a.dtype == NR_F32 ? 4 : 8) == 0 && ((uintptr_t)a.cand_table & 15) == 0 &&
                   ((uintptr_t)a.users & 15) == 0,
               "%s: users and cand_table must be 16-byte aligned with 16-byte row strides", fn);
  NR_CHECK_ARG((a.excl_idx == nullptr) == (a.excl_off == nullptr), "%s: excl_idx and excl_off go together", fn);
  const FilterArgs& f = a.flt;
  NR_CHECK_ARG((f.news_time == nullptr) == (f.q_lo == nullptr) && (f.news_time == nullptr) == (f.q_hi == nullptr),
               "%s: news_time, q_time_lo and q_time_hi go together", fn);
  NR_CHECK_ARG((f.news_cat == nullptr) == (f.q_mask == nullptr), "%s: news_cat and q_cat_mask go together", fn);
  NR_CHECK_ARG((a.news_prior == nullptr) == (a.user_gain == nullptr), "%s: news_prior and user_gain go together", fn);
  NR_CHECK_ARG(a.users && a.cand_table && a.cand_inv_norm, "%s: null pointer", fn);
  return NR_OK;
}

// NR_CHECK_DEVICE over a scan's pointers, the feature's own (`outs`) between the scan's and the
// filter's; the prior's come last
static inline int check_scan_device(const char* fn, const ScanArgs& a, const char* out_names,
                                    std::initializer_list<const void*> outs) {
  if (const int rc = nr::check_device_ptrs(fn, "users, cand_table, cand_inv_norm, excl_idx, excl_off",
                                           {a.users, a.cand_table, a.cand_inv_norm, a.excl_idx, a.excl_off}))
    return rc;
  if (const int rc = nr::check_device_ptrs(fn, out_names, outs)) return rc;
  if (const int rc = nr::check_device_ptrs(fn, "news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask",
                                           {a.flt.news_time, a.flt.q_lo, a.flt.q_hi, a.flt.news_cat, a.flt.q_mask}))
    return rc;
  return nr::check_device_ptrs(fn, "news_prior, user_gain", {a.news_prior, a.user_gain});
}

// What a scan launches with: the users operand (NR_BF16: converted into `ub`, U * D * 2 bytes of
// the workspace), the grids of user blocks and of (user block, run of chunks).  A workgroup keeps
// one running state over chunk_span consecutive chunks: the longer its walk, the fewer rows ever
// pass top-K's threshold (K (1 + ln(rows / K)) of them).  No result depends on it.
struct ScanLaunch {
  const void* urows;
  dim3 g0, g1;
  int64_t span_rows;  // news rows per workgroup of g1
};
static inline int scan_prepare(const char* fn, const ScanArgs& a, void* ub, ScanLaunch& L, float* gsel = nullptr) {
  // the prior's pre-pass: gsel [a.U] of the workspace
  if (a.prior())
    if (const int rc = prior_gains_launch(a.U, a.users, a.user_gain, gsel, (hipStream_t)a.stream, fn)) return rc;
  const int64_t nchunks = chunks_of(a.N), span = chunk_span(a.U, nchunks);
  L.g0 = dim3((unsigned)((a.U + TS - 1) / TS));
  L.g1 = dim3(L.g0.x, (unsigned)((nchunks + span - 1) / span));
  L.span_rows = span * kChunk;
  L.urows = a.users;
  if (a.dtype == NR_BF16) {
    if (const int rc = bf16_users_launch(a.U, a.users, (__bf16*)ub, (hipStream_t)a.stream, fn)) return rc;
    L.urows = ub;
  }
  return NR_OK;
}

// f(TypeTag<TI>, std::bool_constant<FILT>, std::bool_constant<PRIOR>) for the scan's dtype and
// whether it carries a filter and a prior; an f that takes a fourth tag (topk.hip's stage 1)
// gets std::bool_constant<AFTER> too: whether the scan carries a cursor
template <typename F>
static int with_scan_types(const ScanArgs& a, F&& f) {
  return nr::with_dtype(a.dtype, [&](auto ti) {
    auto with_after = [&](auto filt, auto prior) {
      if constexpr (std::is_invocable_v<F&, decltype(ti), decltype(filt), decltype(prior), std::true_type>)
        return a.after() ? f(ti, filt, prior, std::true_type{}) : f(ti, filt, prior, std::false_type{});
      else
        return f(ti, filt, prior);
    };
    auto with_prior = [&](auto filt) {
      return a.prior() ? with_after(filt, std::true_type{}) : with_after(filt, std::false_type{});
    };
    return a.flt.any() ? with_prior(std::true_type{}) : with_prior(std::false_type{});
  });
}

// ---- what the top-K entries (topk.hip, sections.hip) share behind their stage 1
struct alignas(8) Pair {
  float s;
  int32_t r;
};

// The workspace of a top-K that keeps K (score, row) pairs per user and chunk; with a prior,
// the U scaled gains behind the base layout.
struct TopkLayout {
  int64_t nchunks, ub, cnt, uidx, coff, part, gsel, total;
};
static inline TopkLayout topk_layout(int dtype, int64_t U, int64_t N, int64_t K, bool prior = false) {
  TopkLayout L{};
  L.nchunks = chunks_of(N);
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += align256(bytes);
    return at;
  };
  L.ub = take(dtype == NR_BF16 ? U * D * 2 : 0);
  L.cnt = take(U * 4);
  L.uidx = take(U * 4);
  L.coff = take((U + 1) * 8);
  L.part = take(U * L.nchunks * K * (int64_t)sizeof(Pair));
  L.gsel = take(prior ? U * 4 : 0);
  L.total = o;
  return L;
}

// Stage 2 (topk.hip) over a.U users of S lists each: stage 1 left list (u, s)'s rank-sorted
// runs of k pairs at part[((u S + s) nruns + run) k].  Merge per list, the evaluation path's
// scores of a user's S k survivors, a rank sort per list: top_idx / top_scores [U][S][k].
// cnt ([U] int32) is used when S == 1; with more lists per user a list's length is counted
// from its runs again, so the workspace is topk_layout(dtype, U, N, S k) for every S.
// top_keys (null: none wanted) [U][S][k]: with a prior in `a` the rank sort orders by
// fl(score + fl(gain * prior)) and writes these keys; without one they are the scores.
// next_key / next_row (null: not wanted) [U S]: each list's last survivor in selection order,
// the cursor of include/newsrec_page.h.
int topk_stage2_launch(const char* fn, const ScanArgs& a, int64_t S, int64_t k, int nruns, const Pair* part,
                       int32_t* cnt, int32_t* uidx, int64_t* coff, int32_t* top_idx, float* top_scores,
                       float* top_keys = nullptr, float* next_key = nullptr, int32_t* next_row = nullptr);
// Its steps behind the merge (the re-score and the rank sort), for an entry with a merge of its
// own (caps.hip): that merge has left what topk_merge_kernel leaves in top_idx, cnt, uidx, coff.
int topk_stage2_finish(const char* fn, const ScanArgs& a, int64_t S, int64_t k, int nruns, const Pair* part,
                       int32_t* cnt, int32_t* uidx, int64_t* coff, int32_t* top_idx, float* top_scores,
                       float* top_keys = nullptr);

}  // namespace tk
}  // namespace nr
