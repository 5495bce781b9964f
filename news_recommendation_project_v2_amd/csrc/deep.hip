// Deep retrieval (include/newsrec_deep.h): up to NR_TOPK_DEEP_MAX rows per user from one walk
// over the table.  topk.hip keeps a user's list as a 64-slot heap in LDS; 256 slots for 128
// users do not fit beside the operand ring, so here the list lives in the workspace.
//
//   stage 1  topk.hip's grid, walk, score tile, staging and scan masks (nr_score_tile.h).  The
//            owner thread of a user appends every scan survivor that is not excluded and lies
//            behind the cursor to the (user, run)'s LOG of CAP (key, row) pairs: one 8-byte
//            store, no compare against the list.  thr, the key a row must beat, is -inf until
//            the log is first COMPACTED: a wave reads the log, finds the K-th best pair under
//            better() by bisection over the key's and the row's bits (ballots and popcounts over
//            8 pairs per lane: no LDS, no sort), writes the K best back to the log's head and
//            publishes the K-th key as the new thr.  A tile adds at most TS pairs, so logs are
//            looked at between tiles only: a log with fewer than TS free slots sends the
//            workgroup into a compaction phase, in which the four waves also take every other
//            log SLACK pairs past K.  After the walk every log is cut to its K best once more
//            and rank-sorted in place.
//   stage 2  topk.hip's steps at four pairs per lane: a merge of the runs' sorted heads (a copy
//            when there is one run), the evaluation path's scoring kernel over the survivors,
//            a rank sort of each user's <= 256 (score or key, row) pairs.
//
// Why no result depends on when logs are compacted.  Within a run rows arrive in ascending row
// order.  A compaction keeps the K best of the eligible rows seen so far in the strict total
// order of better() (rows are distinct, so the K-th best is one pair), and thr becomes its key.
// A later row is dropped only if !(key > thr): it ties the K-th on the key at best, and then
// loses on its higher row; K pairs already beat it, so it is in no K best.  What is in the log
// at the end is therefore a superset of the run's K best eligible rows, and the final cut takes
// exactly those, whatever was dropped on the way and whenever.
#include "nr_score_tile.h"

#include "../../include/newsrec_deep.h"

namespace nr {
namespace tk {
namespace deep {

constexpr int KDEEP = NR_TOPK_DEEP_MAX;
constexpr int CAP = 2 * KDEEP;  // pairs per log
constexpr int EPL = CAP / 64;   // pairs per lane of the wave that compacts a log
constexpr int SLACK = 64;       // pairs past K from which a log is compacted along with a full one
static_assert(CAP - TS >= KDEEP + SLACK, "a log with fewer than TS free slots must be worth compacting");
static_assert(CAP - KDEEP >= TS, "a compacted log must take a whole tile");

// f32 -> u32, monotone in the order of the float compares the kernels make (-0 == +0; no NaN
// reaches a log: the scan's `v > thr` refuses it).  0 is below every key: the pad of a lane's
// unused slots.
__device__ __forceinline__ uint32_t ord_of(float s) {
  uint32_t b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_of(uint32_t o) {
  return __uint_as_float((o >> 31) ? o ^ 0x80000000u : ~o);
}

// The K-th best of a wave's pairs (EPL per lane: ord_of(key) in o, 0 for an unused slot, row in
// r; more than K of them used), as the cut (T, R): a pair is among the K best iff kept(o, r).
// Every lane of the wave calls it; every lane gets the same cut.
struct Cut {
  uint32_t T;  // ord_of the K-th best key
  int32_t R;   // the highest row kept at that key
  __device__ __forceinline__ bool kept(uint32_t o, int32_t r) const { return o > T || (o == T && r <= R); }
};
__device__ __forceinline__ Cut select_cut(const uint32_t (&o)[EPL], const int32_t (&r)[EPL], int K) {
  auto count = [&](auto pred) __attribute__((always_inline)) {
    int c = 0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) c += __popcll(__ballot(pred(e)));
    return c;
  };
  // the largest T with at least K keys >= T: the K-th largest key
  uint32_t T = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t c = T | (1u << b);
    if (count([&](int e) { return o[e] >= c; }) >= K) T = c;
  }
  // m of the pairs at T are kept, those of the lowest rows: R is the m-th lowest
  const int m = K - count([&](int e) { return o[e] > T; });
  int32_t R = INT32_MAX;
  if (count([&](int e) { return o[e] == T; }) > m) {
    R = 0;  // the largest R with fewer than m rows below it
    for (int b = 30; b >= 0; --b) {
      const int32_t c = R | (1 << b);
      if (count([&](int e) { return o[e] == T && r[e] < c; }) < m) R = c;
    }
  }
  return Cut{T, R};
}

// A wave's view of one log of n <= CAP pairs: slot lane + 64 e in element e.
struct LogRegs {
  float s[EPL];
  uint32_t o[EPL];
  int32_t r[EPL];
  __device__ __forceinline__ void load(const Pair* lg, int n, int lane) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int i = lane + 64 * e;
      const Pair p = i < n ? lg[i] : Pair{0.f, INT32_MAX};
      s[e] = p.s;
      r[e] = p.r;
      o[e] = i < n ? ord_of(p.s) : 0u;
    }
  }
  // the kept pairs (at most lim: dst's size) to dst[0 .. ), lane-major (any fixed order does: the
  // final cut sorts)
  template <typename Keep>
  __device__ __forceinline__ void pack(Pair* dst, int lim, int lane, Keep keep) const {
    int c = 0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) c += keep(e) ? 1 : 0;
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    int pos = inc - c;
#pragma unroll
    for (int e = 0; e < EPL; ++e)
      if (keep(e) && pos < lim) dst[pos++] = Pair{s[e], r[e]};
  }
};

// FILT, PRIOR, AFTER: as in topk_stage1_kernel (topk.hip), mask for mask.
template <typename TI, bool FILT, bool PRIOR, bool AFTER>
__global__ __launch_bounds__(256) void deep_stage1_kernel(int64_t U, int64_t N, const TI* __restrict__ users,
                                                          const TI* __restrict__ tab, int64_t ldt,
                                                          const float* __restrict__ cinv,
                                                          const int32_t* __restrict__ excl_idx,
                                                          const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                          int K, int64_t span_rows, Pair* logs, PriorArgs pri,
                                                          AfterArgs aft) {
  __shared__ __attribute__((aligned(16))) uint32_t smem[4 * TILE_WORDS];  // ring [2][news | users]; score tile
  __shared__ __attribute__((aligned(16))) float cinv_s[TS];
  __shared__ int cnt_s[TS];    // the logs' lengths, owner -> compacting wave -> owner
  __shared__ float thr_s[TS];  // the users' thresholds, compacting wave -> both threads of the user
  __shared__ Pair sort_s[4][KDEEP];  // the final cut: a wave's kept pairs
  __shared__ uint16_t ex_s[XCAP * TS];
  __shared__ uint32_t ov_mask[TS / 32];
  __shared__ __attribute__((aligned(16))) int32_t ft_s[FILT ? ATTR_TIME_WORDS : 4];
  __shared__ uint32_t fc_s[FILT ? ATTR_CAT_WORDS : 1];
  __shared__ __attribute__((aligned(16))) float prior_s[PRIOR ? TS : 4];
  __shared__ float gsel_s[PRIOR ? TS : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NINF = -__builtin_inff();
  ChunkWalk<TI, FILT, PRIOR> w(smem, cinv_s, ex_s, ov_mask, ft_s, fc_s, U, N, users, tab, ldt, cinv, excl_idx,
                               excl_off, flt, span_rows, prior_s, gsel_s, pri);
  // threads 2u and 2u + 1 serve user u of the block; 2u owns its log
  const int su = w.su, sh = w.sh;
  const int64_t m0 = w.m0;
  // log of (user m0 + u, this run); only users below U have one
  auto log_of = [&](int u) __attribute__((always_inline)) {
    return logs + ((m0 + u) * gridDim.y + blockIdx.y) * CAP;
  };
  Pair* const mine = log_of(su);
  int cnt = 0;       // pairs in the log
  float thr = NINF;  // the K-th best key at the log's latest compaction; -inf before the first
  float cur_key = __builtin_inff();
  int32_t cur_row = -1;
  if constexpr (AFTER) {
    if (w.live) {
      cur_key = aft.key[m0 + su];
      cur_row = aft.row[m0 + su];
    }
  }
  if (sh == 0) thr_s[su] = NINF;  // (read behind a compaction phase's barriers)

  w.run([&](int64_t n0, float* T) __attribute__((always_inline)) {
    // ---- the scan of topk_stage1_kernel
    uint32_t mlo = 0, mhi = 0;
    {
      const float* row = T + su * TLD + 64 * sh;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
        uint32_t b = (v.x > thr ? 1u : 0u) | (v.y > thr ? 2u : 0u) | (v.z > thr ? 4u : 0u) | (v.w > thr ? 8u : 0u);
        if constexpr (AFTER)  // (a NaN cursor passes nothing)
          b &= (v.x <= cur_key ? 1u : 0u) | (v.y <= cur_key ? 2u : 0u) | (v.z <= cur_key ? 4u : 0u) |
               (v.w <= cur_key ? 8u : 0u);
        if (i < 8) mlo |= b << (4 * i);
        else mhi |= b << (4 * (i - 8));
      }
    }
    if constexpr (FILT) w.el.keep_eligible(sh, mlo, mhi);
    const uint32_t plo = __shfl_down(mlo, 1, 64), phi = __shfl_down(mhi, 1, 64);
    if (sh == 0 && w.live) {
      // at most TS appends, and the log had TS free slots when the tile began
      auto drain = [&](uint32_t bits, int col0) __attribute__((always_inline)) {
        while (bits) {
          const int col = col0 + __builtin_ctz(bits);
          bits &= bits - 1;
          const float s = T[su * TLD + col];
          const int32_t row = (int32_t)(n0 + col);
          if (w.ex.staged(row)) continue;
          if constexpr (AFTER) {
            if (s == cur_key && row <= cur_row) continue;  // at the cursor's key: only the rows behind its row
          }
          if (cnt < CAP) mine[cnt++] = Pair{s, row};
        }
      };
      drain(mlo, 0);
      drain(mhi, 32);
      drain(plo, 64);
      drain(phi, 96);
    }
    // ---- between tiles: does a log of this block lack room for the next tile?
    if (sh == 0) cnt_s[su] = cnt;
    // The hand-off.  A log is appended to by its owner's wave and read, cut and rewritten by
    // wave u & 3.  __syncthreads() is a workgroup-scope release and acquire around the barrier:
    // every wave waits for its outstanding vector stores (vmcnt) before it arrives, so the
    // appends have left the wave when the reader starts; the waves of a workgroup share the
    // compute unit's write-through vector L1, where a load behind the barrier finds what a store
    // ahead of it wrote -- workgroup scope needs no cache invalidate on this target.  The
    // same holds for the way back (the rewritten head is only read at a later compaction) and
    // for cnt_s / thr_s in LDS.  No other workgroup touches these logs.
    if (__syncthreads_or(sh == 0 && cnt > CAP - TS)) {
      for (int u = wave; u < TS; u += 4) {
        const int n = cnt_s[u];       // wave-uniform
        if (n < K + SLACK) continue;  // (a user past U has 0)
        Pair* lg = log_of(u);
        LogRegs e;
        e.load(lg, n, lane);
        const Cut cut = select_cut(e.o, e.r, K);  // n > K
        // (every lane's loads were consumed by the ballots above: the head is rewritten in place)
        e.pack(lg, K, lane, [&](int i) { return cut.kept(e.o[i], e.r[i]); });
        if (lane == 0) {
          cnt_s[u] = K;
          thr_s[u] = key_of(cut.T);
        }
      }
      __syncthreads();
      if (sh == 0) cnt = cnt_s[su];
      thr = thr_s[su];
    }
  });

  // ---- the final cut: min(count, K) pairs per log, best first at its head, then (-inf, -1) up to K.
  // Every wave makes TS / 4 rounds, users past U included (with nothing), for the barriers.
  if (sh == 0) cnt_s[su] = cnt;
  __syncthreads();
  for (int u = wave; u < TS; u += 4) {
    const bool have = m0 + u < U;  // wave-uniform
    const int n = have ? cnt_s[u] : 0;
    Pair* lg = log_of(u);
    LogRegs e;
    e.load(lg, n, lane);
    if (n > K) {
      const Cut cut = select_cut(e.o, e.r, K);
      e.pack(sort_s[wave], K, lane, [&](int i) { return cut.kept(e.o[i], e.r[i]); });
    } else {
      e.pack(sort_s[wave], K, lane, [&](int i) { return lane + 64 * i < n; });
    }
    __syncthreads();
    const int nk = min(n, K);
    Pair p[KDEEP / 64];
    int rank[KDEEP / 64];
#pragma unroll
    for (int q = 0; q < KDEEP / 64; ++q) {
      const int j = lane + 64 * q;
      p[q] = j < nk ? sort_s[wave][j] : Pair{NINF, INT32_MAX};
      rank[q] = 0;
    }
    for (int t = 0; t < nk; ++t) {
      const Pair x = sort_s[wave][t];
#pragma unroll
      for (int q = 0; q < KDEEP / 64; ++q) rank[q] += better(x.s, x.r, p[q].s, p[q].r) ? 1 : 0;
    }
    if (have) {
#pragma unroll
      for (int q = 0; q < KDEEP / 64; ++q) {
        const int j = lane + 64 * q;
        if (j < nk) lg[rank[q]] = p[q];
        else if (j < K) lg[j] = Pair{NINF, -1};
      }
    }
    __syncthreads();  // sort_s is the next round's
  }
}

// One wave per user: K rounds over the heads of its runs' sorted lists (topk_merge_kernel with
// the winner stored as it is found); with one run the list is copied.  top_idx gets the
// survivors' rows, 0 in place of a missing one (never row -1 to the scoring gather), cnt_out
// their number; uidx / coff are the re-score's user index and offsets; next_key / next_row
// (null: not wanted) the K-th survivor, or the end cursor when fewer than K survived.
__global__ __launch_bounds__(256) void deep_merge_kernel(int64_t U, int K, int nruns, const Pair* __restrict__ logs,
                                                         int32_t* __restrict__ top_idx, int32_t* __restrict__ cnt_out,
                                                         int32_t* __restrict__ uidx, int64_t* __restrict__ coff,
                                                         float* __restrict__ next_key, int32_t* __restrict__ next_row) {
  __shared__ uint16_t head[4][kMaxChunks];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= U) return;  // wave-uniform; no block-wide barrier below
  const Pair* p = logs + u * nruns * CAP;
  const float NINF = -__builtin_inff();
  int cnt = 0;
  float last_s = NINF;
  int32_t last_r = INT32_MAX;
  if (nruns == 1) {
    for (int j = lane; j < K; j += 64) {
      const Pair e = p[j];
      top_idx[u * K + j] = e.r >= 0 ? e.r : 0;
      cnt += e.r >= 0 ? 1 : 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if (cnt == K) {
      last_s = p[K - 1].s;
      last_r = p[K - 1].r;
    }
  } else {
    for (int c = lane; c < nruns; c += 64) head[wave][c] = 0;
    float bs;
    int32_t br;
    int bc;
    auto refresh = [&]() {
      bs = NINF;
      br = INT32_MAX;
      bc = -1;
      for (int c = lane; c < nruns; c += 64) {
        const int h = head[wave][c];
        if (h >= K) continue;
        const Pair e = p[(int64_t)c * CAP + h];
        if (e.r >= 0 && better(e.s, e.r, bs, br)) {
          bs = e.s;
          br = e.r;
          bc = c;
        }
      }
    };
    refresh();
    for (int j = 0; j < K; ++j) {
      float ws = bs;
      int32_t wr = br;
      int wl = lane;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float os = __shfl_xor(ws, m, 64);
        const int32_t orow = __shfl_xor(wr, m, 64);
        const int ol = __shfl_xor(wl, m, 64);
        // rows are distinct across runs; two exhausted lanes (row INT32_MAX) tie and either may stand
        if (better(os, orow, ws, wr)) {
          ws = os;
          wr = orow;
          wl = ol;
        }
      }
      wl = __shfl(wl, 0, 64);
      wr = __shfl(wr, 0, 64);
      ws = __shfl(ws, 0, 64);
      if (wr == INT32_MAX) break;  // every list is exhausted
      if (lane == 0) top_idx[u * K + j] = wr;
      last_s = ws;
      last_r = wr;
      ++cnt;
      if (lane == wl) {
        head[wave][bc] += 1;
        refresh();
      }
    }
    for (int j = cnt + lane; j < K; j += 64) top_idx[u * K + j] = 0;
  }
  if (lane == 0) {
    cnt_out[u] = cnt;
    if (next_key) {
      next_key[u] = cnt == K ? last_s : NINF;
      next_row[u] = cnt == K ? last_r : INT32_MAX;
    }
    uidx[u] = (int32_t)u;
    coff[u] = u * K;
    if (u == U - 1) coff[U] = U * K;
  }
}

// One wave per user: order its n <= K <= 256 (evaluation score, row) pairs, four per lane, and
// pad the tail with (-1, -inf, -inf): topk_sort_kernel's result.  PRIOR: the order is by the key
// fl(score + fl(gain[user] * prior[row])), written to top_keys (null: not wanted).
template <bool PRIOR>
__global__ __launch_bounds__(256) void deep_sort_kernel(int64_t U, int K, const int32_t* __restrict__ cnt_in,
                                                        int32_t* __restrict__ top_idx, float* __restrict__ top_scores,
                                                        const float* __restrict__ news_prior,
                                                        const float* __restrict__ user_gain,
                                                        float* __restrict__ top_keys) {
  __shared__ Pair key_s[4][KDEEP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  const bool have = u < U;  // (no early return: block-wide barriers below)
  const int n = have ? cnt_in[u] : 0;
  const float NINF = -__builtin_inff();
  float s[KDEEP / 64], key[KDEEP / 64];
  int32_t r[KDEEP / 64];
  int rank[KDEEP / 64];
#pragma unroll
  for (int q = 0; q < KDEEP / 64; ++q) {
    const int j = lane + 64 * q;
    const bool valid = j < n;
    s[q] = valid ? top_scores[u * K + j] : NINF;
    r[q] = valid ? top_idx[u * K + j] : INT32_MAX;
    key[q] = s[q];
    if constexpr (PRIOR) {
      if (valid) key[q] = add_rn(s[q], mul_rn(user_gain[u], news_prior[r[q]]));
    }
    if (valid) key_s[wave][j] = Pair{key[q], r[q]};
    rank[q] = 0;
  }
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    const Pair x = key_s[wave][t];
#pragma unroll
    for (int q = 0; q < KDEEP / 64; ++q) rank[q] += better(x.s, x.r, key[q], r[q]) ? 1 : 0;
  }
  // (every lane's loads are behind the barrier: the row is rewritten in place)
  if (!have) return;
#pragma unroll
  for (int q = 0; q < KDEEP / 64; ++q) {
    const int j = lane + 64 * q;
    if (j >= K) continue;
    const int at = j < n ? rank[q] : j;
    top_idx[u * K + at] = j < n ? r[q] : -1;
    top_scores[u * K + at] = s[q];
    if constexpr (PRIOR) {
      if (top_keys) top_keys[u * K + at] = key[q];
    }
  }
}

// The workspace behind K > NR_TOPK_MAX (include/newsrec_deep.h states the formula).
struct DeepLayout {
  int64_t nruns, ub, cnt, uidx, coff, logs, gsel, total;
};
static inline DeepLayout deep_layout(int dtype, int64_t U, int64_t N) {
  DeepLayout L{};
  const int64_t nchunks = chunks_of(N), span = chunk_span(U, nchunks);
  L.nruns = (nchunks + span - 1) / span;
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
  L.logs = take(U * L.nruns * CAP * (int64_t)sizeof(Pair));
  L.gsel = take(U * 4);
  L.total = o;
  return L;
}

}  // namespace deep
}  // namespace tk
}  // namespace nr

extern "C" int64_t nr_topk_users_deep_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K) {
  if (!nr::tk::scan_shape_ok(dtype, U, N) || K < 1 || K > nr::tk::deep::KDEEP) return -1;
  if (K <= NR_TOPK_MAX) return nr_topk_users_after_workspace_bytes(dtype, U, N, K);
  return nr::tk::deep::deep_layout(dtype, U, N).total;
}

extern "C" int nr_topk_users_deep(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                  const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                  const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                  const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                  const uint64_t* q_cat_mask, const float* news_prior, const float* user_gain,
                                  const float* after_key, const int32_t* after_row, float* next_key,
                                  int32_t* next_row, int64_t K, int32_t* top_idx, float* top_scores, float* top_keys,
                                  void* ws, int64_t ws_bytes, void* stream) {
  using namespace nr::tk;
  using namespace nr::tk::deep;
  const char* fn = "nr_topk_users_deep";
  const ScanArgs a{dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                   {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream, news_prior, user_gain,
                   after_key, after_row};
  // nr_topk_users_after's checks, in its order
  auto k_ok = [&] {
    NR_CHECK_ARG(K >= 1 && K <= KDEEP, "%s: K = %lld outside [1, %d]", fn, (long long)K, KDEEP);
    return NR_OK;
  };
  if (const int rc = check_scan(fn, a, k_ok, no_check)) return rc;
  NR_CHECK_ARG((after_key == nullptr) == (after_row == nullptr), "%s: after_key and after_row go together", fn);
  NR_CHECK_ARG((next_key == nullptr) == (next_row == nullptr), "%s: next_key and next_row go together", fn);
  NR_CHECK_ARG(top_idx && top_scores && ws, "%s: null pointer", fn);
  const int64_t need = nr_topk_users_deep_workspace_bytes(dtype, U, N, K);
  NR_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes, (long long)need);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  if (const int rc = check_scan_device(fn, a, "top_idx, top_scores, top_keys, ws", {top_idx, top_scores, top_keys, ws}))
    return rc;
  if (const int rc = nr::check_device_ptrs(fn, "after_key, after_row, next_key, next_row",
                                           {after_key, after_row, next_key, next_row}))
    return rc;
  if (K <= NR_TOPK_MAX)
    return nr_topk_users_after(dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                               news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask, news_prior, user_gain, after_key,
                               after_row, next_key, next_row, K, top_idx, top_scores, top_keys, ws, ws_bytes, stream);

  hipStream_t st = (hipStream_t)stream;
  const DeepLayout L = deep_layout(dtype, U, N);
  char* w = (char*)ws;
  int32_t* cnt = (int32_t*)(w + L.cnt);
  int32_t* uidx = (int32_t*)(w + L.uidx);
  int64_t* coff = (int64_t*)(w + L.coff);
  Pair* logs = (Pair*)(w + L.logs);
  float* gsel = (float*)(w + L.gsel);
  ScanLaunch sl;
  if (const int rc = scan_prepare(fn, a, w + L.ub, sl, gsel)) return rc;
  if ((int64_t)sl.g1.y != L.nruns) {
    nr::set_error("%s: internal: %lld runs launched against %lld laid out", fn, (long long)sl.g1.y, (long long)L.nruns);
    return NR_ERR_INVALID;
  }
  const int rc1 = with_scan_types(a, [&](auto ti, auto filt, auto prior, auto after) {
    using TI = typename decltype(ti)::type;
    hipLaunchKernelGGL(
        (deep_stage1_kernel<TI, decltype(filt)::value, decltype(prior)::value, decltype(after)::value>), sl.g1,
        dim3(256), 0, st, U, N, (const TI*)sl.urows, (const TI*)cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
        a.flt, (int)K, sl.span_rows, logs, PriorArgs{news_prior, gsel}, AfterArgs{after_key, after_row});
    return NR_OK;
  });
  if (rc1) return rc1;
  NR_CHECK_LAUNCH(fn);
  const dim3 gw((unsigned)((U + 3) / 4));
  hipLaunchKernelGGL(deep_merge_kernel, gw, dim3(256), 0, st, U, (int)K, (int)L.nruns, (const Pair*)logs, top_idx, cnt,
                     uidx, coff, next_key, next_row);
  NR_CHECK_LAUNCH(fn);
  if (const int rc = nr::score_users_dispatch(dtype, users, uidx, cand_table, cand_ld, cand_inv_norm, top_idx, coff, U,
                                              top_scores, st))
    return rc;
  if (a.prior())
    hipLaunchKernelGGL((deep_sort_kernel<true>), gw, dim3(256), 0, st, U, (int)K, (const int32_t*)cnt, top_idx,
                       top_scores, news_prior, user_gain, top_keys);
  else
    hipLaunchKernelGGL((deep_sort_kernel<false>), gw, dim3(256), 0, st, U, (int)K, (const int32_t*)cnt, top_idx,
                       top_scores, news_prior, user_gain, top_keys);
  NR_CHECK_LAUNCH(fn);
  // without a prior the keys are the scores
  if (top_keys && !a.prior() &&
      hipMemcpyAsync(top_keys, top_scores, (size_t)(U * K) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    nr::set_error("%s: hipMemcpyAsync failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return NR_ERR_HIP;
  }
  return NR_OK;
}
