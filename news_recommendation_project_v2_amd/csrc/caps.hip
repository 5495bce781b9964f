// Top-K retrieval under per-group caps (include/newsrec_caps.h): at most `cap` news of one
// group in a user's list, exact, in topk.hip's one pass over the table.
//
//   stage 1  topk.hip's walk (nr_score_tile.h: the same product, exclusion staging, overflow
//            knock-out, filter and prior, so the selection bits are topk.hip's) and its scan of
//            the score tile against the running K-th best.  Only the insertion differs: the
//            owner thread scans its list once for the candidate's group (count, worst member).
//            A group at its cap takes the candidate in place of its worst member, if the
//            candidate beats it, and the heap is repaired from that slot; any other candidate
//            takes topk.hip's path (append, or replace the overall worst).  Rows arrive in
//            ascending row order and thresholds only rise, so a dropped entry never returns and
//            the list is always the capped list of the rows walked so far.
//            The group of a kept row rides in the 10 spare high bits of the list's row word
//            (N <= 2^22), so the lists cost no LDS beyond topk.hip's; every compare and the
//            exclusion lookup see the row alone.  The tile's 128 group ids are staged one tile
//            ahead in a double-buffered 2 x 256 B array, with no barrier of their own.
//   stage 2  a capped merge: one wave per user, the best head of the chunk lists wins a round
//            and is taken unless its group already has `cap` survivors (it is skipped, its list
//            advances), until K are taken or every list is exhausted.  The greedy walk over the
//            union of the per-chunk capped lists is the global capped list.  The partials are
//            topk.hip's (score, row) pairs; the merge reads a head's group from news_group.
//            The re-score and the rank sort are topk.hip's (topk_stage2_finish).
//
// cap >= K never reaches these kernels: the entry hands the call to nr_topk_users_prior /
// nr_topk_users_filtered.
#include "nr_score_tile.h"

#include "../../include/newsrec_caps.h"

namespace nr {
namespace tk {

constexpr int KMAX = NR_TOPK_MAX;
constexpr int GSHIFT = 22;  // list word = row | group << GSHIFT
constexpr uint32_t ROW_MASK = (1u << GSHIFT) - 1;
constexpr uint32_t GROUP_MASK = NR_CAP_GROUPS_MAX - 1;
static_assert(kChunk * kMaxChunks <= (1ll << GSHIFT) && NR_CAP_GROUPS_MAX == (1 << (32 - GSHIFT)),
              "a row and a group share one 32-bit list word");

template <typename TI, bool FILT, bool PRIOR>
__global__ __launch_bounds__(256) void caps_stage1_kernel(int64_t U, int64_t N, const TI* __restrict__ users,
                                                          const TI* __restrict__ tab, int64_t ldt,
                                                          const float* __restrict__ cinv,
                                                          const int32_t* __restrict__ excl_idx,
                                                          const int64_t* __restrict__ excl_off, FilterArgs flt,
                                                          const uint16_t* __restrict__ news_group, int cap, int K,
                                                          int64_t span_rows, Pair* __restrict__ part, PriorArgs pri) {
  __shared__ __attribute__((aligned(16))) uint32_t smem[4 * TILE_WORDS];  // ring [2][news | users]; score tile
  __shared__ float ls[KMAX * TS];     // the users' lists, [slot][user]: keys
  __shared__ uint32_t li[KMAX * TS];  //   and row | group << GSHIFT
  __shared__ __attribute__((aligned(16))) float cinv_s[TS];
  __shared__ int cnt_s[TS];
  __shared__ uint16_t ex_s[XCAP * TS];
  __shared__ uint32_t ov_mask[TS / 32];
  __shared__ __attribute__((aligned(16))) int32_t ft_s[FILT ? ATTR_TIME_WORDS : 4];  // the tile's news times
  __shared__ uint32_t fc_s[FILT ? ATTR_CAT_WORDS : 1];                                //   and categories
  __shared__ __attribute__((aligned(16))) float prior_s[PRIOR ? TS : 4];  // the tile's priors
  __shared__ float gsel_s[PRIOR ? TS : 1];                                //   and the block's scaled gains
  __shared__ uint16_t grp_s[2 * TS];  // the groups of this tile's rows and of the next one's

  const int tid = threadIdx.x, lane = tid & 63;
  const float NINF = -__builtin_inff();
  ChunkWalk<TI, FILT, PRIOR> w(smem, cinv_s, ex_s, ov_mask, ft_s, fc_s, U, N, users, tab, ldt, cinv, excl_idx,
                               excl_off, flt, span_rows, prior_s, gsel_s, pri);
  const int su = w.su, sh = w.sh;
  const int64_t m0 = w.m0;
  int cnt = 0;       // rows kept so far (a heap in LDS, the worst at slot 0)
  float thr = NINF;  // the worst's key once K are kept; -inf until then (every finite key passes)
  // Thread c < TS carries the group of column c of the NEXT tile, loaded one tile ahead (the
  // load lands under that tile's product) and stored into the half of grp_s that the current
  // epilogue does not read: the walk's barriers around a product order the store before the next
  // epilogue's reads, its closing barrier the previous epilogue's reads before the store.
  int par = 0;  // the half that holds the current tile's groups
  uint32_t grp_next = 0;
  if (tid < TS) {
    grp_s[tid] = news_group[min(w.c0 + tid, N - 1)];
    grp_next = news_group[min(w.c0 + TS + tid, N - 1)];
  }

  w.run([&](int64_t n0, float* T) __attribute__((always_inline)) {
    const uint16_t* grp = grp_s + par * TS;
    if (tid < TS) {
      grp_s[(par ^ 1) * TS + tid] = (uint16_t)grp_next;
      grp_next = news_group[min(n0 + 2 * TS + tid, N - 1)];
    }
    par ^= 1;
    // ---- scan against the running K-th best (topk.hip's: the worst member of a group is never
    // below the overall worst, so the test stays necessary for every candidate)
    uint32_t mlo = 0, mhi = 0;
    {
      const float* row = T + su * TLD + 64 * sh;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
        const uint32_t b = (v.x > thr ? 1u : 0u) | (v.y > thr ? 2u : 0u) | (v.z > thr ? 4u : 0u) | (v.w > thr ? 8u : 0u);
        if (i < 8) mlo |= b << (4 * i);
        else mhi |= b << (4 * (i - 8));
      }
    }
    if constexpr (FILT) w.el.keep_eligible(sh, mlo, mhi);
    const uint32_t plo = __shfl_down(mlo, 1, 64), phi = __shfl_down(mhi, 1, 64);
    if (sh == 0 && w.live) {
      // 32 columns of the row at a time, in ascending row order
      auto drain = [&](uint32_t bits, int col0) __attribute__((always_inline)) {
        while (bits) {
          const int col = col0 + __builtin_ctz(bits);
          bits &= bits - 1;
          const float s = T[su * TLD + col];
          const int32_t row = (int32_t)(n0 + col);
          // a later row never beats an equal key already kept, so the compare is strict
          if (!(s > thr) || w.ex.staged(row)) continue;  // (the threshold may have risen since the scan)
          // one pass over the list: how many rows of the candidate's group it holds, and the
          // worst of them
          const uint32_t g = grp[col] & GROUP_MASK;
          int ng = 0, wslot = 0;
          float wkey = 0.f;
          int32_t wrow = 0;
          for (int t = 0; t < cnt; ++t) {
            const uint32_t wd = li[t * TS + su];
            if ((wd >> GSHIFT) != g) continue;
            const float ts = ls[t * TS + su];
            const int32_t tr = (int32_t)(wd & ROW_MASK);
            if (ng == 0 || better(wkey, wrow, ts, tr)) {
              wslot = t;
              wkey = ts;
              wrow = tr;
            }
            ++ng;
          }
          // the list is a binary heap with the WORST kept entry (lowest key, then highest row)
          // at slot 0
          int i;
          if (ng < cap && cnt < K) {  // append, sift up while worse than the parent
            i = cnt++;
            while (i > 0) {
              const int p = (i - 1) >> 1;
              const float ps = ls[p * TS + su];
              const uint32_t pw = li[p * TS + su];
              if (!better(ps, (int32_t)(pw & ROW_MASK), s, row)) break;
              ls[i * TS + su] = ps;
              li[i * TS + su] = pw;
              i = p;
            }
          } else {
            // a group at its cap gives up its worst member, and only to a better row; a full
            // list below the cap its overall worst (the root, which the candidate beats).  The
            // newcomer is better than what it replaces, hence than that slot's parent: it can
            // only move towards the leaves.
            if (ng >= cap && !better(s, row, wkey, wrow)) continue;
            i = ng >= cap ? wslot : 0;
            for (int c = 2 * i + 1; c < cnt; c = 2 * i + 1) {
              float cs = ls[c * TS + su];
              uint32_t cw = li[c * TS + su];
              if (c + 1 < cnt) {
                const float ds = ls[(c + 1) * TS + su];
                const uint32_t dw = li[(c + 1) * TS + su];
                if (better(cs, (int32_t)(cw & ROW_MASK), ds, (int32_t)(dw & ROW_MASK))) {
                  cs = ds;
                  cw = dw;
                  ++c;
                }
              }
              if (!better(s, row, cs, (int32_t)(cw & ROW_MASK))) break;
              ls[i * TS + su] = cs;
              li[i * TS + su] = cw;
              i = c;
            }
          }
          ls[i * TS + su] = s;
          li[i * TS + su] = (uint32_t)row | (g << GSHIFT);
          if (cnt == K) thr = ls[su];
        }
      };
      drain(mlo, 0);
      drain(mhi, 32);
      drain(plo, 64);
      drain(phi, 96);
    }
    thr = __shfl(thr, lane & ~1, 64);
  });
  // ---- K (key, row) pairs per (user, run of chunks), best first (a rank sort of the kept list,
  // the group bits dropped); a short list ends in (-inf, -1): topk.hip's partials
  if (sh == 0) cnt_s[su] = cnt;
  __syncthreads();
  for (int i = tid; i < TS * K; i += 256) {
    const int u = i / K, j = i - u * K;
    if (m0 + u >= U) break;
    const int n = cnt_s[u];
    Pair pr{NINF, -1};
    int at = j;
    if (j < n) {
      pr.s = ls[j * TS + u];
      pr.r = (int32_t)(li[j * TS + u] & ROW_MASK);
      at = 0;
      for (int t = 0; t < n; ++t)
        at += better(ls[t * TS + u], (int32_t)(li[t * TS + u] & ROW_MASK), pr.s, pr.r) ? 1 : 0;
    }
    part[((m0 + u) * gridDim.y + blockIdx.y) * K + at] = pr;
  }
}

// topk_merge_kernel (topk.hip) under the caps: one wave per user over the heads of its chunk
// lists (each sorted, each a capped list of its own rows).  Lane l keeps the best head among
// chunks l, l + 64, ... with that row's group, and re-reads them only after it won; lane j < cnt
// holds survivor j and its group.  A round's winner is taken unless `cap` survivors share its
// group; either way its list advances.  At most nchunks K rounds.
__global__ __launch_bounds__(256) void caps_merge_kernel(int64_t U, int K, int cap, int nchunks,
                                                         const Pair* __restrict__ part,
                                                         const uint16_t* __restrict__ news_group,
                                                         int32_t* __restrict__ top_idx, int32_t* __restrict__ cnt_out,
                                                         int32_t* __restrict__ uidx, int64_t* __restrict__ coff) {
  __shared__ uint8_t head[4][kMaxChunks];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= U) return;  // wave-uniform; no block-wide barrier below
  const Pair* p = part + u * nchunks * K;
  for (int c = lane; c < nchunks; c += 64) head[wave][c] = 0;
  const float NINF = -__builtin_inff();
  float bs;
  int32_t br;
  int bc;
  uint32_t bg = 0;
  auto refresh = [&]() {
    bs = NINF;
    br = INT32_MAX;
    bc = -1;
    for (int c = lane; c < nchunks; c += 64) {
      const int h = head[wave][c];
      if (h >= K) continue;
      const Pair e = p[(int64_t)c * K + h];
      if (e.r >= 0 && better(e.s, e.r, bs, br)) {
        bs = e.s;
        br = e.r;
        bc = c;
      }
    }
    if (bc >= 0) bg = news_group[br] & GROUP_MASK;
  };
  refresh();
  int32_t mine = 0;     // lane j: the j-th survivor
  uint32_t mine_g = 0;  //   and its group
  int cnt = 0;
  while (cnt < K) {
    float ws = bs;
    int32_t wr = br;
    int wl = lane;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float os = __shfl_xor(ws, m, 64);
      const int32_t orow = __shfl_xor(wr, m, 64);
      const int ol = __shfl_xor(wl, m, 64);
      // rows are distinct across chunks, so (key, row) alone orders every live head; two
      // exhausted lanes (row INT32_MAX) tie and either may stand
      if (better(os, orow, ws, wr)) {
        ws = os;
        wr = orow;
        wl = ol;
      }
    }
    wl = __shfl(wl, 0, 64);
    wr = __shfl(wr, 0, 64);
    if (wr == INT32_MAX) break;  // every list is exhausted
    const uint32_t g = __shfl(bg, wl, 64);
    const int held = __popcll(__ballot(lane < cnt && mine_g == g));
    if (held < cap) {  // wave-uniform
      if (lane == cnt) {
        mine = wr;
        mine_g = g;
      }
      ++cnt;
    }
    if (lane == wl) {
      head[wave][bc] += 1;
      refresh();
    }
  }
  if (lane < K) top_idx[u * K + lane] = lane < cnt ? mine : 0;  // never row -1 to the scoring gather
  if (lane == 0) {
    cnt_out[u] = cnt;
    uidx[u] = (int32_t)u;
    coff[u] = u * K;
    if (u == U - 1) coff[U] = U * K;
  }
}

}  // namespace tk
}  // namespace nr

extern "C" int64_t nr_topk_users_capped_workspace_bytes(int dtype, int64_t U, int64_t N, int64_t K) {
  return nr_topk_users_prior_workspace_bytes(dtype, U, N, K);
}

extern "C" int nr_topk_users_capped(int dtype, int64_t dim, int64_t U, const float* users, int64_t N,
                                    const void* cand_table, int64_t cand_ld, const float* cand_inv_norm,
                                    const int32_t* excl_idx, const int64_t* excl_off, const int32_t* news_time,
                                    const int32_t* q_time_lo, const int32_t* q_time_hi, const uint8_t* news_cat,
                                    const uint64_t* q_cat_mask, const float* news_prior, const float* user_gain,
                                    const uint16_t* news_group, int64_t cap, int64_t K, int32_t* top_idx,
                                    float* top_scores, float* top_keys, void* ws, int64_t ws_bytes, void* stream) {
  using namespace nr::tk;
  const char* fn = "nr_topk_users_capped";
  const ScanArgs a{dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                   {news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask}, stream, news_prior, user_gain};
  auto k_ok = [&] {
    NR_CHECK_ARG(K >= 1 && K <= KMAX, "%s: K = %lld outside [1, %d]", fn, (long long)K, KMAX);
    return NR_OK;
  };
  if (const int rc = check_scan(fn, a, k_ok, no_check)) return rc;
  NR_CHECK_ARG(cap >= 1 && cap <= KMAX, "%s: cap = %lld outside [1, %d]", fn, (long long)cap, KMAX);
  NR_CHECK_ARG(news_group != nullptr, "%s: news_group is required", fn);
  NR_CHECK_ARG(top_idx && top_scores && ws && (top_keys || !a.prior()), "%s: null pointer", fn);
  const TopkLayout L = topk_layout(dtype, U, N, K, true);
  NR_CHECK_ARG(ws_bytes >= L.total, "%s: workspace too small (%lld < %lld)", fn, (long long)ws_bytes,
               (long long)L.total);
  NR_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
  if (const int rc = check_scan_device(fn, a, "news_group, top_idx, top_scores, top_keys, ws",
                                       {news_group, top_idx, top_scores, top_keys, ws}))
    return rc;
  // the rule cannot bind: the base entry, bit for bit by construction (include/newsrec_caps.h)
  if (cap >= K) {
    if (top_keys || a.prior())
      return nr_topk_users_prior(dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                                 news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask, news_prior, user_gain, K,
                                 top_idx, top_scores, top_keys, ws, ws_bytes, stream);
    return nr_topk_users_filtered(dtype, dim, U, users, N, cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                                  news_time, q_time_lo, q_time_hi, news_cat, q_cat_mask, K, top_idx, top_scores, ws,
                                  ws_bytes, stream);
  }

  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  int32_t* cnt = (int32_t*)(w + L.cnt);
  int32_t* uidx = (int32_t*)(w + L.uidx);
  int64_t* coff = (int64_t*)(w + L.coff);
  Pair* part = (Pair*)(w + L.part);
  float* gsel = (float*)(w + L.gsel);
  ScanLaunch sl;
  if (const int rc = scan_prepare(fn, a, w + L.ub, sl, gsel)) return rc;
  const int rc1 = with_scan_types(a, [&](auto ti, auto filt, auto prior) {
    using TI = typename decltype(ti)::type;
    hipLaunchKernelGGL((caps_stage1_kernel<TI, decltype(filt)::value, decltype(prior)::value>), sl.g1, dim3(256), 0, st,
                       U, N, (const TI*)sl.urows, (const TI*)cand_table, cand_ld, cand_inv_norm, excl_idx, excl_off,
                       a.flt, news_group, (int)cap, (int)K, sl.span_rows, part, PriorArgs{news_prior, gsel});
    return NR_OK;
  });
  if (rc1) return rc1;
  NR_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(caps_merge_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, st, U, (int)K, (int)cap,
                     (int)sl.g1.y, part, news_group, top_idx, cnt, uidx, coff);
  NR_CHECK_LAUNCH(fn);
  return topk_stage2_finish(fn, a, 1, K, (int)sl.g1.y, part, cnt, uidx, coff, top_idx, top_scores, top_keys);
}
