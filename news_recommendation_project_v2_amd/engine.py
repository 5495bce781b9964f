"""Device-resident eval engine for the embed -> pool -> score hot path.

Layout in HBM (one GPU):
  cand_table  [N, 1024] news embeddings in the compute dtype (f32 | bf16)
  cand_inv    [N] f32   1 / max(||row||, 1e-8)           (cosine clamp)
  hist_table  FinalAttention: [N, 2, 1024] = (x, exp(w)) rows, 4/8 KiB
              Latent        : [N, 1024] per-item hiddens
  hist_idx/hist_off, cand_idx/cand_off   int32 rows + int64 CSR offsets
  scores      [C] f32, ranks [C] int32, users [I, 1024] f32 (optional)

One ``step`` = the per-news pooler transform over all N news (MFMA GEMM
chain), the candidate inverse norms, and the fused pool+score kernel over all
impressions.  Everything is enqueued on the current stream; nothing syncs.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .data_utils import distinct_segments, lengths_to_offsets

# below this share of impressions that repeat an earlier impression's history,
# the fused pass (which re-gathers a shared history per impression) moves fewer
# bytes than pooling the distinct histories into f32 user rows (+4 KiB written
# and +4 KiB read per user row): break-even ~ 2 x 4 KiB / (33 x 2 KiB) ~ 0.12
DEDUPE_MIN_SHARE = 0.15

# The column-sliced pool+score (ops.pool_score(sliced=...)) gathers the same rows from slice
# images whose L2 share is 1024 / W times today's, and pays for it with f32 user rows and
# per-slice partial dots written and read once, the index arrays re-read per slice and the
# history table's image rebuilt every step.  Measured on bf16 tables (DESIGN.md §3.1,
# profiles/sliced), stage time against today's kernel on the same machine:
#   MIND-large-dev (147 MB table), latent: W = 128 6.82 ms, W = 64 7.08 ms, today 7.17 ms
#   MIND-large-dev, FinalAttention       : W = 128 10.04 ms, W = 64 9.37 ms, today 10.57 ms
#   MIND-small-dev (87 MB table), latent : W = 128 1.375 ms, W = 64 1.47 ms, today 1.405 ms
# W = 64 hits L2 more often (47 % against 34 %; 2.7 % today) but its launches run out of
# instruction issue on 128-byte rows; FinalAttention's image rows are twice as wide, so there
# it wins.  The smaller table's 2 % is within what another impression mix could undo, so the
# rule switches bf16 tables of at least SLICED_MIN_TABLE_BYTES (one [N, 1024] table) and
# leaves everything else -- f32 tables, which were not measured, included -- on today's
# kernel.  A width of 0 turns the path off for that pooler.
SLICED_W = 128        # latent and mean poolers
SLICED_W_FINAL = 64   # FinalAttention
SLICED_MIN_TABLE_BYTES = 128 << 20


def sliced_width(n_news: int, dtype: torch.dtype, want_users: bool, deduped: bool, pooler: str = "latent") -> int:
    """The slice width pool_score runs at (0: today's kernels): ``want_users`` and the
    deduplicated-history path stay on today's kernels, and so does every table under
    SLICED_MIN_TABLE_BYTES, which a single slice image of W columns no longer misses L2 for
    often enough to pay for the extra passes."""
    w = SLICED_W_FINAL if pooler == "final" else SLICED_W
    if not w or want_users or deduped or dtype != torch.bfloat16:
        return 0
    return w if n_news * 1024 * 2 >= SLICED_MIN_TABLE_BYTES else 0


def _may_repeat(hist_idx: np.ndarray, hist_len: np.ndarray) -> bool:
    """Cheap bound before the exact grouping: repeated histories share (length,
    first id, last id), so if fewer than DEDUPE_MIN_SHARE of the impressions
    repeat such a triple, fewer repeat a whole history."""
    off = lengths_to_offsets(hist_len)
    nz = hist_len > 0
    first = np.where(nz, hist_idx[np.minimum(off[:-1], max(len(hist_idx) - 1, 0))] if len(hist_idx) else 0, -1)
    last = np.where(nz, hist_idx[np.maximum(off[1:] - 1, 0)] if len(hist_idx) else 0, -1)
    key = (hist_len.astype(np.int64) << 42) ^ (first.astype(np.int64) + 1 << 21) ^ (last.astype(np.int64) + 1)
    return 1.0 - len(np.unique(key)) / len(hist_len) >= DEDUPE_MIN_SHARE


def _check_segments(idx: np.ndarray, lens: np.ndarray, what: str) -> None:
    """Validate one CSR index set's lengths on the host (I entries): negative
    lengths and a length sum that does not match the index array (the offsets
    would run past it on the device) are refused.  The rows themselves are
    range-checked on the device after the upload (_row_range)."""
    if len(lens) and int(lens.min()) < 0:
        raise ValueError(f"{what} lengths must be >= 0")
    if int(lens.sum()) != len(idx):
        raise ValueError(f"{what} lengths sum to {int(lens.sum())} but {len(idx)} indices were given")


def _row_range(idx: torch.Tensor, what: str) -> int:
    """Largest row of an uploaded index array (-1 if empty); a negative row is
    refused (IndexError, as torch indexing does).  One min/max reduction where
    the array already is (on the device: microseconds for the 26 M MIND-large-dev
    rows that took ~20 ms of host passes) and one small sync."""
    if idx.numel() == 0:
        return -1
    lo, hi = (int(v) for v in torch.aminmax(idx))
    if lo < 0:
        raise IndexError(f"{what} index {lo} is negative (rows are 0-based indices into the news table)")
    return hi


def _upload(x, dev: torch.device, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Host arrays / CPU tensors to the device; a table converts to the compute
    dtype on the device.  torch's own host-to-device copy of pageable memory runs
    at the PCIe DMA rate here (56 GB/s for the MIND-large-dev index arrays,
    tools/pcie_probe.py, profiles/round6/pcie_probe.jsonl), faster than staging
    through a ring of pinned chunks (45 GB/s, measured and removed in round 6):
    the round-5 "14 GB/s" upload was load_impressions' host-side checks and
    offsets, not the copy."""
    t = torch.as_tensor(x)
    t = t.to(dev)
    return (t if dtype is None or t.dtype == dtype else t.to(dtype)).contiguous()


def section_masks(sections) -> list:
    """recommend_sections' ``sections`` as 64-bit masks (Python ints): an item is either a
    mask (an integer: the same 64 bits as a Python int, int64 or uint64) or an iterable of
    category ids 0 .. 63."""
    if isinstance(sections, (str, bytes)) or not hasattr(sections, "__iter__"):
        raise ValueError("sections must be a sequence of category masks or of category-id lists")
    masks = []
    for item in sections:
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            masks.append(int(item) & 0xFFFFFFFFFFFFFFFF)
            continue
        if isinstance(item, (str, bytes)) or not hasattr(item, "__iter__"):
            raise ValueError(f"a section must be a 64-bit mask or an iterable of category ids, got {item!r}")
        m = 0
        for c in item:
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < 64:
                raise ValueError(f"a section's category ids must be integers in 0 .. 63, got {c!r}")
            m |= 1 << int(c)
        masks.append(m)
    return masks


def check_prior(news_prior, n_news: Optional[int]) -> np.ndarray:
    """set_catalogue's ``news_prior`` as contiguous f32 [N]: one finite value per news."""
    a = np.asarray(news_prior)
    if a.ndim != 1 or (n_news is not None and len(a) != n_news):
        raise ValueError("news_prior must have one entry per news" + ("" if n_news is None else f" ({n_news})"))
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("news_prior must be numbers")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError("news_prior must be finite")
    return a


def check_gain(prior_gain, n_imp: int) -> np.ndarray:
    """``prior_gain`` (a scalar or one value per impression) as finite f32 [n_imp]."""
    try:
        g = np.asarray(prior_gain, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("prior_gain must be a number or one number per impression") from None
    if g.ndim > 1 or (g.ndim == 1 and len(g) != n_imp):
        raise ValueError(f"prior_gain must be a scalar or have one value per impression ({n_imp})")
    if not np.isfinite(g).all():
        raise ValueError("prior_gain must be finite")
    return np.ascontiguousarray(np.broadcast_to(g, (n_imp,))) + np.float32(0)  # (-0 and +0 are one gain)


def _no_prior(what: str, prior_gain) -> None:
    if prior_gain is not None:
        raise ValueError(f"{what}: prior_gain cannot be combined with diversify or explain")


def _no_cap(what: str, group_cap) -> None:
    if group_cap is not None:
        raise ValueError(f"{what}: group_cap is recommend's alone (no ranks, sections, MMR or explained lists "
                         "under per-group caps)")


def check_groups(news_group, n_news: Optional[int]) -> np.ndarray:
    """set_catalogue's ``news_group`` as contiguous int16 [N]: one integer label in [0, 1024)
    per news (the 16 bits the kernels read as uint16)."""
    a = news_group.cpu().numpy() if isinstance(news_group, torch.Tensor) else np.asarray(news_group)
    if a.ndim != 1 or (n_news is not None and len(a) != n_news):
        raise ValueError("news_group must have one entry per news" + ("" if n_news is None else f" ({n_news})"))
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("news_group must be integer labels (data_utils.dense_groups makes them)")
    if len(a) and (a.min() < 0 or a.max() >= GROUPS_MAX):
        raise ValueError(f"news_group labels must lie in [0, {GROUPS_MAX})")
    return np.ascontiguousarray(a, dtype=np.int16)


GROUPS_MAX = 1024  # NR_CAP_GROUPS_MAX (include/newsrec_caps.h)
DEEP_MAX = 1024    # _lib.NR_DEEP_MAX: the longest list recommend_deep pages to
PAGE_MAX = 64      # _lib.NR_TOPK_MAX: the rows of one cursor call
WALK_MAX = 256     # _lib.NR_TOPK_DEEP_MAX: the rows of one deep call (one walk over the table)


def _no_cursor(what: str, **given) -> None:
    for name, v in given.items():
        if v is not None and v is not False:
            raise ValueError(f"{what}: {name} is recommend's alone (no cursors for sections, per-group caps, MMR or "
                             "explained lists)")


def check_cursor(after, n_imp: int):
    """recommend's ``after`` as host arrays (key f32 [n_imp], row int32 [n_imp]): the pair a
    previous call returned (device tensors are read back) or host arrays of the same kind."""
    if not isinstance(after, (tuple, list)) or len(after) != 2:
        raise ValueError("after must be the (key, row) pair a previous call returned")
    key, row = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in after)
    if key.shape != (n_imp,) or row.shape != (n_imp,):
        raise ValueError(f"after must hold one (key, row) per impression ({n_imp})")
    if not np.issubdtype(key.dtype, np.floating) or not np.issubdtype(row.dtype, np.integer):
        raise ValueError("after must be (float keys, integer rows)")
    return np.ascontiguousarray(key, dtype=np.float32), np.ascontiguousarray(row, dtype=np.int32)


def check_deep(what: str, k, page, walk=None) -> None:
    """The sizes of a paged list: 1 <= k <= DEEP_MAX rows in cursor calls of 1 <= page <= PAGE_MAX,
    or, with ``walk``, in one-walk calls of 1 <= walk <= WALK_MAX rows (``page`` then left alone)."""
    for name, v, top in (("k", k, DEEP_MAX), ("page", page, PAGE_MAX)) + ((("walk", walk, WALK_MAX),) if walk is not None
                                                                          else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top:
            raise ValueError(f"{what}: {name} = {v!r} must be an integer in 1 .. {top}")
    if walk is not None and page != PAGE_MAX:
        raise ValueError(f"{what}: walk = {walk!r} cannot be combined with page = {page!r} (walk sizes the calls; "
                         "leave page at its default)")


class _Queries:
    """The distinct (history, time window, category mask, prior gain, cursor) tuples of the loaded
    impressions under a catalogue filter, a prior or a cursor: retrieval and ranks run once per
    query."""

    def __init__(self, user: np.ndarray, sel: np.ndarray, lo, hi, mask, dev, gain=None, after=None):
        self.n = len(user)
        self.user_host, self.sel_host = user, sel
        self.user = _upload(user.astype(np.int64), dev)  # the query's pooled user row
        self.sel = _upload(sel.astype(np.int64), dev)    # the impression's query
        self.lo = None if lo is None else _upload(lo, dev)
        self.hi = None if hi is None else _upload(hi, dev)
        self.mask = None if mask is None else _upload(mask, dev)
        self.gain = None if gain is None else _upload(gain, dev)
        self.after = None if after is None else (_upload(after[0], dev), _upload(after[1], dev))


class PoolScoreEngine:
    def __init__(self, model: torch.nn.Module, dtype: torch.dtype = torch.float32,
                 device: Optional[torch.device] = None):
        self.model = model
        self.pooler = model.pooler_kind
        self.dtype = dtype
        self.device = device or next(model.parameters()).device
        self.weights = model.hip_weights(dtype)  # prepared once
        self.cand_table = None
        self.hist_src = None
        self.cand_inv = None
        self.hist_table = None
        self._ws = None
        self._users = None  # f32 [distinct histories, D], reused across steps
        self._cand_image = self._hist_image = self._sliced_ws = None  # the sliced path's buffers, reused
        self._cand_image_of = None
        self.news_time = None  # int32 [N] / uint8 [N] / f32 [N]: set_catalogue
        self.news_cat = None
        self.news_prior = None
        self.news_group = None  # int16 [N]

    # ------------------------------------------------------------ inputs
    def load_news(self, news_embeddings: torch.Tensor, query_news_embeddings: Optional[torch.Tensor] = None):
        """Upload the news table (and optional separate history-side table)."""
        self.cand_table = _upload(news_embeddings, self.device, self.dtype)
        if query_news_embeddings is not None:
            self.hist_src = _upload(query_news_embeddings, self.device, self.dtype)
        else:
            self.hist_src = self.cand_table
        self._check_rows()
        self._cand_image = None
        self._req_of = None  # prepare_requests builds its tables again
        w = sliced_width(self.cand_table.shape[0], self.dtype, False, False, getattr(self, "pooler", "latent"))
        if w:  # a layout of the loaded table, like its dtype conversion
            self._candidate_image(w)
        return self

    def _candidate_image(self, w: int) -> torch.Tensor:
        """The candidate table's slice image of width ``w``, built once per loaded table (and
        again should the table have been replaced or written to since)."""
        t = self.cand_table
        key = (w, t.data_ptr(), tuple(t.shape), t._version)
        if getattr(self, "_cand_image", None) is None or self._cand_image_of != key:
            self._cand_image = ops.slice_table(t, w)
            self._cand_image_of = key
        return self._cand_image

    def set_catalogue(self, news_time=None, news_cat=None, news_prior=None, news_group=None):
        """Per-news attributes for the catalogue filters of recommend, recommend_diverse,
        recommend_explained and rank_targets: ``news_time`` int32 [N] (any unit; e.g. the
        time a news was first seen) and ``news_cat`` [N] category ids (0 .. 63 can be asked
        for; 64 .. 255 never match); and for ``prior_gain`` (recommend, recommend_sections,
        rank_targets) ``news_prior`` f32 [N], finite: a popularity or recency value per news; and
        for recommend's ``group_cap`` ``news_group`` [N], integer labels in [0, 1024) on the host
        or the device (data_utils.dense_groups makes them from any labels).
        None drops an attribute."""
        n = None if self.cand_table is None else self.cand_table.shape[0]
        prior = None if news_prior is None else check_prior(news_prior, n)
        groups = None if news_group is None else check_groups(news_group, n)
        up = {}
        for name, arr, dt in (("news_time", news_time, np.int32), ("news_cat", news_cat, np.uint8)):
            if arr is None:
                up[name] = None
                continue
            a = np.asarray(arr)
            if a.ndim != 1 or (n is not None and len(a) != n):
                raise ValueError(f"{name} must have one entry per news" + ("" if n is None else f" ({n})"))
            if not np.issubdtype(a.dtype, np.integer) or (len(a) and (a.min() < np.iinfo(dt).min
                                                                     or a.max() > np.iinfo(dt).max)):
                raise ValueError(f"{name} must be integers in the range of {np.dtype(dt).name}")
            up[name] = _upload(np.ascontiguousarray(a, dtype=dt), self.device)
        self.news_time, self.news_cat = up["news_time"], up["news_cat"]
        self.news_prior = None if prior is None else _upload(prior, self.device)
        self.news_group = None if groups is None else _upload(groups, self.device)
        return self

    def _queries(self, time_window, categories, prior_gain=None, after=None) -> Optional[_Queries]:
        """None without a filter, prior or cursor argument (today's paths run), else the distinct
        queries.  ``time_window`` = (lo, hi), ``categories`` = a 64-bit mask, ``prior_gain`` = the
        gain of the set news_prior; each a scalar or one value per impression.  ``after`` =
        check_cursor's pair: an impression's cursor is part of its query, as its gain is."""
        if time_window is None and categories is None and prior_gain is None and after is None:
            return None
        if prior_gain is not None and getattr(self, "news_prior", None) is None:
            raise ValueError("prior_gain needs set_catalogue(news_prior=...)")
        n = self.n_imp
        lo = hi = mask = gain = None
        keys = [self.user_idx.cpu().numpy().astype(np.int64) if self.user_idx is not None
                else np.arange(n, dtype=np.int64)]
        if time_window is not None:
            if self.news_time is None:
                raise ValueError("time_window needs set_catalogue(news_time=...)")
            lo_in, hi_in = time_window
            lo = np.broadcast_to(np.asarray(lo_in, dtype=np.int64), (n,))
            hi = np.broadcast_to(np.asarray(hi_in, dtype=np.int64), (n,))
            i32 = np.iinfo(np.int32)
            lo, hi = np.clip(lo, i32.min, i32.max).astype(np.int32), np.clip(hi, i32.min, i32.max).astype(np.int32)
            keys += [lo.astype(np.int64), hi.astype(np.int64)]
        if categories is not None:
            if self.news_cat is None:
                raise ValueError("categories needs set_catalogue(news_cat=...)")
            # Python ints, int64 or uint64 arrays: the same 64 bits, carried as int64
            m = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(categories).reshape(-1).tolist()],
                         dtype=np.uint64).view(np.int64)
            mask = np.ascontiguousarray(np.broadcast_to(m, (n,)))
            keys.append(mask)
        if prior_gain is not None:
            gain = check_gain(prior_gain, n)
            keys.append(gain.view(np.int32).astype(np.int64))
            if self.news_prior.numel() != self.cand_table.shape[0]:
                raise ValueError("the catalogue attributes must have one entry per news")
        if after is not None:  # the bits: NaN keys and -0 stay what they are
            keys += [after[0].view(np.int32).astype(np.int64), after[1].astype(np.int64)]
        if self.news_time is not None and self.news_time.numel() != self.cand_table.shape[0] or (
                self.news_cat is not None and self.news_cat.numel() != self.cand_table.shape[0]):
            raise ValueError("the catalogue attributes must have one entry per news")
        if n == 0:
            e = np.zeros(0, np.int64)
            return _Queries(e, e, lo, hi, mask, self.device, gain, after)
        _, first, sel = np.unique(np.stack(keys, axis=1), axis=0, return_index=True, return_inverse=True)
        sel = np.asarray(sel).reshape(-1)
        pick = lambda a: None if a is None else np.ascontiguousarray(a[first])
        return _Queries(keys[0][first], sel, pick(lo), pick(hi), pick(mask), self.device, pick(gain),
                        None if after is None else (pick(after[0]), pick(after[1])))

    def _query_block(self, q: _Queries, users, hidx, hoff, a: int, b: int, exclude_history: bool):
        """Queries [a, b): their pooled rows gathered (f32, so a block bounds them), their
        exclusion CSR gathered from the histories, and the filter tensors of the ops call."""
        qu = q.user[a:b]
        eidx = eoff = None
        if exclude_history:
            ln = hoff[qu + 1] - hoff[qu]
            eoff = torch.zeros(b - a + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(ln, 0, out=eoff[1:])
            total = int(eoff[-1])
            pos = (torch.arange(total, dtype=torch.int64, device=self.device)
                   + torch.repeat_interleave(hoff[qu] - eoff[:-1], ln, output_size=total))
            eidx = hidx[pos] if total else torch.zeros(0, dtype=torch.int32, device=self.device)
        flt = dict(news_time=self.news_time if q.lo is not None else None,
                   time_lo=None if q.lo is None else q.lo[a:b], time_hi=None if q.hi is None else q.hi[a:b],
                   news_cat=self.news_cat if q.mask is not None else None,
                   cat_mask=None if q.mask is None else q.mask[a:b])
        if q.gain is not None:  # the callers then run the prior entries
            flt.update(news_prior=self.news_prior, user_gain=q.gain[a:b])
        return users[qu], eidx, eoff, flt

    def _distinct_hist(self):
        """The history CSR with one segment per DISTINCT history: (hidx, hoff), the
        deduplicated CSR when load_impressions built it, else the impressions' own."""
        if self.user_idx is not None:
            return self.uhist_idx, self.uhist_off
        return self.hist_idx, self.hist_off

    def _pooled_users(self, hidx, hoff) -> torch.Tensor:
        """The histories' pooled rows, f32 [n_u, D], in a buffer reused across calls."""
        n_u = hoff.numel() - 1
        if self._users is None or self._users.shape[0] != n_u:
            self._users = torch.empty((n_u, 1024), dtype=torch.float32, device=self.device)
        return ops.pool_users(self.pooler, self.hist_table, hidx, hoff, out=self._users)

    def _blocks(self, q: Optional[_Queries], users, hidx, hoff, n_rows: int, blk: int, exclude_history: bool,
                wanted=None):
        """The rows a scan of the table sees -- distinct histories, or with ``q`` distinct queries
        -- in blocks of ``blk``: yields (a, b, rows, eidx, eoff, flt) with the pooled rows
        [a, b), their exclusion CSR (None without ``exclude_history``) and the filter arguments
        of the ops call ({} without ``q``).  Without ``q`` these are views: the offsets rebased
        on the device, the indices' tail shared.  ``wanted(a, b)`` false skips a block unbuilt."""
        for a in range(0, n_rows, blk):
            b = min(a + blk, n_rows)
            if wanted is not None and not wanted(a, b):
                continue
            if q is not None:
                yield (a, b) + self._query_block(q, users, hidx, hoff, a, b, exclude_history)
                continue
            eidx = eoff = None
            if exclude_history:
                eoff = hoff[a:b + 1] - hoff[a:a + 1] if a else hoff[:b + 1]
                eidx = hidx[int(self._hoff_host(hoff)[a]):] if a else hidx
            yield a, b, users[a:b], eidx, eoff, {}

    def load_impressions(self, hist_idx, hist_len, cand_idx, cand_len, dedupe: Optional[bool] = None):
        """Upload the CSR index arrays.  ``dedupe`` (default: automatic) pools
        each DISTINCT history once (MIND repeats a user's history on every
        impression of that user) and scores the candidates against the stored
        user rows: same scores bit for bit, fewer gathered bytes once at least
        DEDUPE_MIN_SHARE of the impressions repeat a history.  ``dedupe=False`` asks for the
        fused per-impression pass those bits are defined by (pool_score_kernel), so it also keeps
        pool_score off the column-sliced path, whose scores differ by f32 reassociation; the
        automatic mode is free to take it (sliced_width) when the histories are not deduplicated."""
        dev = self.device
        if len(hist_len) != len(cand_len):
            raise ValueError("Number of rows should be consistent")  # data_model_helper.py:183-185
        hist_idx = np.ascontiguousarray(hist_idx, dtype=np.int32)
        hist_len = np.asarray(hist_len, dtype=np.int64)
        cand_idx = np.ascontiguousarray(cand_idx, dtype=np.int32)
        cand_len_a = np.asarray(cand_len, dtype=np.int64)
        _check_segments(hist_idx, hist_len, "history")
        _check_segments(cand_idx, cand_len_a, "candidate")
        hi_d, ci_d = _upload(hist_idx, dev), _upload(cand_idx, dev)
        # the kernels index tables with these rows: an out-of-range row would be an
        # out-of-bounds device read, so refuse it here, before the engine takes the
        # arrays (a refused load leaves the previous impressions in place), as torch
        # indexing does (IndexError)
        max_row = {"hist": _row_range(hi_d, "history"), "cand": _row_range(ci_d, "candidate")}
        prev, self._max_row = getattr(self, "_max_row", None), max_row
        try:
            self._check_rows()
        except IndexError:
            self._max_row = prev
            raise
        self.hist_idx, self.cand_idx = hi_d, ci_d
        self.hist_off = _upload(lengths_to_offsets(hist_len), dev)
        self.cand_off = _upload(lengths_to_offsets(cand_len_a), dev)
        self.n_cand = int(cand_len_a.sum())
        self.n_imp = len(cand_len)
        self.user_idx = None
        self._fused_asked = dedupe is False
        self.shared_history_share = 0.0
        if dedupe is not False and self.n_imp and (dedupe or _may_repeat(hist_idx, hist_len)):
            group, first = distinct_segments(hist_idx, hist_len)
            self.shared_history_share = 1.0 - len(first) / self.n_imp
            if dedupe or self.shared_history_share >= DEDUPE_MIN_SHARE:
                ho, ulen = lengths_to_offsets(hist_len), hist_len[first]
                uoff = lengths_to_offsets(ulen)
                rows = np.repeat(ho[:-1][first], ulen) + (np.arange(int(uoff[-1])) - np.repeat(uoff[:-1], ulen))
                self.uhist_idx = _upload(hist_idx[rows], dev)
                self.uhist_off = _upload(uoff, dev)
                self.user_idx = _upload(group.astype(np.int32), dev)
        return self

    # ------------------------------------------------------------ stages
    def _workspace(self, n: int) -> torch.Tensor:
        from . import _lib
        dt = _lib.NR_F32 if self.dtype == torch.float32 else _lib.NR_BF16
        fn = (_lib.load().nr_final_attn_workspace_bytes if self.pooler == "final"
              else _lib.load().nr_latent_workspace_bytes)
        self._ws = ops.grow_workspace(self._ws, fn(dt, n), self.device)
        return self._ws

    def transform(self, rows: Optional[slice] = None, out: Optional[torch.Tensor] = None,
                  src: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-news pooler table for src[rows] (default: all rows of hist_src)."""
        src = self.hist_src if src is None else src
        src = src if rows is None else src[rows]
        ws = self._workspace(src.shape[0])
        if self.pooler == "final":
            return ops.final_attn_transform(src, self.weights, out=out, workspace=ws)
        return ops.latent_transform(src, self.weights, out=out, workspace=ws)

    def inv_norms(self) -> torch.Tensor:
        self.cand_inv = ops.row_inv_norm(self.cand_table, 1e-8, out=self.cand_inv)
        return self.cand_inv

    def _check_rows(self) -> None:
        """Host-side: every index row of the loaded impressions exists in the loaded
        tables (no device sync; the maxima were taken at load_impressions)."""
        mr = getattr(self, "_max_row", None)
        if mr is None:
            return
        for name, table in (("hist", self.hist_src), ("cand", self.cand_table)):
            if table is not None and mr[name] >= table.shape[0]:
                raise IndexError(f"{'history' if name == 'hist' else 'candidate'} index {mr[name]} is out of bounds "
                                 f"for dimension 0 with size {table.shape[0]}")

    def pool_score(self, want_users: bool = False, scores: Optional[torch.Tensor] = None):
        """(scores [C] f32, users [I, D] f32 or None) of the loaded impressions.  Deduplicated
        histories and ``want_users`` run today's kernels; otherwise sliced_width decides between
        today's fused kernel and the column-sliced path on the tables' slice images, whose scores
        differ from the fused kernel's by f32 reassociation only; load_impressions(dedupe=False)
        keeps the fused kernel.  Images and workspace are allocated once and reused across steps."""
        if self.user_idx is not None:  # distinct histories pooled once, then scored per impression
            users = self._pooled_users(self.uhist_idx, self.uhist_off)
            s = ops.score_users(users, self.user_idx, self.cand_table, self.cand_inv, self.cand_idx, self.cand_off,
                                self.n_cand, scores=scores)
            return s, (users[self.user_idx.long()] if want_users else None)
        w = 0 if getattr(self, "_fused_asked", False) else sliced_width(self.cand_table.shape[0], self.dtype,
                                                                          want_users, False, self.pooler)
        if not w:
            return ops.pool_score(self.pooler, self.hist_table, self.cand_table, self.cand_inv, self.hist_idx,
                                  self.hist_off, self.cand_idx, self.cand_off, self.n_cand, want_users=want_users,
                                  scores=scores)
        # the transformed table changes every step, so its image is rebuilt here (into the
        # same buffer); hist_table itself stays row-major for every other reader
        parts = 2 if self.pooler == "final" else 1
        shape = (1024 // w, self.hist_table.shape[0], parts * w)
        img = getattr(self, "_hist_image", None)
        if img is not None and (tuple(img.shape) != shape or img.dtype != self.hist_table.dtype):
            img = None
        self._hist_image = ops.slice_table(self.hist_table, w, parts, out=img)
        self._sliced_ws = ops.grow_workspace(
            getattr(self, "_sliced_ws", None), max(ops.pool_score_sliced_workspace_bytes(w, self.n_imp, self.n_cand), 256), self.device)
        return ops.pool_score(self.pooler, self.hist_table, self.cand_table, self.cand_inv, self.hist_idx,
                              self.hist_off, self.cand_idx, self.cand_off, self.n_cand, scores=scores, sliced=w,
                              hist_image=self._hist_image, cand_image=self._candidate_image(w),
                              workspace=self._sliced_ws)

    def step(self, want_users: bool = False, scores: Optional[torch.Tensor] = None):
        """Full eval pass: transform + inverse norms + pool/score."""
        self.hist_table = self.transform(out=self.hist_table)
        self.inv_norms()
        return self.pool_score(want_users=want_users, scores=scores)

    def _recommend_distinct(self, k: int, exclude_history: bool, user_block: Optional[int],
                            q: Optional[_Queries] = None, want_keys: bool = False, group_cap=None):
        """recommend's lists per DISTINCT history (the deduplicated CSR when
        load_impressions built it, else one per impression): (idx [n_u, k], scores [n_u, k]).
        Under a catalogue filter or a prior ``q``: per distinct query, [q.n, k].  ``want_keys``
        appends what the lists are ordered by (the scores themselves without a prior).
        ``group_cap``: at most that many news of one news_group per list (ops.topk_users_capped)."""
        capped = group_cap is not None
        if not 1 <= k <= PAGE_MAX:  # the entry's own refusal, ahead of the device work
            ops.topk_workspace_bytes(self.dtype, 1, self.cand_table.shape[0], k)
        if capped:
            if isinstance(group_cap, bool) or not isinstance(group_cap, (int, np.integer)) or not 1 <= group_cap <= 64:
                raise ValueError(f"group_cap = {group_cap!r} must be an integer in 1 .. 64")
            if getattr(self, "news_group", None) is None:
                raise ValueError("group_cap needs set_catalogue(news_group=...)")
            if self.news_group.numel() != self.cand_table.shape[0]:
                raise ValueError("the catalogue attributes must have one entry per news")
        self.hist_table = self.transform(out=self.hist_table)
        self.inv_norms()
        hidx, hoff = self._distinct_hist()
        n_rows = hoff.numel() - 1 if q is None else q.n
        idx = torch.empty((n_rows, k), dtype=torch.int32, device=self.device)
        scores = torch.empty((n_rows, k), dtype=torch.float32, device=self.device)
        prior = q is not None and q.gain is not None
        keys = torch.empty((n_rows, k), dtype=torch.float32, device=self.device) if prior or capped else None
        if n_rows:
            users = self._pooled_users(hidx, hoff)  # pooled once per distinct history, searched once per distinct query
            blk = n_rows if not user_block else max(1, min(int(user_block), n_rows))
            need = (ops.topk_users_prior_workspace_bytes if prior or capped else ops.topk_workspace_bytes)(
                self.dtype, blk, self.cand_table.shape[0], k)
            self._topk_ws = ops.grow_workspace(getattr(self, "_topk_ws", None), need, self.device)
            for a, b, rows, eidx, eoff, flt in self._blocks(q, users, hidx, hoff, n_rows, blk, exclude_history):
                if capped:
                    ops.topk_users_capped(rows, self.cand_table, self.cand_inv, k, self.news_group, int(group_cap),
                                          excl_idx=eidx, excl_off=eoff, out=(idx[a:b], scores[a:b], keys[a:b]),
                                          workspace=self._topk_ws, **flt)
                    continue
                if prior:
                    ops.topk_users_prior(rows, self.cand_table, self.cand_inv, k, excl_idx=eidx, excl_off=eoff,
                                         out=(idx[a:b], scores[a:b], keys[a:b]), workspace=self._topk_ws, **flt)
                    continue
                (ops.topk_users_filtered if flt else ops.topk_users)(
                    rows, self.cand_table, self.cand_inv, k, excl_idx=eidx, excl_off=eoff,
                    out=(idx[a:b], scores[a:b]), workspace=self._topk_ws, **flt)
        if want_keys:
            return idx, scores, (keys if prior or capped else scores.clone())
        return idx, scores

    def _expansion(self, q: Optional[_Queries]) -> Optional[torch.Tensor]:
        """Row of the distinct lists behind each impression (None: one list per impression)."""
        if q is not None:
            return q.sel
        return None if self.user_idx is None else self.user_idx.long()

    def _paged_distinct(self, sizes, exclude_history: bool, user_block: Optional[int], q: Optional[_Queries] = None,
                        deep: bool = False):
        """Consecutive pages of ``sizes[p]`` rows (each 1 .. 64; with ``deep`` 1 .. 256, by
        ops.topk_users_deep: one walk over the table per page) per DISTINCT history, or with ``q``
        per distinct query, by cursor calls (ops.topk_users_after) that start at the queries'
        cursors (``q.after``; the start of the list without).  Returns (idx, scores, keys), each
        [n_rows, sum(sizes)] with the pages side by side, and the cursor behind the last page
        (key f32 [n_rows], row int32 [n_rows]).  The cursors stay on the device: nothing waits
        for a page before the next one is enqueued."""
        self.hist_table = self.transform(out=self.hist_table)
        self.inv_norms()
        hidx, hoff = self._distinct_hist()
        n_rows = hoff.numel() - 1 if q is None else q.n
        dev = self.device
        pages = [tuple(torch.empty((n_rows, k), dtype=dt, device=dev)
                       for dt in (torch.int32, torch.float32, torch.float32)) for k in sizes]
        if q is not None and q.after is not None:
            cur = (q.after[0].clone(), q.after[1].clone())
        else:
            cur = ops.start_cursor(n_rows, dev)
        if n_rows:
            users = self._pooled_users(hidx, hoff)
            blk = n_rows if not user_block else max(1, min(int(user_block), n_rows))
            op, op_bytes = ((ops.topk_users_deep, ops.topk_users_deep_workspace_bytes) if deep else
                            (ops.topk_users_after, ops.topk_users_after_workspace_bytes))
            need = max(op_bytes(self.dtype, blk, self.cand_table.shape[0], k) for k in set(sizes))
            self._topk_ws = ops.grow_workspace(getattr(self, "_topk_ws", None), need, dev)
            for a, b, rows, eidx, eoff, flt in self._blocks(q, users, hidx, hoff, n_rows, blk, exclude_history):
                at = (cur[0][a:b], cur[1][a:b])  # read by a call's first kernels, rewritten by its last
                for p, k in enumerate(sizes):
                    op(rows, self.cand_table, self.cand_inv, k, after=at, next_out=at, excl_idx=eidx, excl_off=eoff,
                       out=tuple(t[a:b] for t in pages[p]), workspace=self._topk_ws, excl_checked=p > 0, **flt)
        return tuple(torch.cat([pg[i] for pg in pages], dim=1) if len(pages) > 1 else pages[0][i]
                     for i in range(3)) + (cur,)

    def recommend_deep(self, k: int, page: int = 64, exclude_history: bool = True, user_block: Optional[int] = None,
                       time_window=None, categories=None, prior_gain=None, want_keys: bool = False,
                       walk: Optional[int] = None):
        """recommend past 64 rows: the k best news (1 <= k <= 1024) per impression, fetched in
        ceil(k / page) cursor calls of ``page`` rows (1 .. 64; the last call asks for the
        remainder), each continuing where the one before ended (ops.topk_users_after): the
        pages are consecutive, disjoint slices of the order the retrieval selects in, so together
        they are the k best rows of that order, and no state grows with the depth.  The
        concatenated list is then ordered by (key descending, row ascending) -- the key is the
        score without ``prior_gain`` -- and returned as recommend returns it: (idx int32 [I, k],
        scores f32 [I, k]) and with ``want_keys`` the keys, (-1, -inf) where fewer than k rows
        are eligible.  The other arguments are recommend's (``group_cap`` is not taken).  For
        k <= 64 with page = k it is recommend(k) bit for bit.

        ``walk`` = W (1 .. 256; ``page`` left at its default) fetches the list in ceil(k / W)
        chained calls of W rows that each keep their whole list over ONE walk of the table
        (ops.topk_users_deep): 256 rows cost one users x table product instead of four, 1024
        four instead of sixteen.  The result is the same bit for bit for every ``walk`` and
        ``page``; the workspace grows to 4 KiB per distinct user (``user_block`` bounds it)."""
        check_deep("recommend_deep", k, page, walk)
        k, page = int(k), int(page if walk is None else walk)
        q = self._queries(time_window, categories, prior_gain)
        sizes = [page] * (k // page) + ([k % page] if k % page else [])
        idx, scores, keys, _ = self._paged_distinct(sizes, exclude_history, user_block, q, deep=walk is not None)
        if len(sizes) > 1 and idx.shape[0]:
            # (key descending, row ascending) by two stable sorts: rows first, then keys
            by_row = torch.sort(idx, dim=1, stable=True).indices
            by_key = torch.sort(keys.gather(1, by_row), dim=1, descending=True, stable=True).indices
            order = by_row.gather(1, by_key)
            idx, scores, keys = (t.gather(1, order) for t in (idx, scores, keys))
        out = (idx, scores) + ((keys,) if want_keys else ())
        sel = self._expansion(q)
        if sel is not None and idx.shape[0]:
            return tuple(t[sel] for t in out)
        return out

    def recommend(self, k: int, exclude_history: bool = True, user_block: Optional[int] = None,
                  time_window=None, categories=None, prior_gain=None, want_keys: bool = False, group_cap=None,
                  after=None, want_cursor: bool = False):
        """The k best news of the WHOLE table per impression (ops.topk_users over the
        pooled users): (idx int32 [I, k], scores f32 [I, k]), score descending, ties by
        ascending row, (-1, -inf) where fewer than k rows are eligible; the scores are
        pool_score's for that (impression, news) pair bit for bit (today's kernel's,
        ops.pool_score(sliced=False): the column-sliced path that pool_score takes on large
        bf16 tables sums the dot per slice and differs by f32 reassociation).  ``exclude_history``
        leaves an impression's own history out of its list.  Distinct histories are
        pooled and searched once (the deduplicated CSR when load_impressions built it).
        ``user_block`` bounds the workspace by running the users in blocks of that many
        rows; the results do not depend on it.

        Catalogue filters (set_catalogue): ``time_window`` = (lo, hi) keeps the news with lo <=
        news_time <= hi (inclusive; lo > hi is empty), ``categories`` = a 64-bit mask keeps
        the news whose category's bit is set; each a scalar or one value per impression.
        Users are still pooled once per distinct history; the table is searched once per
        distinct (history, lo, hi, mask).  Without either argument nothing changes.

        ``prior_gain`` = g (a finite scalar or one value per impression; needs
        set_catalogue(news_prior=...)) selects and orders the news by ``score + g * news_prior``
        (ops.topk_users_prior): a popularity or recency prior; g = 0 changes nothing for that
        impression, and an empty history is ordered by the prior alone.  The gain is part of
        the distinct query.  The returned scores stay the cosines; ``want_keys`` appends the
        keys f32 [I, k] the lists are ordered by (the scores themselves without a gain).
        Without ``prior_gain`` today's paths run.

        ``group_cap`` = c (1 .. 64; needs set_catalogue(news_group=...)) allows at most c news
        of one group in a list (ops.topk_users_capped): the eligible news are walked best first
        and one is taken while its group holds fewer than c, until k are taken, so a list may
        be shorter than k.  It composes with every argument above; c >= k changes nothing, and
        without ``group_cap`` today's paths run.

        ``after`` = (key f32 [I], row int32 [I]), the pair a previous call returned with
        ``want_cursor``, continues each impression's list behind that position
        (ops.topk_users_after): the next k rows of the same ordering, disjoint from every page
        before.  ``want_cursor`` appends the pair behind this call's last row to the result (the
        end cursor (-inf, INT32_MAX) where fewer than k rows were left).  A cursor is opaque --
        selection keys, not scores -- and valid only with the same history, table, dtype and
        ``prior_gain``; ``time_window`` / ``categories`` / ``exclude_history`` may change between
        pages.  It is part of the distinct query, as the gain is.  Inside a page the order is by
        score (by key); across a boundary scores may be out of order by the selection band
        (include/newsrec_page.h).  ``group_cap`` is refused with either; without both today's
        paths run."""
        if after is not None or want_cursor:
            if group_cap is not None:
                raise ValueError("recommend: after / want_cursor cannot be combined with group_cap (no cursors under "
                                 "per-group caps)")
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= PAGE_MAX:
                raise ValueError(f"recommend: k = {k!r} must be an integer in 1 .. {PAGE_MAX} with a cursor "
                                 "(recommend_deep pages further)")
            cur = None if after is None else check_cursor(after, self.n_imp)
            q = self._queries(time_window, categories, prior_gain, after=cur)
            idx, scores, keys, nxt = self._paged_distinct([int(k)], exclude_history, user_block, q)
            sel = self._expansion(q)
            out = (idx, scores) + ((keys,) if want_keys else ())
            if sel is not None and idx.shape[0]:
                out, nxt = tuple(t[sel] for t in out), (nxt[0][sel], nxt[1][sel])
            return out + ((nxt,) if want_cursor else ())
        q = self._queries(time_window, categories, prior_gain)
        out = self._recommend_distinct(k, exclude_history, user_block, q, want_keys=want_keys, group_cap=group_cap)
        sel = self._expansion(q)
        if sel is not None and out[0].shape[0]:
            return tuple(t[sel] for t in out)
        return out

    # ------------------------------------------------------------ the request path
    def prepare_requests(self):
        """The tables recommend_request reads -- the transformed history table and the candidate
        rows' inverse norms -- built once for the loaded tables and again only when ``cand_table``
        or ``hist_src`` was replaced or written to (their data_ptr, shape and _version, as
        _candidate_image keys its image).  They are the request path's own: recommend* keep
        rebuilding theirs."""
        if self.cand_table is None:
            raise ValueError("prepare_requests: load_news first")
        key = tuple((t.data_ptr(), tuple(t.shape), t._version) for t in (self.cand_table, self.hist_src))
        if getattr(self, "_req_of", None) != key:
            hist = getattr(self, "_req_hist", None)
            inv = getattr(self, "_req_inv", None)
            if inv is not None and inv.shape[0] != self.cand_table.shape[0]:
                inv = None
            self._req_of = None
            self._req_hist = self.transform(out=hist if hist is not None and hist.shape[0] == self.hist_src.shape[0]
                                            else None)
            self._req_inv = ops.row_inv_norm(self.cand_table, 1e-8, out=inv)
            self._req_of = key
        return self

    def _request_rows(self, what: str, arrays, n_rows: int) -> list:
        """``arrays`` as int32 host arrays of rows below ``n_rows`` (IndexError otherwise, as
        _check_rows raises)."""
        out = []
        for a in arrays:
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)) or a.dtype == np.bool_:
                raise ValueError(f"recommend_request: {what} must be 1-D integer arrays of news rows")
            if a.size and (int(a.min()) < 0 or int(a.max()) >= n_rows):
                bad = int(a.min()) if int(a.min()) < 0 else int(a.max())
                raise IndexError(f"{what} index {bad} is out of bounds for dimension 0 with size {n_rows}")
            out.append(np.ascontiguousarray(a, dtype=np.int32))
        return out

    def recommend_request(self, histories, k: int, exclude_history: bool = True, exclude=None, time_window=None,
                          categories=None, prior_gain=None, want_keys: bool = False, after=None,
                          want_cursor: bool = False):
        """recommend for the readers of a request: ``histories`` is a sequence of 1 .. 32 integer
        arrays of news rows (an empty array is a cold reader), and the result is recommend's for
        impressions with these histories, bit for bit -- (idx int32 [R, k], scores f32 [R, k]),
        with ``want_keys`` the keys, with ``want_cursor`` the (key, row) pair behind the lists --
        with one value per reader wherever recommend takes one per impression.  Nothing of
        load_impressions is needed or touched.  The per-news tables come from prepare_requests
        (built once per loaded table); the readers are pooled (ops.pool_users) and searched by
        ops.topk_request: one read of the table with the whole device busy, where recommend's
        kernels are shaped for hundreds of thousands of users.  ``exclude`` is a sequence of
        arrays of rows already shown, one per reader, left out like the history.  The pooled rows
        and the workspace live on the engine across calls.  ``group_cap``, sections, ``walk`` and
        ``page`` are recommend's and recommend_deep's; MMR and explanations take the returned
        lists.  More than 32 readers: load_impressions and recommend."""
        from . import _lib
        if isinstance(histories, (str, bytes, np.ndarray, torch.Tensor)) or not hasattr(histories, "__len__"):
            raise ValueError("recommend_request: histories must be a sequence of integer arrays, one per reader")
        n = len(histories)
        if n > _lib.NR_REQUEST_MAX_USERS:
            raise ValueError(f"recommend_request: {n} histories (at most {_lib.NR_REQUEST_MAX_USERS}; "
                             "load_impressions and recommend serve more)")
        if n < 1:
            raise ValueError("recommend_request: histories must hold at least one reader")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= PAGE_MAX:
            raise ValueError(f"recommend_request: k = {k!r} must be an integer in 1 .. {PAGE_MAX}")
        if self.cand_table is None:
            raise ValueError("recommend_request: load_news first")
        k, dev, n_news = int(k), self.device, self.cand_table.shape[0]
        hists = self._request_rows("history", histories, self.hist_src.shape[0])
        shown = [np.zeros(0, np.int32)] * n
        if exclude is not None:
            if isinstance(exclude, (str, bytes, np.ndarray, torch.Tensor)) or not hasattr(exclude, "__len__") \
                    or len(exclude) != n:
                raise ValueError(f"recommend_request: exclude must hold one array of rows per reader ({n})")
            shown = self._request_rows("exclude", exclude, n_news)
        flt = {}
        if time_window is not None:
            if self.news_time is None:
                raise ValueError("time_window needs set_catalogue(news_time=...)")
            i32 = np.iinfo(np.int32)
            lo, hi = (np.clip(np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)), i32.min, i32.max).astype(np.int32)
                      for v in time_window)
            flt.update(news_time=self.news_time, time_lo=_upload(lo, dev), time_hi=_upload(hi, dev))
        if categories is not None:
            if self.news_cat is None:
                raise ValueError("categories needs set_catalogue(news_cat=...)")
            m = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(categories).reshape(-1).tolist()],
                         dtype=np.uint64).view(np.int64)
            flt.update(news_cat=self.news_cat, cat_mask=_upload(np.broadcast_to(m, (n,)).copy(), dev))
        if prior_gain is not None:
            if getattr(self, "news_prior", None) is None:
                raise ValueError("prior_gain needs set_catalogue(news_prior=...)")
            flt.update(news_prior=self.news_prior, user_gain=_upload(check_gain(prior_gain, n), dev))
        if any(t is not None and t.numel() != n_news for t in (flt.get("news_time"), flt.get("news_cat"),
                                                                flt.get("news_prior"))):
            raise ValueError("the catalogue attributes must have one entry per news")
        cur = None
        if after is not None:
            key, row = check_cursor(after, n)
            cur = (_upload(key, dev), _upload(row, dev))
        self.prepare_requests()
        hoff = lengths_to_offsets(np.array([len(h) for h in hists], dtype=np.int64))
        hidx = np.concatenate(hists) if n else np.zeros(0, np.int32)
        users = getattr(self, "_req_users", None)
        if users is None:
            users = self._req_users = torch.empty((_lib.NR_REQUEST_MAX_USERS, 1024), dtype=torch.float32, device=dev)
        users = ops.pool_users(self.pooler, self._req_hist, _upload(hidx, dev), _upload(hoff, dev), out=users[:n])
        eidx = eoff = None
        if exclude_history or exclude is not None:
            # a history row that the candidate table does not have excludes nothing
            rows = [np.concatenate((h[h < n_news] if exclude_history else h[:0], s)) for h, s in zip(hists, shown)]
            eoff = _upload(lengths_to_offsets(np.array([len(r) for r in rows], dtype=np.int64)), dev)
            eidx = _upload(np.concatenate(rows).astype(np.int32), dev)
        self._req_ws = ops.grow_workspace(getattr(self, "_req_ws", None),
                                          ops.topk_request_workspace_bytes(self.dtype, n, n_news, k), dev)
        idx, scores, keys, nxt = ops.topk_request(users, self.cand_table, self._req_inv, k, after=cur,
                                                  want_next=want_cursor, excl_idx=eidx, excl_off=eoff,
                                                  workspace=self._req_ws, excl_checked=True, **flt)
        return (idx, scores) + ((keys,) if want_keys else ()) + ((nxt,) if want_cursor else ())

    def recommend_sections(self, k: int, sections, exclude_history: bool = True, user_block: Optional[int] = None,
                           time_window=None, prior_gain=None, want_keys: bool = False, group_cap=None, after=None):
        """A front page per impression: the k best eligible news of each of S sections, from
        ONE walk over the table (ops.topk_sections): (idx int32 [I, S, k], scores f32
        [I, S, k]).  ``sections`` is a sequence whose items are a 64-bit category mask or an
        iterable of category ids (0 .. 63); the sections are disjoint, at most 16, and
        S * k <= 64.  Section s equals recommend(k, categories=mask_s, time_window=...) bit
        for bit.  Needs set_catalogue(news_cat=...), with ``time_window`` also news_time.
        Users are pooled once per distinct history and the table is searched once per
        distinct (history, lo, hi); the results do not depend on ``user_block``.  ``prior_gain`` /
        ``want_keys`` are recommend's (ops.topk_sections_prior): section s then equals
        recommend(k, categories=mask_s, prior_gain=...), keys included."""
        _no_cap("recommend_sections", group_cap)
        _no_cursor("recommend_sections", after=after)
        masks = section_masks(sections)
        k, n_sec = int(k), len(masks)
        if not 1 <= n_sec <= 16 or k < 1 or n_sec * k > 64:
            raise ValueError(f"recommend_sections: {n_sec} sections of k = {k} (1 .. 16 sections, k >= 1, "
                             "sections * k <= 64)")
        for i in range(n_sec):
            for j in range(i):
                if masks[i] & masks[j]:
                    raise ValueError(f"recommend_sections: sections {j} and {i} share a category (sections are "
                                     "disjoint)")
        if self.news_cat is None:
            raise ValueError("sections needs set_catalogue(news_cat=...)")
        if self.news_cat.numel() != self.cand_table.shape[0]:
            raise ValueError("the catalogue attributes must have one entry per news")
        q = self._queries(time_window, None, prior_gain)
        self.hist_table = self.transform(out=self.hist_table)
        self.inv_norms()
        hidx, hoff = self._distinct_hist()
        n_rows = hoff.numel() - 1 if q is None else q.n
        idx = torch.empty((n_rows, n_sec, k), dtype=torch.int32, device=self.device)
        scores = torch.empty((n_rows, n_sec, k), dtype=torch.float32, device=self.device)
        prior = q is not None and q.gain is not None
        keys = torch.empty((n_rows, n_sec, k), dtype=torch.float32, device=self.device) if prior else None
        if n_rows:
            users = self._pooled_users(hidx, hoff)
            blk = n_rows if not user_block else max(1, min(int(user_block), n_rows))
            need = (ops.topk_sections_prior_workspace_bytes if prior else ops.topk_sections_workspace_bytes)(
                self.dtype, blk, self.cand_table.shape[0], n_sec, k)
            self._topk_ws = ops.grow_workspace(getattr(self, "_topk_ws", None), need, self.device)
            for a, b, rows, eidx, eoff, flt in self._blocks(q, users, hidx, hoff, n_rows, blk, exclude_history):
                win = dict(news_time=flt.get("news_time"), time_lo=flt.get("time_lo"), time_hi=flt.get("time_hi"))
                if prior:
                    ops.topk_sections_prior(rows, self.cand_table, self.cand_inv, k, masks, self.news_cat,
                                            news_prior=flt["news_prior"], user_gain=flt["user_gain"], excl_idx=eidx,
                                            excl_off=eoff, out=(idx[a:b], scores[a:b], keys[a:b]),
                                            workspace=self._topk_ws, **win)
                    continue
                ops.topk_sections(rows, self.cand_table, self.cand_inv, k, masks, self.news_cat, excl_idx=eidx,
                                  excl_off=eoff, out=(idx[a:b], scores[a:b]), workspace=self._topk_ws, **win)
        out = (idx, scores) + (((keys if prior else scores.clone()),) if want_keys else ())
        sel = self._expansion(q)
        if sel is not None and n_rows:
            return tuple(t[sel] for t in out)
        return out

    def recommend_diverse(self, k: int, lam: float, pool: int = 64, exclude_history: bool = True,
                          user_block: Optional[int] = None, want_ild: bool = False, want_plain: bool = False,
                          time_window=None, categories=None, prior_gain=None, group_cap=None, after=None):
        """recommend's lists re-ranked for diversity (ops.rerank_mmr, greedy MMR): the
        ``pool`` best news per distinct history are retrieved as recommend(pool) does,
        k of them are picked one at a time, each maximising lam * score - (1 - lam) *
        (largest cosine to a news already picked), and only then are the lists expanded
        to the impressions.  Returns (idx int32 [I, k], scores f32 [I, k]) -- the scores
        are recommend's for the chosen news, in pick order -- and with ``want_ild`` also
        f32 [I, 2]: the intra-list diversity (mean 1 - cosine over the pairs) of
        recommend(k)'s list and of the returned one; with ``want_plain`` also recommend(k)'s
        scores f32 [I, k] (the pool's first k), for comparing the relevance given up.
        lam = 1 returns recommend(k).  ``time_window`` / ``categories`` filter the retrieved pool
        as in recommend; the re-ranking itself sees only that pool.  ``prior_gain`` is refused:
        MMR re-ranks by the scores alone."""
        _no_prior("recommend_diverse", prior_gain)
        _no_cap("recommend_diverse", group_cap)
        _no_cursor("recommend_diverse", after=after)
        q = self._queries(time_window, categories)
        idx, scores, ild, pscores = self._diverse_distinct(k, lam, pool, exclude_history, user_block, want_ild, q)
        k = int(k)
        sel = self._expansion(q)
        if idx.shape[0] and sel is not None:
            idx, scores = idx[sel], scores[sel]
            ild = ild[sel] if want_ild else None
            pscores = pscores[sel] if want_plain else pscores
        return (idx, scores) + ((ild,) if want_ild else ()) + ((pscores[:, :k].contiguous(),) if want_plain else ())

    def _diverse_distinct(self, k: int, lam: float, pool: int, exclude_history: bool, user_block: Optional[int],
                          want_ild: bool = False, q: Optional[_Queries] = None):
        """recommend_diverse's lists per DISTINCT history: (idx [n_u, k], scores [n_u, k], ild
        [n_u, 2] or None, the retrieved pool's scores [n_u, pool])."""
        k, pool = int(k), int(pool)
        if pool < k:
            raise ValueError(f"recommend_diverse: pool = {pool} < k = {k}")
        # lam = 1 keeps recommend's order: its list is the first k of any pool, so only k are retrieved
        pidx, pscores = self._recommend_distinct(k if float(lam) == 1.0 else pool, exclude_history, user_block, q)
        n_u = pidx.shape[0]
        idx = torch.empty((n_u, k), dtype=torch.int32, device=self.device)
        scores = torch.empty((n_u, k), dtype=torch.float32, device=self.device)
        ild = torch.empty((n_u, 2), dtype=torch.float32, device=self.device) if want_ild else None
        if n_u:
            ops.rerank_mmr(self.cand_table, self.cand_inv, pidx, pscores, k, lam, want_ild=want_ild,
                           out=(idx, scores, None, ild, None))
        return idx, scores, ild, pscores

    def explain(self, idx: torch.Tensor, top: int = 3, want_sum: bool = False, want_matrix: bool = False,
                prior_gain=None):
        """Why these news: the exact per-click attribution of the scores of one list per
        impression (ops.explain_scores over the loaded history CSR).  ``idx`` int32 [I, K]
        rows of the news table (K <= 64; an entry outside the table is a pad): recommend's
        or recommend_diverse's lists, or an impression's own candidates padded to a
        rectangle.  Returns (top_pos int32 [I, K, top], top_val f32 [I, K, top]): the
        positions within the impression's history of the ``top`` clicks that contributed
        most to each listed news' score and their contributions (-1, -inf past the
        history's length or for a pad); with ``want_sum`` also f32 [I, K], every click's
        contributions added up (pool_score's score of the pair, up to the f32 order of the
        sums: of today's kernel and of the column-sliced path alike); with ``want_matrix`` also
        f32 [len(hist_idx), K], all of them.  The pooler table and the inverse norms are
        computed when a step has not left them.  ``prior_gain`` is refused: a prior is no click's
        contribution."""
        _no_prior("explain", prior_gain)
        idx = torch.as_tensor(idx).to(self.device)
        if idx.dim() != 2 or idx.shape[0] != self.n_imp:
            raise ValueError("Number of rows should be consistent")
        self._tables()
        return ops.explain_scores(self.pooler, self.hist_table, self.cand_table, self.cand_inv, self.hist_idx,
                                  self.hist_off, idx.to(torch.int32).contiguous(), top=top, want_sum=want_sum,
                                  want_matrix=want_matrix)

    def _tables(self) -> None:
        if self.hist_table is None:
            self.hist_table = self.transform()
        if self.cand_inv is None:
            self.inv_norms()

    def recommend_explained(self, k: int, top: int = 3, lam: Optional[float] = None, pool: int = 64,
                            exclude_history: bool = True, user_block: Optional[int] = None):
        """recommend's lists (with ``lam``: recommend_diverse's, re-ranked from the ``pool``
        best) together with their reasons: (idx int32 [I, k], scores f32 [I, k], why_news
        int32 [I, k, top], why_val f32 [I, k, top]).  why_news[i, j] are the ``top`` news of
        impression i's history (rows of the news table) whose clicks contributed most to
        the score of idx[i, j], why_val their contributions (ops.explain_scores: the
        contributions of all clicks add up to the score), value descending; (-1, -inf) for a
        pad and past the history's length.  The lists are retrieved and explained once per
        distinct history (the deduplicated CSR when load_impressions built it) and only
        then expanded to the impressions; the result does not depend on that."""
        return self.recommend_explained_filtered(k, top=top, lam=lam, pool=pool, exclude_history=exclude_history,
                                                 user_block=user_block)

    def recommend_explained_filtered(self, k: int, time_window=None, categories=None, top: int = 3,
                                     lam: Optional[float] = None, pool: int = 64, exclude_history: bool = True,
                                     user_block: Optional[int] = None, prior_gain=None, group_cap=None,
                                     after=None):
        """recommend_explained under recommend's catalogue filters ``time_window`` /
        ``categories``: the filtered lists are expanded to the impressions first and explained
        against each impression's own history.  Without a filter argument it is
        recommend_explained itself.  ``prior_gain`` and ``group_cap`` are refused, the first as in
        explain (recommend_explained does not take either argument at all); ``explain(idx)`` takes
        any lists, recommend's capped ones included."""
        _no_prior("recommend_explained", prior_gain)
        _no_cap("recommend_explained", group_cap)
        _no_cursor("recommend_explained", after=after)
        q = self._queries(time_window, categories)
        if lam is None:
            idx, scores = self._recommend_distinct(int(k), exclude_history, user_block, q)
        else:
            idx, scores, _, _ = self._diverse_distinct(k, lam, pool, exclude_history, user_block, q=q)
        if q is not None:
            idx, scores = idx[q.sel].contiguous(), scores[q.sel].contiguous()
            hidx, hoff = self.hist_idx, self.hist_off
        else:
            hidx, hoff = self._distinct_hist()
        n_u, top = idx.shape[0], int(top)
        if n_u == 0:
            return (idx, scores, torch.empty((0, int(k), top), dtype=torch.int32, device=self.device),
                    torch.empty((0, int(k), top), dtype=torch.float32, device=self.device))
        pos, val = ops.explain_scores(self.pooler, self.hist_table, self.cand_table, self.cand_inv, hidx, hoff, idx,
                                      top=top)
        if hidx.numel():
            row = (hoff[:-1].view(-1, 1, 1) + pos.clamp(min=0)).clamp(max=hidx.numel() - 1)
            why = torch.where(pos >= 0, hidx[row], torch.full_like(pos, -1))
        else:
            why = torch.full_like(pos, -1)
        if q is None and self.user_idx is not None:
            sel = self.user_idx.long()
            idx, scores, why, val = idx[sel], scores[sel], why[sel], val[sel]
        return idx, scores, why, val

    def rank_targets(self, tgt_idx, tgt_len, exclude_history: bool = True, user_block: Optional[int] = None,
                     time_window=None, categories=None, prior_gain=None, group_cap=None):
        """Full-table ranks of given news per impression (ops.rank_targets over the pooled
        users): int32 [T] in the caller's target order, ``tgt_len[i]`` targets (rows of the
        news table, e.g. the clicked candidates) for impression i.  A rank is the number
        of eligible news that beat the target in recommend's order, 0 for the best; -1 for
        a target that is in the impression's own history (with ``exclude_history``) or
        outside the table.  The targets with rank < k are exactly recommend(k)'s rows.
        Distinct histories are pooled once: with the deduplicated CSR the impressions'
        targets are grouped under their distinct user (a stable sort) and the ranks
        scattered back.  ``user_block`` bounds the workspace; the results depend on neither.
        ``time_window`` / ``categories`` (as in recommend) count only the eligible news, and a
        target that its impression's filter leaves out gets -1.  ``prior_gain`` (as in recommend)
        ranks on ``score + g * news_prior`` (ops.rank_targets_prior): the targets with rank < k are
        then recommend(k, prior_gain=...)'s rows."""
        _no_cap("rank_targets", group_cap)
        tgt_idx = np.ascontiguousarray(tgt_idx, dtype=np.int32)
        tgt_len = np.asarray(tgt_len, dtype=np.int64)
        if len(tgt_len) != self.n_imp:
            raise ValueError("Number of rows should be consistent")
        _check_segments(tgt_idx, tgt_len, "target")
        q = self._queries(time_window, categories, prior_gain)
        self.hist_table = self.transform(out=self.hist_table)
        self.inv_norms()
        hidx, hoff = self._distinct_hist()
        prior = q is not None and q.gain is not None
        n_u = hoff.numel() - 1
        n_t = len(tgt_idx)
        ranks = torch.empty(n_t, dtype=torch.int32, device=self.device)
        if n_t == 0 or n_u == 0:
            return ranks
        n_rows = n_u if q is None else q.n  # the rows the kernel sees: distinct histories, or distinct queries
        order = None
        if q is not None or self.user_idx is not None:  # the impressions' targets under their distinct row, in impression order
            owner = np.repeat(q.sel_host if q is not None else self.user_idx.cpu().numpy().astype(np.int64), tgt_len)
            order = np.argsort(owner, kind="stable")
            tgt_idx = tgt_idx[order]
            toff = lengths_to_offsets(np.bincount(owner, minlength=n_rows))
        else:
            toff = lengths_to_offsets(tgt_len)
        users = self._pooled_users(hidx, hoff)
        tidx_d = _upload(tgt_idx, self.device)
        blk = n_rows if not user_block else max(1, min(int(user_block), n_rows))
        n_news = self.cand_table.shape[0]
        most = max(int(toff[min(u0 + blk, n_rows)] - toff[u0]) for u0 in range(0, n_rows, blk))
        need = (ops.rank_targets_prior_workspace_bytes if prior else ops.rank_targets_workspace_bytes)(
            self.dtype, blk, n_news, most)
        self._rank_ws = ops.grow_workspace(getattr(self, "_rank_ws", None), max(need, 256), self.device)
        sorted_ranks = ranks if order is None else torch.empty_like(ranks)
        has_targets = lambda u0, u1: toff[u0] != toff[u1]
        for u0, u1, rows, eidx, eoff, flt in self._blocks(q, users, hidx, hoff, n_rows, blk, exclude_history,
                                                          wanted=has_targets):
            a, b = int(toff[u0]), int(toff[u1])
            (ops.rank_targets_prior if prior else ops.rank_targets_filtered if flt else ops.rank_targets)(
                rows, self.cand_table, self.cand_inv, tidx_d[a:b], _upload(toff[u0:u1 + 1] - a, self.device),
                excl_idx=eidx, excl_off=eoff, out=sorted_ranks[a:b], workspace=self._rank_ws, **flt)
        if order is not None:
            ranks[_upload(order, self.device)] = sorted_ranks
        return ranks

    def _hoff_host(self, hoff: torch.Tensor) -> np.ndarray:
        """Host copy of a history offset array (one read-back per loaded impression set)."""
        cache = getattr(self, "_hoff_cache", None)
        if cache is None or cache[0] is not hoff:
            self._hoff_cache = cache = (hoff, hoff.cpu().numpy())
        return cache[1]

    def rank(self, scores: torch.Tensor) -> torch.Tensor:
        return ops.dense_rank(scores, self.cand_off)
