"""CPU reference (test support) of the catalogue filters (include/newsrec_filter.h), in
numpy over float64 score matrices.  It holds the eligibility predicate and the helper
that turns a filter into the equivalent exclusion lists; top-K and ranks themselves are
tests/topk_ref.py's and tests/fullrank_ref.py's, run on those lists.

  * row c is eligible for user u when lo[u] <= news_time[c] <= hi[u] (both inclusive;
    lo > hi is an empty window) and news_cat[c] < 64 and bit news_cat[c] of mask[u] is set;
  * a pair that is None passes every row;
  * a user's exclusion list is applied on top.
"""
from __future__ import annotations

import numpy as np

import fullrank_ref
import topk_ref


def eligible(n_users: int, n_news: int, news_time=None, lo=None, hi=None, news_cat=None, mask=None) -> np.ndarray:
    """bool [U, N]: the window and the category mask (not the exclusion lists)."""
    ok = np.ones((n_users, n_news), dtype=bool)
    if news_time is not None:
        t = np.asarray(news_time, dtype=np.int64)[None, :]
        ok &= (t >= np.asarray(lo, dtype=np.int64)[:, None]) & (t <= np.asarray(hi, dtype=np.int64)[:, None])
    if news_cat is not None:
        c = np.asarray(news_cat, dtype=np.int64)[None, :]
        m = np.asarray(mask).astype(np.uint64)[:, None]
        bit = (m >> np.minimum(c, 63).astype(np.uint64)) & np.uint64(1)
        ok &= (c < 64) & (bit != 0)
    return ok


def eligible_brute(n_users, n_news, news_time=None, lo=None, hi=None, news_cat=None, mask=None) -> np.ndarray:
    """The same, one (user, row) pair at a time in Python integers."""
    ok = np.ones((n_users, n_news), dtype=bool)
    for u in range(n_users):
        for c in range(n_news):
            if news_time is not None and not (int(lo[u]) <= int(news_time[c]) <= int(hi[u])):
                ok[u, c] = False
            if news_cat is not None:
                cat = int(news_cat[c])
                m = int(mask[u]) & 0xFFFFFFFFFFFFFFFF
                if cat >= 64 or not (m >> cat) & 1:
                    ok[u, c] = False
    return ok


def as_exclusions(elig: np.ndarray, excl_idx=None, excl_off=None):
    """(idx int32, off int64 [U + 1]): each user's own exclusion list followed by its
    ineligible rows in row order -- the unfiltered call that a filtered call must equal."""
    U = elig.shape[0]
    parts = []
    for u in range(U):
        own = (np.asarray(excl_idx[int(excl_off[u]):int(excl_off[u + 1])], dtype=np.int32)
               if excl_idx is not None else np.zeros(0, np.int32))
        parts.append(np.concatenate([own, np.nonzero(~elig[u])[0].astype(np.int32)]))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    idx = np.concatenate(parts).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return idx, off


def topk(scores, k: int, elig: np.ndarray, excl_idx=None, excl_off=None):
    return topk_ref.topk(scores, k, *as_exclusions(elig, excl_idx, excl_off))


def rank_targets(scores, tgt_idx, tgt_off, elig: np.ndarray, excl_idx=None, excl_off=None) -> np.ndarray:
    return fullrank_ref.rank_targets(scores, tgt_idx, tgt_off, *as_exclusions(elig, excl_idx, excl_off))
