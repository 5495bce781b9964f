"""CPU reference (test support) of the sectioned top-K (include/newsrec_sections.h), in
numpy over float64 score matrices: per section, tests/filter_ref.py's top-K with that
section's mask for every user.  ``topk_brute`` is the same in plain Python, one (user,
section) at a time."""
from __future__ import annotations

import numpy as np

import filter_ref


def topk(scores, k: int, sec_masks, news_cat, news_time=None, lo=None, hi=None, excl_idx=None, excl_off=None):
    """(idx int64 [U, S, k], scores float64 [U, S, k]); a short section ends in (-1, -inf)."""
    U, N = scores.shape
    idx = np.full((U, len(sec_masks), k), -1, dtype=np.int64)
    sc = np.full((U, len(sec_masks), k), -np.inf)
    for s, m in enumerate(sec_masks):
        mask = np.full(U, int(m) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        elig = filter_ref.eligible(U, N, news_time, lo, hi, news_cat, mask)
        idx[:, s], sc[:, s] = filter_ref.topk(scores, k, elig, excl_idx, excl_off)
    return idx, sc


def topk_brute(scores, k: int, sec_masks, news_cat, news_time=None, lo=None, hi=None, excl_idx=None, excl_off=None):
    U, N = scores.shape
    idx = np.full((U, len(sec_masks), k), -1, dtype=np.int64)
    sc = np.full((U, len(sec_masks), k), -np.inf)
    for u in range(U):
        banned = set() if excl_idx is None else {int(r) for r in excl_idx[int(excl_off[u]):int(excl_off[u + 1])]}
        for s, m in enumerate(sec_masks):
            m = int(m) & 0xFFFFFFFFFFFFFFFF
            rows = []
            for r in range(N):
                cat = int(news_cat[r])
                if r in banned or cat >= 64 or not (m >> cat) & 1:
                    continue
                if news_time is not None and not int(lo[u]) <= int(news_time[r]) <= int(hi[u]):
                    continue
                rows.append((-float(scores[u, r]), r))
            for j, (neg, r) in enumerate(sorted(rows)[:k]):
                idx[u, s, j], sc[u, s, j] = r, -neg
    return idx, sc
