"""CPU reference (test support) of retrieval under a rank-one prior
(include/newsrec_prior.h), in float64 numpy: tests/topk_ref.py's top-K over the keys

    key(u, c) = cos(u, c) + gain[u] * prior[c]

with its tie, exclusion and short-row rules, plus a brute-force check of itself.  The
returned scores are the cosines of the listed rows, the keys what they are ordered by.
"""
from __future__ import annotations

import numpy as np

import topk_ref


def keys(scores, gain, prior) -> np.ndarray:
    """[U, N] float64 keys of a [U, N] score matrix."""
    s = np.asarray(scores, dtype=np.float64)
    return s + np.asarray(gain, dtype=np.float64)[:, None] * np.asarray(prior, dtype=np.float64)[None, :]


def topk(scores, k: int, gain, prior, excl_idx=None, excl_off=None, eligible=None):
    """(idx int32 [U, k], scores float64 [U, k], keys float64 [U, k]); ``eligible`` bool [U, N]
    (None: every row) leaves rows out as an exclusion list does."""
    s = np.asarray(scores, dtype=np.float64)
    ky = keys(s, gain, prior)
    if eligible is not None:
        ky = np.where(eligible, ky, -np.inf)
    idx, kk = topk_ref.topk(ky, k, excl_idx, excl_off)
    if eligible is not None:  # an ineligible row sorts last but is still a row to topk_ref: drop it
        gone = np.isneginf(kk)
        idx[gone] = -1
    sc = np.where(idx >= 0, np.take_along_axis(s, np.maximum(idx, 0).astype(np.int64), axis=1), -np.inf)
    return idx, sc, kk


def brute_force(scores, k: int, gain, prior, excl_idx=None, excl_off=None, eligible=None):
    """The same by a plain Python sort of (-key, row) tuples."""
    s = np.asarray(scores, dtype=np.float64)
    U, N = s.shape
    idx = np.full((U, k), -1, dtype=np.int32)
    sc = np.full((U, k), -np.inf)
    kk = np.full((U, k), -np.inf)
    for u in range(U):
        banned = set()
        if excl_idx is not None:
            banned = {int(r) for r in excl_idx[int(excl_off[u]):int(excl_off[u + 1])]}
        rows = [r for r in range(N) if r not in banned and (eligible is None or eligible[u, r])]
        pairs = sorted((-(float(s[u, r]) + float(gain[u]) * float(prior[r])), r) for r in rows)
        for j, (neg, r) in enumerate(pairs[:k]):
            idx[u, j], sc[u, j], kk[u, j] = r, s[u, r], -neg
    return idx, sc, kk
