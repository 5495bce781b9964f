"""CPU reference (test support) of the full-table ranks (include/newsrec_fullrank.h), in
float64 numpy, over a [U, N] score matrix as tests/topk_ref.py's cosine_scores gives it.
Its rules are exactly the contract's:

  * rank = the number of eligible rows c != t with (score descending, row ascending)
    before the target t: 0 for the best row;
  * rows in a user's exclusion list are not eligible (duplicates allowed, entries
    outside [0, N) ignored);
  * a target that is itself excluded or outside [0, N) gets -1;
  * duplicate targets each get their own (equal) answer; a user may have none;
  * a zero user scores 0 everywhere: rank = the number of eligible rows below the target.
"""
from __future__ import annotations

import numpy as np

from topk_ref import cosine_scores  # noqa: F401  (the scores both references rank)


def _eligible(N, u, excl_idx, excl_off) -> np.ndarray:
    ok = np.ones(N, dtype=bool)
    if excl_idx is not None:
        e = np.asarray(excl_idx[int(excl_off[u]):int(excl_off[u + 1])], dtype=np.int64)
        ok[e[(e >= 0) & (e < N)]] = False
    return ok


def rank_targets(scores, tgt_idx, tgt_off, excl_idx=None, excl_off=None) -> np.ndarray:
    """int32 [T] ranks of tgt_idx[tgt_off[u]:tgt_off[u + 1]] under user u's scores."""
    s = np.asarray(scores, dtype=np.float64)
    U, N = s.shape
    out = np.full(len(tgt_idx), -1, dtype=np.int32)
    rows = np.arange(N)
    for u in range(U):
        ok = _eligible(N, u, excl_idx, excl_off)
        for j in range(int(tgt_off[u]), int(tgt_off[u + 1])):
            t = int(tgt_idx[j])
            if t < 0 or t >= N or not ok[t]:
                continue
            out[j] = int((ok & ((s[u] > s[u, t]) | ((s[u] == s[u, t]) & (rows < t)))).sum())
    return out


def brute_force(scores, tgt_idx, tgt_off, excl_idx=None, excl_off=None) -> np.ndarray:
    """The same by a plain Python full sort of (-score, row) tuples: a target's rank is
    its position in the sorted list of the eligible rows."""
    s = np.asarray(scores, dtype=np.float64)
    U, N = s.shape
    out = np.full(len(tgt_idx), -1, dtype=np.int32)
    for u in range(U):
        banned = set()
        if excl_idx is not None:
            banned = {int(r) for r in excl_idx[int(excl_off[u]):int(excl_off[u + 1])]}
        order = sorted((-float(s[u, r]), r) for r in range(N) if r not in banned)
        place = {r: i for i, (_, r) in enumerate(order)}
        for j in range(int(tgt_off[u]), int(tgt_off[u + 1])):
            out[j] = place.get(int(tgt_idx[j]), -1)
    return out
