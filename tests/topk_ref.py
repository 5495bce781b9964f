"""CPU reference (test support) of top-K retrieval (include/newsrec_topk.h), in
float64 numpy.  Its tie and exclusion rules are exactly the contract's:

  * score descending, equal scores by ascending row;
  * rows in a user's exclusion list are left out (duplicates allowed, entries
    outside [0, N) ignored);
  * fewer than K eligible rows: the tail is (idx -1, score -inf);
  * a zero user (|u| < 1e-8) scores 0 everywhere: the first K eligible rows.
"""
from __future__ import annotations

import numpy as np


def cosine_scores(users, table, cand_inv=None) -> np.ndarray:
    """[U, N] float64 cosine scores of the operands as given (round them first for the
    bf16 mode).  ``cand_inv`` (the evaluation path's f32 1 / max(|e_c|, 1e-8)) is used as
    given when passed, else computed in float64."""
    u = np.asarray(users, dtype=np.float64)
    e = np.asarray(table, dtype=np.float64)
    un = np.sqrt((u * u).sum(1))
    ci = (1.0 / np.maximum(np.sqrt((e * e).sum(1)), 1e-8) if cand_inv is None
          else np.asarray(cand_inv, dtype=np.float64))
    s = (u @ e.T) / np.maximum(un, 1e-8)[:, None] * ci[None, :]
    s[un < 1e-8] = 0.0
    return s


def topk(scores, k: int, excl_idx=None, excl_off=None):
    """(idx int32 [U, k], scores float64 [U, k]) of a [U, N] score matrix."""
    s = np.asarray(scores, dtype=np.float64)
    U, N = s.shape
    idx = np.full((U, k), -1, dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    rows = np.arange(N)
    for u in range(U):
        ok = np.ones(N, dtype=bool)
        if excl_idx is not None:
            e = np.asarray(excl_idx[int(excl_off[u]):int(excl_off[u + 1])], dtype=np.int64)
            e = e[(e >= 0) & (e < N)]
            ok[e] = False
        elig = rows[ok]
        # lexsort: last key is primary -> (-score, row)
        order = elig[np.lexsort((elig, -s[u, elig]))][:k]
        idx[u, :len(order)] = order
        out[u, :len(order)] = s[u, order]
    return idx, out


def brute_force(scores, k: int, excl_idx=None, excl_off=None):
    """The same by a plain Python full sort of (−score, row) tuples."""
    s = np.asarray(scores, dtype=np.float64)
    U, N = s.shape
    idx = np.full((U, k), -1, dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    for u in range(U):
        banned = set()
        if excl_idx is not None:
            banned = {int(r) for r in excl_idx[int(excl_off[u]):int(excl_off[u + 1])]}
        pairs = sorted((-float(s[u, r]), r) for r in range(N) if r not in banned)
        for j, (neg, r) in enumerate(pairs[:k]):
            idx[u, j], out[u, j] = r, -neg
    return idx, out
