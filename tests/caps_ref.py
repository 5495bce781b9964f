"""CPU reference (test support) of top-K retrieval under per-group caps
(include/newsrec_caps.h), in float64 numpy.

The rule: walk a user's eligible rows in the strict total order (key descending, row
ascending); take a row if and only if fewer than ``cap`` rows of its group have been taken;
stop at K.  ``capped_topk`` is that walk.  ``brute_force`` knows nothing of the walk: it
enumerates every feasible subset (at most K rows, at most ``cap`` per group) and keeps the
one whose sorted tuple of order positions is lexicographically smallest, a missing slot
counting as +inf -- the optimum of the partition matroid truncated at K that the greedy walk
is claimed to reach.  Eligibility: ``eligible`` bool [U, N] (None: all), and the exclusion CSR
of tests/topk_ref.py (duplicates allowed, entries outside [0, N) ignored).
"""
from __future__ import annotations

from itertools import combinations

import numpy as np


def _ok_rows(u, N, eligible, excl_idx, excl_off) -> np.ndarray:
    ok = np.ones(N, dtype=bool) if eligible is None else np.asarray(eligible[u], dtype=bool).copy()
    if excl_idx is not None:
        e = np.asarray(excl_idx[int(excl_off[u]):int(excl_off[u + 1])], dtype=np.int64)
        e = e[(e >= 0) & (e < N)]
        ok[e] = False
    return ok


def order_of(keys_row, ok) -> np.ndarray:
    """The eligible rows, best first: (key descending, row ascending)."""
    elig = np.nonzero(ok)[0]
    return elig[np.lexsort((elig, -np.asarray(keys_row, dtype=np.float64)[elig]))]


def capped_topk(keys, k: int, groups, cap: int, eligible=None, excl_idx=None, excl_off=None):
    """(idx int32 [U, k], keys float64 [U, k]) of a [U, N] key matrix; pads are (-1, -inf)."""
    s = np.asarray(keys, dtype=np.float64)
    g = np.asarray(groups, dtype=np.int64)
    U, N = s.shape
    idx = np.full((U, k), -1, dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    for u in range(U):
        held: dict = {}
        n = 0
        for r in order_of(s[u], _ok_rows(u, N, eligible, excl_idx, excl_off)):
            if n == k:
                break
            if held.get(int(g[r]), 0) >= cap:
                continue
            held[int(g[r])] = held.get(int(g[r]), 0) + 1
            idx[u, n], out[u, n] = r, s[u, r]
            n += 1
    return idx, out


def brute_force(keys, k: int, groups, cap: int, eligible=None, excl_idx=None, excl_off=None):
    """The same by enumeration of all subsets of at most k eligible rows (tiny N only)."""
    s = np.asarray(keys, dtype=np.float64)
    g = np.asarray(groups, dtype=np.int64)
    U, N = s.shape
    idx = np.full((U, k), -1, dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    for u in range(U):
        order = order_of(s[u], _ok_rows(u, N, eligible, excl_idx, excl_off))
        best, best_sig = (), (np.inf,) * k
        for size in range(1, min(k, len(order)) + 1):
            for pos in combinations(range(len(order)), size):  # positions in the order, ascending
                if max(np.bincount(g[order[list(pos)]])) > cap:
                    continue
                sig = tuple(pos) + (np.inf,) * (k - size)
                if sig < best_sig:
                    best, best_sig = pos, sig
        rows = order[list(best)] if len(best) else np.zeros(0, np.int64)
        idx[u, :len(rows)] = rows
        out[u, :len(rows)] = s[u, rows]
    return idx, out
