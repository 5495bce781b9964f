"""CPU reference (test support) of cursors for top-K retrieval (include/newsrec_page.h), in
float64 numpy on top of tests/topk_ref.py, whose order it reuses: score descending, equal
scores by ascending row.  A row r with score s is eligible behind the cursor (key, row) only
if ``key > s or (key == s and row < r)``; (+inf, -1) is the start of the list, (-inf,
INT32_MAX) its end, a NaN key makes nothing eligible.  In the reference the selection key of
a row is its score."""
from __future__ import annotations

import numpy as np

import topk_ref

START = (np.inf, -1)
END = (-np.inf, np.iinfo(np.int32).max)


def topk_after(scores, k: int, after_key=None, after_row=None, excl_idx=None, excl_off=None):
    """(idx int32 [U, k], scores float64 [U, k], (next_key float64 [U], next_row int32 [U])):
    the k best eligible rows behind each user's cursor (None: the start) and the cursor behind
    the last of them, the end cursor where fewer than k were left."""
    s = np.asarray(scores, dtype=np.float64)
    U, N = s.shape
    ak = np.full(U, START[0]) if after_key is None else np.asarray(after_key, dtype=np.float64)
    ar = np.full(U, START[1], dtype=np.int64) if after_row is None else np.asarray(after_row, dtype=np.int64)
    rows = np.arange(N)
    lists = []
    for u in range(U):
        behind = (ak[u] > s[u]) | ((ak[u] == s[u]) & (ar[u] < rows))
        out = rows[~behind]
        if excl_idx is not None:
            out = np.concatenate([out, np.asarray(excl_idx[int(excl_off[u]):int(excl_off[u + 1])], dtype=np.int64)])
        lists.append(out)
    eoff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    eidx = np.concatenate(lists).astype(np.int64) if eoff[-1] else np.zeros(0, np.int64)
    idx, top = topk_ref.topk(s, k, eidx, eoff)
    full = idx[:, k - 1] >= 0
    next_key = np.where(full, top[:, k - 1], END[0])
    next_row = np.where(full, idx[:, k - 1], END[1]).astype(np.int32)
    return idx, top, (next_key, next_row)


def pages(scores, k: int, n_pages: int, excl_idx=None, excl_off=None):
    """``n_pages`` consecutive pages of k rows from the start: (idx [U, n_pages * k], scores)."""
    cur, idx, top = (None, None), [], []
    for _ in range(n_pages):
        i, t, cur = topk_after(scores, k, cur[0], cur[1], excl_idx, excl_off)
        idx.append(i)
        top.append(t)
    return np.concatenate(idx, axis=1), np.concatenate(top, axis=1)
