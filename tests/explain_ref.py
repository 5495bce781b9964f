"""Float64 reference of the per-click attribution contract (include/newsrec_explain.h),
from the same stored operands the kernel reads (a bf16 table is passed in upcast, cand_inv
as the evaluation path computes it); test support for tests/test_explain_host.py and
tests/test_explain_gpu.py."""
from __future__ import annotations

import numpy as np

D = 1024
TOP_MAX = 8


def valid_entries(lst, n_news: int) -> np.ndarray:
    lst = np.asarray(lst)
    return (lst >= 0) & (lst < n_news)


def shares(pooler: str, rows: np.ndarray):
    """(g [H, D], u [D]) of one history's table rows [H, D or 2 D] in float64: the share
    rows and their sum, the pooled user."""
    rows = np.asarray(rows, dtype=np.float64)
    h = len(rows)
    if pooler == "final":
        x, p = rows[:, :D], rows[:, D:2 * D]
        g = x * p / (p.sum(axis=0) + 1e-10)
    elif pooler == "mean":
        g = rows[:, :D] / h
    elif pooler == "latent":
        m = rows[:, :D].sum(axis=0) / h
        g = rows[:, :D] / (h * max(float(np.linalg.norm(m)), 1e-12))
    else:
        raise ValueError(pooler)
    return g, g.sum(axis=0)


def contributions(pooler: str, hist_table, cand_table, cand_inv, hist, lst):
    """One user: (a [H, K], mass [H, K], valid [K]); a[h][j] the contribution of click h to
    list entry j, mass[h][j] = sum_d |term_d| its absolute mass; a pad's column is 0."""
    hist, lst = np.asarray(hist, dtype=np.int64), np.asarray(lst, dtype=np.int64)
    valid = valid_entries(lst, len(cand_table))
    a = np.zeros((len(hist), len(lst)))
    mass = np.zeros_like(a)
    if len(hist) == 0 or not valid.any():
        return a, mass, valid
    g, u = shares(pooler, np.asarray(hist_table)[hist])
    e = np.asarray(cand_table, dtype=np.float64)[lst[valid]]
    scale = np.asarray(cand_inv, dtype=np.float64)[lst[valid]] / max(float(np.linalg.norm(u)), 1e-8)
    # one product per distinct news: its occurrences share a share row, and so a contribution,
    # to the last bit (a BLAS product's bits may depend on the row's place)
    _, first, inv = np.unique(hist, return_index=True, return_inverse=True)
    a[:, valid] = ((g[first] @ e.T) * scale)[inv]
    mass[:, valid] = ((np.abs(g[first]) @ np.abs(e).T) * scale)[inv]
    return a, mass, valid


def top_t(col: np.ndarray, hist, t: int):
    """Top-t of one column under the contract's order (value descending, equal values by
    ascending position): (pos [t], val [t], gaps [t]); the tail is (-1, -inf).  gaps[i] is
    the difference between the i-th and the (i+1)-th entry of that order, inf where there is
    no (i+1)-th entry or where both are occurrences of one news (bit-identical on the
    device, so the tie rule decides)."""
    col, hist = np.asarray(col, dtype=np.float64), np.asarray(hist)
    order = np.lexsort((np.arange(len(col)), -col))[:t + 1]
    pos = np.full(t, -1, dtype=np.int32)
    val = np.full(t, -np.inf)
    gaps = np.full(t, np.inf)
    n = min(t, len(order))
    pos[:n], val[:n] = order[:n], col[order[:n]]
    for i in range(min(t, len(order) - 1)):
        if hist[order[i]] != hist[order[i + 1]]:
            gaps[i] = col[order[i]] - col[order[i + 1]]
    return pos, val, gaps


def explain(pooler: str, hist_table, cand_table, cand_inv, hist_idx, hist_off, list_idx, top: int = TOP_MAX):
    """Batched over the users: dict of a [n_hist, K], mass [n_hist, K], valid [U, K], sums
    [U, K], top_pos int32 [U, K, top], top_val [U, K, top], gaps [U, K, top]."""
    hist_idx, hist_off, list_idx = np.asarray(hist_idx), np.asarray(hist_off), np.asarray(list_idx)
    n_users, k = list_idx.shape
    out = {"a": np.zeros((len(hist_idx), k)), "mass": np.zeros((len(hist_idx), k)),
           "valid": np.zeros((n_users, k), bool), "sums": np.zeros((n_users, k)),
           "top_pos": np.full((n_users, k, top), -1, dtype=np.int32), "top_val": np.full((n_users, k, top), -np.inf),
           "gaps": np.full((n_users, k, top), np.inf)}
    for u in range(n_users):
        h0, h1 = int(hist_off[u]), int(hist_off[u + 1])
        hist = hist_idx[h0:h1]
        a, mass, valid = contributions(pooler, hist_table, cand_table, cand_inv, hist, list_idx[u])
        out["a"][h0:h1], out["mass"][h0:h1], out["valid"][u] = a, mass, valid
        out["sums"][u] = a.sum(axis=0)
        if h1 > h0:
            for j in np.nonzero(valid)[0]:
                out["top_pos"][u, j], out["top_val"][u, j], out["gaps"][u, j] = top_t(a[:, j], hist, top)
    return out
