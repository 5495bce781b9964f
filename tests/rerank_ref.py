"""Reference of the MMR re-ranking (include/newsrec_rerank.h) in numpy, float64 unless a
dtype is given, batched over the users; test support for tests/test_rerank_host.py and
tests/test_rerank_gpu.py.

Shapes: rel [U, M], G [U, M, M] (the similarity matrix: symmetric, diagonal and pads 0),
valid bool [U, M]; a single user may be passed without its leading axis."""
from __future__ import annotations

import numpy as np

D = 1024
PLANT_COLS = np.arange(64) * 16 + 3  # the planted rows' non-zero columns: four in every 256-byte slice of an f32 row


def valid_entries(idx, n_news: int) -> np.ndarray:
    idx = np.asarray(idx)
    return (idx >= 0) & (idx < n_news)


def gram(table, cand_inv, idx) -> np.ndarray:
    """sim(i, j) = (e_i . e_j) inv_i inv_j over the listed table rows, [..., M, M] float64; the
    diagonal and every pad row and column are 0."""
    table = np.asarray(table, dtype=np.float64)
    inv = np.asarray(cand_inv, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    ok = valid_entries(idx, table.shape[0])
    safe = np.where(ok, idx, 0)
    E = table[safe] * (inv[safe] * ok)[..., None]
    G = np.where(ok[..., :, None] & ok[..., None, :], E @ np.swapaxes(E, -1, -2), 0.0)
    m = idx.shape[-1]
    G[..., np.arange(m), np.arange(m)] = 0.0
    return G


def mmr(rel, G, valid, k: int, lam, dtype=np.float64):
    """Greedy MMR, every step evaluated in ``dtype`` as the library does in f32 (two rounded
    products, one rounded difference).  Returns (pos int64 [U, k], -1 where the valid entries
    ran out, gap [U]: the smallest difference between the best and the second-best
    objective over all rounds; inf where no round had two candidates)."""
    rel = np.asarray(rel, dtype=dtype)
    single = rel.ndim == 1
    rel = np.atleast_2d(rel)
    G = np.asarray(G, dtype=dtype).reshape(rel.shape + rel.shape[-1:])
    valid = np.atleast_2d(np.asarray(valid, dtype=bool))
    U, M = rel.shape
    lam = dtype(lam)
    oml = dtype(1) - lam
    left = valid.copy()
    ms = np.full((U, M), -np.inf, dtype=dtype)
    pos = np.full((U, k), -1, dtype=np.int64)
    gap = np.full(U, np.inf)
    rows = np.arange(U)
    for t in range(k):
        with np.errstate(invalid="ignore"):
            obj = rel if t == 0 else lam * rel - oml * ms
        obj = np.where(left, obj, -np.inf)
        p = np.argmax(obj, axis=1)  # the first of equal values: the lower position
        have = left[rows, p]
        if left.shape[1] > 1:
            two = np.sort(obj.astype(np.float64), axis=1)[:, -2:]
            second_live = left.sum(axis=1) >= 2
            with np.errstate(invalid="ignore"):
                g = np.where(second_live, two[:, 1] - two[:, 0], np.inf)
            gap = np.minimum(gap, g)
        pos[have, t] = p[have]
        left[rows[have], p[have]] = False
        ms = np.where(have[:, None], np.maximum(ms, G[rows, :, p]), ms)
    return (pos[0], float(gap[0])) if single else (pos, gap)


def check_valid_greedy(pos, rel, G, valid, lam, eps: float) -> float:
    """Replay the library's OWN picks ``pos`` [U, k]: at every round the pick must be a valid
    entry not picked before whose float64 objective is within ``eps`` of the float64
    maximum over the remaining entries, and a -1 may only stand where none remains.
    Returns the largest deficit seen."""
    rel = np.atleast_2d(np.asarray(rel, dtype=np.float64))
    pos = np.atleast_2d(np.asarray(pos, dtype=np.int64))
    valid = np.atleast_2d(np.asarray(valid, dtype=bool))
    U, M = rel.shape
    G = np.asarray(G, dtype=np.float64).reshape(U, M, M)
    left = valid.copy()
    ms = np.full((U, M), -np.inf)
    rows = np.arange(U)
    worst = 0.0
    for t in range(pos.shape[1]):
        p = pos[:, t]
        have = left.any(axis=1)
        assert ((p >= 0) == have).all(), f"round {t}: a pick is missing or stands where no entry remains"
        assert (p < M).all()
        ps = np.where(have, p, 0)
        assert left[rows, ps][have].all(), f"round {t}: a pad or an entry picked before was picked"
        with np.errstate(invalid="ignore"):
            obj = rel if t == 0 else lam * rel - (1.0 - lam) * ms
        obj = np.where(left, obj, -np.inf)
        with np.errstate(invalid="ignore"):  # (-inf) - (-inf) of a user with nothing left
            deficit = np.where(have, obj.max(axis=1) - obj[rows, ps], 0.0)
        worst = max(worst, float(deficit.max()))
        assert (deficit <= eps).all(), f"round {t}: a pick lies {deficit.max():.3e} below the best objective (eps {eps:.1e})"
        left[rows[have], ps[have]] = False
        ms = np.where(have[:, None], np.maximum(ms, G[rows, :, ps]), ms)
    return worst


def ild(G, members) -> float:
    """Mean over pairs of 1 - sim among the positions ``members`` of one user's list (0 below two)."""
    m = np.asarray([p for p in members if p >= 0], dtype=np.int64)
    if len(m) < 2:
        return 0.0
    sub = 1.0 - np.asarray(G, dtype=np.float64)[np.ix_(m, m)]
    iu = np.triu_indices(len(m), 1)
    return float(sub[iu].mean())


def brute_force(rel, G, valid, k: int, lam):
    """One user in plain Python floats (float64), no numpy in the selection."""
    rel = [float(v) for v in rel]
    M = len(rel)
    chosen, out = [], []
    for t in range(k):
        best, at = None, -1
        for i in range(M):
            if not valid[i] or i in chosen:
                continue
            if t == 0:
                obj = rel[i]
            else:
                obj = lam * rel[i] - (1.0 - lam) * max(float(G[i][j]) for j in chosen)
            if best is None or obj > best:
                best, at = obj, i
        out.append(at)
        if at >= 0:
            chosen.append(at)
    return out


def planted(rng, n_news: int, n_users: int, m: int):
    """Inputs on which every product, sum and objective is exact in f32 and in bf16: table
    rows with exactly 16 non-zeros of +-1 among the 64 columns PLANT_COLS (norm 4, inverse
    norm 0.25, every cosine a multiple of 1/16) and relevances that are multiples of 1/64
    drawn from 24 values, so that ties occur.  Returns (table f32 [N, D], inv f32 [N],
    list_idx int32 [U, M] -- distinct rows per user --, list_rel f32 [U, M])."""
    table = np.zeros((n_news, D), dtype=np.float32)
    for r in range(n_news):
        cols = rng.choice(PLANT_COLS, 16, replace=False)
        table[r, cols] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), 16)
    inv = np.full(n_news, 0.25, dtype=np.float32)
    return (table, inv) + planted_lists(rng, n_news, n_users, m)


def planted_lists(rng, n_news: int, n_users: int, m: int):
    """Lists over a planted table: (list_idx int32 [U, M], list_rel f32 [U, M])."""
    idx = np.stack([rng.choice(n_news, m, replace=False) for _ in range(n_users)]).astype(np.int32)
    rel = (rng.integers(0, 24, (n_users, m)) / 64.0).astype(np.float32)
    return idx, rel
