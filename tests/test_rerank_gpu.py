"""MMR re-ranking (csrc/rerank.hip, include/newsrec_rerank.h) on the GPU against the
float64 reference of tests/rerank_ref.py.

Bounds.  SIM_EPS = 1e-4 on the cosine scale is the project's f32 cosine contract (the
worst-case f32 accumulation bound of a 1024-term dot product, tests/test_topk_gpu.py);
in bf16 mode the reference is the float64 matrix of the SAME operands (the bf16 table
upcast, cand_inv as the evaluation path computes it), so the same bound holds.  An
objective difference involves two similarities, each within SIM_EPS, weighted 1 - lambda:
check_valid_greedy's eps is 2 (1 - lambda) SIM_EPS.

Exact lists.  SIM_ERR_MEASURED is the largest |sim_out - float64| over the random-table
inputs of this file, both dtypes and every case of RANDOM_CASES, measured on an MI355X
(printed by test_gpu_rerank_random_everybody_checked); EPS_EXACT = 4 x that (two
similarities per objective difference and a factor 2 of headroom) is the reference gap
above which a user's list must equal the reference's.  It must stay below EPS_EXACT_CAP =
2e-5: a larger error means the accumulation is wrong.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import rerank_ref
from news_recommendation_project_v2_amd import weights as W
from retrieval_cases import _model

D = 1024
N_NEWS = 3000
SIM_EPS = 1e-4
SIM_ERR_MEASURED = 1.96e-7
EPS_EXACT = 4 * SIM_ERR_MEASURED
EPS_EXACT_CAP = 2e-5
MAX_LEFT_OUT = 0.15
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
INVALID, UNSUPPORTED = -1, -3


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _run(table, inv, idx, rel, k, lam, **kw):
    """ops.rerank_mmr with every output, as numpy: (idx, rel, pos, ild, sim)."""
    from news_recommendation_project_v2_amd import ops
    dev = table.device
    out = ops.rerank_mmr(table, inv, torch.as_tensor(idx).to(dev), torch.as_tensor(rel).to(dev), k, lam, want_pos=True,
                         want_ild=True, want_sim=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------ 1. planted, exact
_PLANTED = {}


def _planted_table(dtype, dev):
    if "host" not in _PLANTED:
        _PLANTED["host"] = rerank_ref.planted(np.random.default_rng(21), N_NEWS, 1, 1)[:2]
    if dtype not in _PLANTED:
        table, inv = _PLANTED["host"]
        _PLANTED[dtype] = (torch.from_numpy(table).to(dev).to(dtype).contiguous(), torch.from_numpy(inv).to(dev))
    return _PLANTED["host"] + _PLANTED[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 33, 64])
@pytest.mark.parametrize("n_users", [1, 3, 1031])
def test_gpu_rerank_planted_exact(gpu_device, n_users, m, dtype):
    """Every product, sum and objective is exact: idx, pos, rel and sim_out equal the float64
    reference for EVERY user, ties included (tests/test_rerank_host.py shows the f32 and
    float64 evaluations of this construction agree)."""
    table_h, inv_h, table, inv = _planted_table(dtype, gpu_device)
    rng = np.random.default_rng(1000 * n_users + m)
    idx, rel = rerank_ref.planted_lists(rng, N_NEWS, n_users, m)
    G = rerank_ref.gram(table_h[:, rerank_ref.PLANT_COLS], inv_h, idx)  # (every other column is zero)
    valid = np.ones(idx.shape, bool)
    rows = np.arange(n_users)[:, None]
    ties = 0
    for k in sorted({1, min(10, m), m}):
        for lam in (0.25, 0.5, 0.75):
            gi, gr, gp, gild, gsim = _run(table, inv, idx, rel, k, lam)
            pos, gap = rerank_ref.mmr(rel, G, valid, k, lam)
            ties += int((gap == 0.0).sum())
            assert np.array_equal(gp, pos), (k, lam)
            assert np.array_equal(gi, idx[rows, pos]) and np.array_equal(_bits(gr), _bits(rel[rows, pos])), (k, lam)
            assert np.array_equal(_bits(gsim), _bits(G.astype(np.float32) + 0.0)), "sim_out differs from the reference"
            for u in (0, n_users - 1):  # exact here too: sums of multiples of 1/16 below 2^11
                n = min(k, m)
                want = [rerank_ref.ild(G[u], range(n)), rerank_ref.ild(G[u], pos[u])]
                assert np.allclose(gild[u], want, rtol=0, atol=1e-6), (k, lam, gild[u], want)
    if n_users * m >= 1031 * 15:
        assert ties > 0, "the planted lists are meant to contain exact ties"


# ------------------------------------------------------------------ 2, 3. random table
RANDOM_CASES = [(64, 10, 0.7), (64, 10, 0.3), (33, 16, 0.5), (17, 5, 0.5), (64, 64, 0.5)]
EXACT_CASES = RANDOM_CASES[:4]  # (at K = M = 64 every user falls out of the gap rule)
_RANDOM = {}


def _random_inputs(dtype, dev):
    """N(0, 1) table; 300 users, each the normalised mean of 20 random table rows."""
    from news_recommendation_project_v2_amd import ops
    if "host" not in _RANDOM:
        rng = np.random.default_rng(22)
        table = rng.standard_normal((N_NEWS, D)).astype(np.float32)
        users = np.stack([table[rng.choice(N_NEWS, 20, replace=False)].mean(axis=0) for _ in range(300)])
        _RANDOM["host"] = (table, (users / np.linalg.norm(users, axis=1, keepdims=True)).astype(np.float32))
    if dtype not in _RANDOM:
        table_h, users_h = _RANDOM["host"]
        table = torch.from_numpy(table_h).to(dev).to(dtype).contiguous()
        inv = ops.row_inv_norm(table, 1e-8)
        _RANDOM[dtype] = (table, inv, torch.from_numpy(users_h).to(dev), table.double().cpu().numpy(),
                          inv.double().cpu().numpy())
    return _RANDOM[dtype]


def _random_lists(dtype, dev, m):
    """(list_idx, list_rel) from ops.topk_users and the float64 matrix of the same operands."""
    from news_recommendation_project_v2_amd import ops
    key = (dtype, m, "lists")
    if key not in _RANDOM:
        table, inv, users, table64, inv64 = _random_inputs(dtype, dev)
        idx, rel = ops.topk_users(users, table, inv, m)
        torch.cuda.synchronize()
        idx, rel = idx.cpu().numpy(), rel.cpu().numpy()
        _RANDOM[key] = (idx, rel, rerank_ref.gram(table64, inv64, idx))
    return _RANDOM[key]


def _random_run(dtype, dev, case):
    key = (dtype, case)
    if key not in _RANDOM:
        m, k, lam = case
        table, inv = _random_inputs(dtype, dev)[:2]
        idx, rel, G = _random_lists(dtype, dev, m)
        _RANDOM[key] = _run(table, inv, idx, rel, k, lam)
    return _RANDOM[key]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "M%d-K%d-lam%g" % c)
def test_gpu_rerank_random_everybody_checked(gpu_device, case, dtype):
    m, k, lam = case
    idx, rel, G = _random_lists(dtype, gpu_device, m)
    gi, gr, gp, gild, gsim = _random_run(dtype, gpu_device, case)
    valid = np.ones(idx.shape, bool)
    err = float(np.abs(gsim.astype(np.float64) - G).max())
    print(f"max |sim_out - float64| = {err:.3e} (SIM_ERR_MEASURED {SIM_ERR_MEASURED:.1e}, contract {SIM_EPS:.0e})")
    assert err <= SIM_EPS
    assert np.array_equal(_bits(gsim), _bits(np.swapaxes(gsim, 1, 2))), "sim_out is not symmetric bit for bit"
    assert not gsim[:, np.arange(m), np.arange(m)].any()
    worst = rerank_ref.check_valid_greedy(gp, rel, G, valid, lam, 2 * (1 - lam) * SIM_EPS)
    print(f"largest deficit of a pick below the float64 best objective: {worst:.3e}")
    rows = np.arange(len(idx))[:, None]
    assert np.array_equal(gi, idx[rows, gp]) and np.array_equal(_bits(gr), _bits(rel[rows, gp]))
    want = np.array([[rerank_ref.ild(G[u], range(k)), rerank_ref.ild(G[u], gp[u])] for u in range(len(idx))])
    ild_err = float(np.abs(gild - want).max())
    print(f"max |out_ild - reference on the library's picks| = {ild_err:.3e}")
    assert ild_err <= SIM_EPS


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "M%d-K%d-lam%g" % c)
def test_gpu_rerank_random_exact_lists(gpu_device, case, dtype):
    """Every user whose reference gap (best minus second-best objective, smallest over the
    rounds) exceeds EPS_EXACT gets exactly the reference's list; at most 15 % may fall out."""
    assert EPS_EXACT <= EPS_EXACT_CAP
    m, k, lam = case
    idx, rel, G = _random_lists(dtype, gpu_device, m)
    run = _random_run(dtype, gpu_device, case)
    gp = run[2]
    err = float(np.abs(run[4].astype(np.float64) - G).max())
    assert err <= EPS_EXACT / 2, f"|sim_out - float64| = {err:.3e}: EPS_EXACT no longer covers two similarities"
    pos, gap = rerank_ref.mmr(rel, G, np.ones(idx.shape, bool), k, lam)
    keep = gap > EPS_EXACT
    out = 1.0 - keep.mean()
    print(f"left out by the gap rule (gap <= {EPS_EXACT:.1e}): {out:.1%} of {len(idx)} users")
    assert out <= MAX_LEFT_OUT
    assert np.array_equal(gp[keep], pos[keep])


# ------------------------------------------------------------------ 4. properties
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_rerank_lambda_one_and_permutation(gpu_device, dtype):
    table, inv = _random_inputs(dtype, gpu_device)[:2]
    idx, rel, G = _random_lists(dtype, gpu_device, 64)
    for k in (1, 10, 64):
        gi, gr, gp, gild, _ = _run(table, inv, idx, rel, k, 1.0)
        assert np.array_equal(gi, idx[:, :k]) and np.array_equal(_bits(gr), _bits(rel[:, :k]))
        assert (gp == np.arange(k)).all()
        assert np.array_equal(_bits(gild[:, 0]), _bits(gild[:, 1])), "the same set in the same order"
    for lam in (0.0, 0.4):
        gi, gr, gp, _, _ = _run(table, inv, idx, rel, 64, lam)
        assert (np.sort(gp, axis=1) == np.arange(64)).all(), "K = M must return a permutation"
        assert (np.sort(gi, axis=1) == np.sort(idx, axis=1)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_rerank_pads_short_lists_and_large_indices(gpu_device, dtype):
    table, inv, _, table64, inv64 = _random_inputs(dtype, gpu_device)
    idx, rel, _ = _random_lists(dtype, gpu_device, 33)
    idx, rel = idx[:40].copy(), rel[:40].copy()
    rng = np.random.default_rng(23)
    idx[:, 0] = -1                       # a pad at the head,
    idx[:, 7] = N_NEWS                   # the first row past the table in the middle,
    idx[::2, 20] = np.iinfo(np.int32).max
    idx[1::2, 21] = np.iinfo(np.int32).min
    rel[:, [0, 7, 20, 21]] = 50.0        # each with a tempting relevance
    idx[5, 3:] = -1                      # two valid entries left
    idx[6, :] = -7                       # none
    rel[6, 4] = np.nan
    valid = rerank_ref.valid_entries(idx, N_NEWS)
    G = rerank_ref.gram(table64, inv64, idx)
    for k, lam in ((10, 0.5), (33, 0.2)):
        gi, gr, gp, gild, gsim = _run(table, inv, idx, rel, k, lam)
        assert np.isfinite(gsim).all() and np.abs(gsim.astype(np.float64) - G).max() <= SIM_EPS
        pad = ~valid
        assert not gsim[pad].any() and not np.swapaxes(gsim, 1, 2)[pad].any(), "a pad's row or column is not 0"
        rerank_ref.check_valid_greedy(gp, np.where(valid, rel, 0.0), G, valid, lam, 2 * (1 - lam) * SIM_EPS)
        rows = np.arange(len(idx))[:, None]
        short = gp < 0
        assert np.array_equal(np.where(short, -1, idx[rows, gp]), gi)
        assert np.isneginf(gr[short]).all() and np.array_equal(_bits(gr[~short]), _bits(rel[rows, gp][~short]))
        assert short[6].all() and (gp[5, :2] >= 1).all() and short[5, 2:].all()
        assert gild[6].tolist() == [0.0, 0.0]
        n_valid = valid.sum(axis=1)
        assert (short.sum(axis=1) == np.maximum(k - n_valid, 0)).all()
        want = np.array([[rerank_ref.ild(G[u], np.nonzero(valid[u])[0][:k]), rerank_ref.ild(G[u], gp[u])]
                         for u in range(len(idx))])
        assert np.abs(gild - want).max() <= SIM_EPS


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_rerank_duplicate_and_zero_rows(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    table_h, inv_h, table, inv = _planted_table(dtype, gpu_device)
    # the same row twice, every relevance equal: the second copy (cosine exactly 1 to the first) goes last
    idx = np.array([[5, 9, 700, 5, 31, 2999, 64, 1]], dtype=np.int32)
    rel = np.full(idx.shape, 0.5, dtype=np.float32)
    gi, gr, gp, _, gsim = _run(table, inv, idx, rel, 8, 0.5)
    assert gsim[0, 0, 3] == 1.0 and gsim[0, 3, 0] == 1.0
    assert gp[0, 0] == 0 and gp[0, -1] == 3 and sorted(gp[0].tolist()) == list(range(8))
    # a zero table row: inverse norm 1e8, similarity 0 everywhere, nothing NaN
    zt = table.clone()
    zt[9] = 0
    zinv = ops.row_inv_norm(zt, 1e-8)
    assert float(zinv[9]) == 1e8
    gi, gr, gp, gild, gsim = _run(zt, zinv, idx, rel, 8, 0.5)
    assert np.isfinite(gsim).all() and np.isfinite(gild).all()
    assert not gsim[0, 1].any() and not gsim[0, :, 1].any()
    assert sorted(gp[0].tolist()) == list(range(8))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_rerank_stride_grid_and_rerun_independent(gpu_device, dtype):
    table, inv, _, table64, inv64 = _random_inputs(dtype, gpu_device)
    rng = np.random.default_rng(24)
    n_users, m, k, lam = 1031, 33, 12, 0.6
    idx = rng.integers(0, N_NEWS, (n_users, m)).astype(np.int32)
    rel = rng.standard_normal((n_users, m)).astype(np.float32)
    a = _run(table, inv, idx, rel, k, lam)
    b = _run(table, inv, idx, rel, k, lam)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y)), "two runs differ"
    # a padded row stride
    wide = torch.zeros((N_NEWS, 1088), dtype=dtype, device=gpu_device)
    wide[:, :D] = table
    wide[:, D:] = 3.0
    c = _run(wide[:, :D], inv, idx, rel, k, lam)
    for x, y in zip(a, c):
        assert np.array_equal(_bits(x), _bits(y)), "cand_ld = 1088 differs from 1024"
    # one user alone: the same bits as among 1,031
    for u in (0, 517, 1030):
        d = _run(table, inv, idx[u:u + 1], rel[u:u + 1], k, lam)
        for x, y in zip(a, d):
            assert np.array_equal(_bits(x[u:u + 1]), _bits(y)), f"user {u} alone differs"
    # and everybody is a valid greedy run
    G = rerank_ref.gram(table64, inv64, idx[:100])
    rerank_ref.check_valid_greedy(a[2][:100], rel[:100], G, np.ones((100, m), bool), lam, 2 * (1 - lam) * SIM_EPS)


@pytest.mark.gpu
def test_gpu_rerank_refusals_leave_outputs_untouched(gpu_device):
    from news_recommendation_project_v2_amd import _lib, ops
    lib = _lib.load()
    table, inv = _random_inputs(torch.float32, gpu_device)[:2]
    tb = _random_inputs(torch.bfloat16, gpu_device)[0]
    idx, rel, _ = _random_lists(torch.float32, gpu_device, 17)
    li, lr = torch.from_numpy(idx[:4]).to(gpu_device), torch.from_numpy(rel[:4]).to(gpu_device)
    outs = {"oi": torch.full((4, 5), 77, dtype=torch.int32, device=gpu_device),
            "orel": torch.full((4, 5), 7.5, dtype=torch.float32, device=gpu_device),
            "op": torch.full((4, 5), 77, dtype=torch.int32, device=gpu_device),
            "oild": torch.full((4, 2), 7.5, dtype=torch.float32, device=gpu_device),
            "sim": torch.full((4, 17, 17), 7.5, dtype=torch.float32, device=gpu_device)}
    host = np.zeros(4096, dtype=np.float32)
    err = lambda: lib.nr_last_error().decode()
    p = lambda t: None if t is None else t if isinstance(t, int) else t.data_ptr()

    def call(dtype=_lib.NR_F32, dim=1024, U=4, N=N_NEWS, table=table, ld=1024, inv=inv, li=li, lr=lr, M=17, K=5,
             lam=0.5, **o):
        o = {**outs, **o}
        return lib.nr_rerank_mmr(dtype, dim, U, N, p(table), ld, p(inv), p(li), p(lr), M, K, lam, p(o["oi"]),
                                 p(o["orel"]), p(o["op"]), p(o["oild"]), p(o["sim"]), None)

    refused = [
        (dict(dim=512), UNSUPPORTED, "dim 512 unsupported"), (dict(dtype=_lib.NR_F16), INVALID, "bad dtype"),
        (dict(dtype=9), INVALID, "bad dtype"), (dict(M=0, K=1), INVALID, "M = 0 outside"),
        (dict(M=65), INVALID, "M = 65 outside"), (dict(K=0), INVALID, "K = 0 outside"),
        (dict(K=18), INVALID, "K = 18 outside"), (dict(lam=-0.5), INVALID, "outside [0, 1]"),
        (dict(lam=1.5), INVALID, "outside [0, 1]"), (dict(lam=float("nan")), INVALID, "outside [0, 1]"),
        (dict(U=0), INVALID, "U = 0"), (dict(N=0), INVALID, "N = 0"), (dict(ld=1000), INVALID, "cand_ld = 1000 < dim"),
        (dict(ld=1026), INVALID, "16-byte"), (dict(dtype=_lib.NR_BF16, table=tb, ld=1028), INVALID, "16-byte"),
        (dict(table=table.data_ptr() + 4), INVALID, "16-byte"),
    ]
    refused += [({n: None}, INVALID, "null pointer") for n in ("table", "inv", "li", "lr", "oi", "orel")]
    refused += [({n: host.ctypes.data}, INVALID, "not device memory")
                for n in ("table", "inv", "li", "lr", "oi", "orel", "op", "oild", "sim")]
    for kw, want, text in refused:
        assert call(**kw) == want and text in err(), (kw, err())
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert bool((t == (77 if t.dtype == torch.int32 else 7.5)).all()), f"a refused call wrote {n}"
    # the wrapper refuses the same before the library is reached
    for bad in (dict(k=0), dict(k=18), dict(lam=1.5), dict(lam=float("nan"))):
        with pytest.raises(_lib.NewsRecHIPError):
            ops.rerank_mmr(table, inv, li, lr, **{"k": 5, "lam": 0.5, **bad})
    with pytest.raises(_lib.NewsRecHIPError):
        ops.rerank_mmr(table, inv, li.long(), lr, 5, 0.5)
    with pytest.raises(_lib.NewsRecHIPError):
        ops.rerank_mmr(table.cpu(), inv, li, lr, 5, 0.5)
    # and the accepted call writes every output
    assert call() == 0, err()
    torch.cuda.synchronize()
    assert not bool((outs["oi"] == 77).any()) and not bool((outs["sim"] == 7.5).any())


# ------------------------------------------------------------------ 5. engine
@pytest.mark.gpu
@pytest.mark.parametrize("pooler,dtype", [("final", torch.float32), ("latent", torch.bfloat16)])
def test_gpu_engine_recommend_diverse(gpu_device, pooler, dtype):
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    rng = np.random.default_rng(25)
    n_news, n_imp, k = 300, 60, 10
    distinct = [rng.integers(0, n_news, n).astype(np.int32) for n in rng.integers(1, 9, 14)]
    pick = rng.integers(0, 14, n_imp)  # repeated histories: the deduplicated path
    hl = np.array([len(distinct[p]) for p in pick], dtype=np.int32)
    hi = np.concatenate([distinct[p] for p in pick]).astype(np.int32)
    eq = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    results = {}
    for dedupe in (True, False):
        eng = PoolScoreEngine(_model(pooler, gpu_device), dtype=dtype, device=gpu_device)
        eng.load_news(W.news_table(5, n_news, 1024, name="rerank"))
        eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(n_imp, np.int32), dedupe=dedupe)
        assert (eng.user_idx is not None) == dedupe
        plain = eng.recommend(k)
        assert eq(eng.recommend_diverse(k, 1.0), plain), "lam = 1 must be recommend(k)"
        assert eq(eng.recommend_diverse(k, 1.0, pool=k), plain)
        div = eng.recommend_diverse(k, 0.5, want_ild=True)
        assert eq(eng.recommend_diverse(k, 0.5, user_block=7, want_ild=True), div), "user_block changes the result"
        assert eq(eng.recommend(k), plain), "recommend changed after recommend_diverse"
        i5, s5, ild = div
        assert i5.shape == s5.shape == (n_imp, k) and ild.shape == (n_imp, 2) and i5.dtype == torch.int32
        assert torch.equal(i5[:, 0], plain[0][:, 0]), "round 0 picks the most relevant news"
        pool_i, pool_s = eng.recommend(64)
        torch.cuda.synchronize()
        for i in range(0, n_imp, 7):  # the picks come from the pool, with the pool's own scores
            at = {int(r): float(s) for r, s in zip(pool_i[i].tolist(), pool_s[i].tolist())}
            assert all(at[int(r)] == float(s) for r, s in zip(i5[i].tolist(), s5[i].tolist()))
        with pytest.raises(ValueError):
            eng.recommend_diverse(k, 0.5, pool=k - 1)
        results[dedupe] = (plain, div)
    assert eq(results[True][0], results[False][0]) and eq(results[True][1], results[False][1]), "dedupe changes lists"


@pytest.mark.gpu
def test_gpu_get_top_k_recommendations_diversify(gpu_device):
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    from news_recommendation_project_v2_amd.evaluation import diversity_metrics
    rng = np.random.default_rng(26)
    n_news, n_imp, k = 200, 30, 6
    hl = rng.integers(1, 9, n_imp).astype(np.int32)
    hi = rng.integers(0, n_news, int(hl.sum())).astype(np.int32)
    table = W.news_table(5, n_news, 1024, name="rerank-api")
    m = _model("final", gpu_device)
    eng = PoolScoreEngine(m, dtype=dmh.COMPUTE_DTYPE, device=gpu_device)
    eng.load_news(table)
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(n_imp, np.int32))
    wi, ws = (t.cpu().numpy() for t in eng.recommend(k))
    got = dmh.get_top_k_recommendations(hi, hl, table, m, k)
    assert sorted(got) == ["news_index", "scores"], "the default return shape changed"
    assert np.array_equal(got["news_index"], wi) and np.array_equal(_bits(got["scores"]), _bits(ws))
    same = dmh.get_top_k_recommendations(hi, hl, table, m, k, diversify=1.0)
    assert np.array_equal(same["news_index"], wi) and np.array_equal(_bits(same["scores"]), _bits(ws))
    assert np.array_equal(_bits(same["plain_scores"]), _bits(ws))
    div = dmh.get_top_k_recommendations(hi, hl, table, m, k, diversify=0.3, pool=32)
    di, ds, dild = (t.cpu().numpy() for t in eng.recommend_diverse(k, 0.3, pool=32, want_ild=True))
    assert np.array_equal(div["news_index"], di) and np.array_equal(_bits(div["scores"]), _bits(ds))
    assert np.array_equal(_bits(div["ild"]), _bits(dild)) and div["ild"].dtype == np.float32
    met = diversity_metrics(div["ild"], rel_before=div["plain_scores"], rel_after=div["scores"])
    assert met["lists"] == n_imp and met["relevance_after"] <= met["relevance_before"] + 1e-12
    with pytest.raises(ValueError):
        dmh.get_top_k_recommendations(hi, hl, table, m, k, pool=32)
