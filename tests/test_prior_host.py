"""The rank-one prior entries of the C ABI (include/newsrec_prior.h) on the host: signature
table, the refusals that need no device, the workspace functions, the float64 reference of
the GPU tests (tests/prior_ref.py) against brute force, the engine's and helper's argument
checks, and data_utils.history_popularity / synthetic.catalogue_prior."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

import prior_ref
from conftest import REPO
from news_recommendation_project_v2_amd import _lib, data_utils, synthetic

HEADER = REPO / "include" / "newsrec_prior.h"
F32, BF16 = _lib.NR_F32, _lib.NR_BF16
INVALID, UNSUPPORTED = -1, -3
ENTRIES = ["nr_rank_targets_prior", "nr_rank_targets_prior_workspace_bytes", "nr_topk_sections_prior",
           "nr_topk_sections_prior_workspace_bytes", "nr_topk_users_prior", "nr_topk_users_prior_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.is_file():
        pytest.skip("libnewsrec_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_prior_signatures_cover_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(nr_[a-z0-9_]+)\s*\(", text)))
    assert fns == sorted(_lib.PRIOR_SIGNATURES) == ENTRIES
    for f in fns:
        assert hasattr(lib, f), f
    P = ctypes.c_void_p
    # the two prior pointers behind the mask pointer, top_keys behind top_scores
    a, b = _lib.FILTER_SIGNATURES["nr_topk_users_filtered"][1], _lib.PRIOR_SIGNATURES["nr_topk_users_prior"][1]
    assert b[:15] == a[:15] and b[15:17] == [P, P] and b[17:20] == a[15:18] and b[20] is P and b[21:] == a[18:]
    a, b = _lib.FILTER_SIGNATURES["nr_rank_targets_filtered"][1], _lib.PRIOR_SIGNATURES["nr_rank_targets_prior"][1]
    assert b[:15] == a[:15] and b[15:17] == [P, P] and b[17:] == a[15:]
    a, b = _lib.SECTIONS_SIGNATURES["nr_topk_sections"][1], _lib.PRIOR_SIGNATURES["nr_topk_sections_prior"][1]
    assert b[:15] == a[:15] and b[15:17] == [P, P] and b[17:21] == a[15:19] and b[21] is P and b[22:] == a[19:]
    for base, sib in (("nr_topk_workspace_bytes", "nr_topk_users_prior_workspace_bytes"),
                      ("nr_rank_targets_workspace_bytes", "nr_rank_targets_prior_workspace_bytes"),
                      ("nr_topk_sections_workspace_bytes", "nr_topk_sections_prior_workspace_bytes")):
        sigs = {**_lib.TOPK_SIGNATURES, **_lib.FULLRANK_SIGNATURES, **_lib.SECTIONS_SIGNATURES}
        assert _lib.PRIOR_SIGNATURES[sib] == sigs[base]
    assert "newsrec_prior.h" in [p.name for p in _lib.hip_source_files()]
    assert "newsrec_prior.h" in (REPO / "news_recommendation_project_v2_amd" / "csrc" / "Makefile").read_text()


def test_prior_refusals_on_the_host(lib):
    """Every refusal of the contract returns its code and message before any device call
    (this host has none; a launch would fail differently)."""
    raw = np.zeros(1 << 20, dtype=np.uint8)
    P = raw.ctypes.data + (-raw.ctypes.data) % 256
    WS = 1 << 40
    err = lambda: lib.nr_last_error().decode()
    one = (ctypes.c_uint64 * 2)(0b0011, 0b1100)
    SEC = ctypes.cast(one, ctypes.c_void_p)

    def topk(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=None, qm=None, pr=None, ga=None, K=5, ti=P, ts=P, tk=P, ws=P, wsb=WS):
        return lib.nr_topk_users_prior(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, pr, ga,
                                       K, ti, ts, tk, ws, wsb, None)

    def rank(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=None, qm=None, pr=None, ga=None, T=6, tidx=P, toff=P, out=P, ws=P, wsb=WS):
        return lib.nr_rank_targets_prior(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, pr,
                                         ga, T, tidx, toff, out, ws, wsb, None)

    def sect(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=P, qm=SEC, pr=None, ga=None, S=2, k=4, ti=P, ts=P, tk=P, ws=P, wsb=WS):
        return lib.nr_topk_sections_prior(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, pr,
                                          ga, S, k, ti, ts, tk, ws, wsb, None)

    for call, name in ((topk, "nr_topk_users_prior"), (rank, "nr_rank_targets_prior"),
                       (sect, "nr_topk_sections_prior")):
        # the pairing rule of the prior
        for half in ({"pr": P}, {"ga": P}):
            assert call(**half) == INVALID and "news_prior and user_gain go together" in err(), (name, half)
            assert name in err()
        # the base entries' refusals, with their messages
        for half in ({"nt": P}, {"lo": P, "hi": P}):
            assert call(**half) == INVALID and "news_time, q_time_lo and q_time_hi go together" in err(), half
        assert call(dim=512) == UNSUPPORTED and "dim 512 unsupported" in err()
        assert call(dtype=_lib.NR_F16) == INVALID and "bad dtype" in err()
        assert call(U=0) == INVALID and "U = 0" in err()
        assert call(N=0) == INVALID and "N = 0 < 1" in err()
        assert call(N=(1 << 22) + 1) == UNSUPPORTED and "unsupported" in err()
        assert call(ld=1016) == INVALID and "cand_ld = 1016 < dim" in err()
        assert call(ld=1026) == INVALID and "16-byte" in err()
        assert call(table=P + 4) == INVALID and "16-byte" in err()
        assert call(eidx=P) == INVALID and "excl_idx and excl_off go together" in err()
        for null in ("users", "table", "inv", "ws"):
            assert call(**{null: None}) == INVALID and "null pointer" in err(), (name, null)
        assert call(ws=P + 16, wsb=WS) == INVALID and "256-byte aligned" in err()
        # host pointers, the prior's included, stop at the residency check
        assert call() == INVALID and "not device memory" in err()
        assert call(pr=P, ga=P) == INVALID and "not device memory" in err()
    for call in (topk, rank):
        for half in ({"nc": P}, {"qm": P}):
            assert call(**half) == INVALID and "news_cat and q_cat_mask go together" in err(), half
    # top-K: K, the outputs (top_keys is required), the workspace with its U floats more
    for k in (0, -1, 65):
        assert topk(K=k) == INVALID and f"K = {k} outside [1, 64]" in err()
    for null in ("ti", "ts", "tk"):
        assert topk(**{null: None}) == INVALID and "null pointer" in err(), null
    need = lib.nr_topk_users_prior_workspace_bytes(F32, 4, 100, 5)
    assert need >= lib.nr_topk_workspace_bytes(F32, 4, 100, 5) + 16
    assert topk(wsb=need - 1) == INVALID and "workspace too small" in err()
    assert topk(wsb=need, pr=P, ga=P) == INVALID and "not device memory" in err()
    # ranks
    assert rank(T=-1) == INVALID and "T = -1" in err()
    for null in ("tidx", "toff", "out"):
        assert rank(**{null: None}) == INVALID and "null pointer" in err(), null
    need = lib.nr_rank_targets_prior_workspace_bytes(F32, 4, 100, 6)
    assert rank(wsb=need - 1) == INVALID and "workspace too small" in err()
    assert rank(wsb=need, pr=P, ga=P) == INVALID and "not device memory" in err()
    # sections
    assert sect(S=0) == INVALID and "S = 0 outside [1, 16]" in err()
    assert sect(k=0) == INVALID and "k = 0 < 1" in err()
    assert sect(S=2, k=33) == INVALID and "exceeds the 64 list slots" in err()
    assert sect(nc=None) == INVALID and "news_cat and sec_mask are required" in err()
    both = (ctypes.c_uint64 * 2)(0b0110, 0b1100)
    assert sect(qm=ctypes.cast(both, ctypes.c_void_p)) == INVALID and "sections 0 and 1 share category 2" in err()
    for null in ("ti", "ts", "tk"):
        assert sect(**{null: None}) == INVALID and "null pointer" in err(), null
    need = lib.nr_topk_sections_prior_workspace_bytes(F32, 4, 100, 2, 4)
    assert sect(wsb=need - 1) == INVALID and "workspace too small" in err()
    assert sect(wsb=need, pr=P, ga=P) == INVALID and "not device memory" in err()


def test_prior_workspace_bytes(lib):
    """The base layout plus U floats (256-byte granules); -1 for the base functions' bad shapes."""
    pad = lambda n: (n + 255) // 256 * 256
    for dt in (F32, BF16):
        for U, N, K in ((1, 1, 1), (130, 16384 + 300, 64), (5000, 100000, 10)):
            assert lib.nr_topk_users_prior_workspace_bytes(dt, U, N, K) == lib.nr_topk_workspace_bytes(dt, U, N, K) + pad(4 * U)
            assert (lib.nr_rank_targets_prior_workspace_bytes(dt, U, N, 3 * U)
                    == lib.nr_rank_targets_workspace_bytes(dt, U, N, 3 * U) + pad(4 * U))
            assert (lib.nr_topk_sections_prior_workspace_bytes(dt, U, N, 4, max(1, K // 4))
                    == lib.nr_topk_sections_workspace_bytes(dt, U, N, 4, max(1, K // 4)) + pad(4 * U))
    for bad in ((2, 4, 100, 5), (F32, 0, 100, 5), (F32, 1 << 31, 100, 5), (F32, 4, 0, 5), (F32, 4, (1 << 22) + 1, 5),
                (F32, 4, 100, 0), (F32, 4, 100, 65)):
        assert lib.nr_topk_users_prior_workspace_bytes(*bad) == -1 == lib.nr_topk_workspace_bytes(*bad), bad
    for bad in ((2, 4, 100, 5), (F32, 0, 100, 5), (F32, 4, 0, 5), (F32, 4, (1 << 22) + 1, 5), (F32, 4, 100, -1),
                (F32, 4, 100, 1 << 31)):
        assert lib.nr_rank_targets_prior_workspace_bytes(*bad) == -1 == lib.nr_rank_targets_workspace_bytes(*bad), bad
    for bad in ((2, 4, 100, 2, 4), (F32, 0, 100, 2, 4), (F32, 4, 0, 2, 4), (F32, 4, (1 << 22) + 1, 2, 4),
                (F32, 4, 100, 0, 4), (F32, 4, 100, 17, 1), (F32, 4, 100, 2, 0), (F32, 4, 100, 5, 13)):
        assert (lib.nr_topk_sections_prior_workspace_bytes(*bad) == -1
                == lib.nr_topk_sections_workspace_bytes(*bad)), bad


def test_ops_prior_checks_on_the_host():
    """ops refuses non-device tensors (no CPU fallback) before anything else; the pair is checked."""
    import torch
    from news_recommendation_project_v2_amd import ops
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.topk_users_prior(torch.zeros(2, 1024), torch.zeros(5, 1024), torch.ones(5), 3,
                             news_prior=torch.zeros(5), user_gain=torch.zeros(2))
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.rank_targets_prior(torch.zeros(2, 1024), torch.zeros(5, 1024), torch.ones(5),
                               torch.zeros(1, dtype=torch.int32), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.topk_sections_prior(torch.zeros(2, 1024), torch.zeros(5, 1024), torch.ones(5), 3, [1, 2],
                                torch.zeros(5, dtype=torch.uint8))
    assert ops._check_prior("t", 2, 5, None, None) == [None, None]
    p5, g2 = torch.zeros(5), torch.zeros(2)
    for pair in ((p5, None), (None, g2)):
        with pytest.raises(_lib.NewsRecHIPError, match="news_prior and user_gain go together"):
            ops._check_prior("t", 2, 5, *pair)
    with pytest.raises(_lib.NewsRecHIPError, match=r"news_prior must be contiguous torch.float32 \[5\]"):
        ops._check_prior("t", 2, 5, g2, g2)
    with pytest.raises(_lib.NewsRecHIPError, match=r"user_gain must be contiguous torch.float32 \[2\]"):
        ops._check_prior("t", 2, 5, p5, g2.double())
    assert len(ops._check_prior("t", 2, 5, p5, g2)) == 2
    with pytest.raises(_lib.NewsRecHIPError, match="unsupported shape"):
        ops.topk_users_prior_workspace_bytes(torch.float32, 4, 100, 65)
    with pytest.raises(_lib.NewsRecHIPError, match="unsupported shape"):
        ops.rank_targets_prior_workspace_bytes(torch.float32, 4, 0, 5)
    with pytest.raises(_lib.NewsRecHIPError, match="unsupported shape"):
        ops.topk_sections_prior_workspace_bytes(torch.float32, 4, 100, 17, 1)
    assert (ops.topk_users_prior_workspace_bytes(torch.bfloat16, 4, 100, 16)
            == ops.topk_workspace_bytes(torch.bfloat16, 4, 100, 16) + 256)


# ------------------------------------------------------------------ the reference against brute force
def test_prior_ref_matches_brute_force():
    rng = np.random.default_rng(41)
    seen = {"short": 0, "reordered": 0, "tie": 0}
    for i in range(24):
        U, N, K = int(rng.integers(1, 6)), int(rng.integers(1, 40)), int(rng.integers(1, 12))
        s = rng.standard_normal((U, N))
        prior = rng.random(N)
        gain = rng.standard_normal(U)
        if i % 2 == 0:  # ties between keys: half-integer scores, priors and gains
            s, prior, gain = np.round(s * 2) / 2, np.round(prior * 2) / 2, np.round(gain)
        gain[0] = 0.0
        eidx = eoff = elig = None
        if i % 2:
            lens = rng.integers(0, 5, U)
            eoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            eidx = rng.integers(0, N, int(lens.sum())).astype(np.int32)
        if i % 3 == 0:
            elig = rng.random((U, N)) < 0.6
        got, want = prior_ref.topk(s, K, gain, prior, eidx, eoff, elig), prior_ref.brute_force(s, K, gain, prior, eidx,
                                                                                               eoff, elig)
        for g, w, what in zip(got, want, ("idx", "scores", "keys")):
            assert np.array_equal(g, w), (i, what)
        idx, sc, ky = got
        assert np.array_equal(ky[idx >= 0], (sc + gain[:, None] * prior[np.maximum(idx, 0)])[idx >= 0])
        assert np.isneginf(sc[idx < 0]).all() and np.isneginf(ky[idx < 0]).all()
        assert (ky[:, 1:] <= ky[:, :-1]).all()
        seen["short"] += int((idx < 0).any())
        seen["tie"] += int(((ky[:, 1:] == ky[:, :-1]) & (idx[:, 1:] >= 0)).any())
        plain = prior_ref.topk(s, K, np.zeros(U), prior, eidx, eoff, elig)
        assert np.array_equal(plain[0][0], idx[0]), "gain 0 is no prior"
        seen["reordered"] += int(not np.array_equal(plain[0], idx))
    assert all(v > 0 for v in seen.values()), seen
    # gain 0 everywhere: topk_ref.topk itself
    import topk_ref
    s = rng.standard_normal((3, 20))
    assert np.array_equal(prior_ref.topk(s, 5, np.zeros(3), rng.random(20))[0], topk_ref.topk(s, 5)[0])


# ------------------------------------------------------------------ engine and helper
def test_engine_and_helper_refuse_bad_priors_on_the_host():
    """The argument checks run ahead of any device work: no GPU is needed to be refused."""
    import torch
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd import engine
    eng = engine.PoolScoreEngine.__new__(engine.PoolScoreEngine)
    eng.news_cat = eng.news_time = eng.news_prior = None
    eng.device = torch.device("cpu")
    eng.cand_table = torch.zeros(10, 1024)
    eng.n_imp, eng.user_idx = 3, None
    for bad in (np.full(10, np.nan), np.r_[np.zeros(9), np.inf], np.r_[np.zeros(9), -np.inf]):
        with pytest.raises(ValueError, match="news_prior must be finite"):
            eng.set_catalogue(news_prior=bad)
    for bad in (np.zeros(9), np.zeros(11), np.zeros((10, 1)), 0.5):
        with pytest.raises(ValueError, match=r"one entry per news \(10\)"):
            eng.set_catalogue(news_prior=bad)
    with pytest.raises(ValueError, match="numbers"):
        eng.set_catalogue(news_prior=np.array(["a"] * 10))
    assert eng.news_prior is None
    # a gain without a prior
    for call in (lambda: eng.recommend(4, prior_gain=0.5), lambda: eng.rank_targets([], [0, 0, 0], prior_gain=0.5)):
        with pytest.raises(ValueError, match=r"prior_gain needs set_catalogue\(news_prior"):
            call()
    eng.news_cat = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"prior_gain needs set_catalogue\(news_prior"):
        eng.recommend_sections(4, [[0], [1]], prior_gain=0.5)
    eng.set_catalogue(news_prior=np.linspace(0, 1, 10))
    assert eng.news_prior.dtype == torch.float32 and eng.news_prior.shape == (10,)
    for bad in (float("nan"), float("inf"), [0.1, float("-inf"), 0.2]):
        with pytest.raises(ValueError, match="prior_gain must be finite"):
            eng.recommend(4, prior_gain=bad)
    for bad in ([0.1, 0.2], np.zeros(4), np.zeros((3, 1))):
        with pytest.raises(ValueError, match=r"one value per impression \(3\)"):
            eng.recommend(4, prior_gain=bad)
    with pytest.raises(ValueError, match="must be a number"):
        eng.recommend(4, prior_gain="much")
    # the modes that do not take a prior
    for call in (lambda: eng.recommend_diverse(4, 0.5, prior_gain=0.1), lambda: eng.explain(None, prior_gain=0.1),
                 lambda: eng.recommend_explained_filtered(4, prior_gain=0.1)):
        with pytest.raises(ValueError, match="prior_gain cannot be combined with diversify or explain"):
            call()
    with pytest.raises(TypeError):  # (its signature is as it was: the argument does not exist there)
        eng.recommend_explained(4, prior_gain=0.1)
    # the distinct-query key: (history, gain), +0 and -0 one gain
    assert eng._queries(None, None, np.array([0.5, 0.5, 0.5], np.float32)).n == 3  # three histories
    eng.user_idx = torch.tensor([0, 1, 1], dtype=torch.int32)
    q = eng._queries(None, None, np.array([0.5, 0.0, -0.0], np.float32))
    assert q.n == 2 and q.sel_host[1] == q.sel_host[2] != q.sel_host[0] and sorted(q.gain.tolist()) == [0.0, 0.5]
    eng.user_idx = torch.tensor([0, 0, 0], dtype=torch.int32)
    q = eng._queries(None, None, np.array([0.5, 0.25, 0.5], np.float32))
    assert q.n == 2 and q.user_host.tolist() == [0, 0] and q.sel_host[0] == q.sel_host[2] != q.sel_host[1]
    assert eng._queries(None, None, None) is None
    # the helpers: before any engine exists
    args = (np.zeros(2, np.int32), np.array([1, 1]), torch.zeros(10, 1024), None, 4)
    ok = np.linspace(0, 1, 10, dtype=np.float32)
    for fn, a in ((dmh.get_top_k_recommendations, args),
                  (dmh.get_full_table_ranks, args[:2] + (np.zeros(2, np.int32), np.array([1, 1])) + args[2:4])):
        with pytest.raises(ValueError, match="news_prior must be finite"):
            fn(*a, prior=np.full(10, np.nan), prior_gain=0.1)
        with pytest.raises(ValueError, match=r"one entry per news \(10\)"):
            fn(*a, prior=np.zeros(7), prior_gain=0.1)
        with pytest.raises(ValueError, match="prior_gain needs prior"):
            fn(*a, prior_gain=0.1)
        with pytest.raises(ValueError, match="prior_gain must be finite"):
            fn(*a, prior=ok, prior_gain=float("inf"))
        with pytest.raises(ValueError, match=r"one value per impression \(2\)"):
            fn(*a, prior=ok, prior_gain=[0.1, 0.2, 0.3])
    for combo in ({"diversify": 0.5}, {"explain": 2}, {"diversify": 0.5, "pool": 32}):
        with pytest.raises(ValueError, match="prior_gain cannot be combined with diversify or explain"):
            dmh.get_top_k_recommendations(*args, prior=ok, prior_gain=0.1, **combo)


def test_history_popularity_on_a_hand_made_csr():
    # histories: [0 1 1], the same again, [2 0], an empty one, [3]; news 4 and 5 are in none
    hist_idx = np.array([0, 1, 1, 0, 1, 1, 2, 0, 3], np.int32)
    hist_len = np.array([3, 3, 2, 0, 1])
    pop = data_utils.history_popularity(hist_idx, hist_len, 6)
    assert pop.dtype == np.float32 and pop.shape == (6,)
    # distinct histories per news: 2, 1, 1, 1, 0, 0 (the repeated history and the repeated click count once)
    want = np.log1p(np.array([2, 1, 1, 1, 0, 0], dtype=np.float64)) / np.log1p(2.0)
    assert np.array_equal(pop, want.astype(np.float32))
    assert pop.max() == 1.0 and pop.min() == 0.0
    # a loop over sets
    rng = np.random.default_rng(9)
    n_news = 40
    lens = rng.integers(0, 7, 60)
    idx = rng.integers(0, n_news - 2, int(lens.sum())).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)])
    count = np.zeros(n_news)
    for h in {tuple(idx[off[i]:off[i + 1]].tolist()) for i in range(len(lens))}:
        for r in set(h):
            count[r] += 1
    got = data_utils.history_popularity(idx, lens, n_news)
    assert np.array_equal(got, (np.log1p(count) / np.log1p(count.max())).astype(np.float32))
    assert (data_utils.history_popularity(np.zeros(0, np.int32), np.zeros(4, np.int64), 5) == 0).all()
    assert data_utils.history_popularity(np.zeros(0, np.int32), np.zeros(0, np.int64), 0).shape == (0,)
    with pytest.raises(ValueError):
        data_utils.history_popularity(idx[:-1], lens, n_news)
    with pytest.raises(IndexError):
        data_utils.history_popularity(idx, lens, int(idx.max()))


def test_synthetic_prior_leaves_the_set_unchanged():
    before = synthetic.mind_impressions(500, 300, seed=1234, users=40)
    prior = synthetic.catalogue_prior(500, seed=1234)
    after = synthetic.mind_impressions(500, 300, seed=1234, users=40)
    for name in ("hist_idx", "hist_len", "cand_idx", "cand_len", "labels"):
        assert np.array_equal(getattr(before, name), getattr(after, name)), name
    when, cats = synthetic.catalogue_attributes(500, 300, seed=1234)
    assert np.array_equal(synthetic.catalogue_attributes(500, 300, seed=1234)[1], cats)
    assert prior.dtype == np.float32 and prior.shape == (500,) and np.isfinite(prior).all()
    assert prior.min() >= 0.0 and prior.max() == 1.0 and len(np.unique(prior)) > 10
    assert np.array_equal(synthetic.catalogue_prior(500, seed=1234), prior)
    assert not np.array_equal(synthetic.catalogue_prior(500, seed=1235), prior)


def test_recommend_script_refuses_prior_combinations():
    """argparse refuses the combinations before the script touches a device."""
    script = str(REPO / "scripts" / "recommend.py")
    for extra, msg in ((["--prior", "popularity"], "--prior and --prior-gain go together"),
                       (["--prior-cold", "1"], "--prior-cold needs --prior"),
                       (["--prior", "popularity", "--prior-gain", "0.2", "--explain", "2"],
                        "--prior cannot be combined with --explain")):
        out = subprocess.run([sys.executable, script, "--synthetic", *extra], capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and msg in out.stderr, out.stderr[-500:]
