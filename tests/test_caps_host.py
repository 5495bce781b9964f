"""Per-group caps of top-K retrieval (include/newsrec_caps.h) on the host: the float64
reference of the GPU tests (tests/caps_ref.py) against brute force; the two streaming claims
the kernels rest on -- one running list of <= K entries in ascending row order, and the capped
merge of per-chunk lists -- modelled in Python and compared with the reference on random
ties and cuts; data_utils.dense_groups, evaluation.group_cap_metrics; the C entry's signature,
workspace function and the refusals that need no device; the Python layers' argument checks."""
import ctypes
import re

import numpy as np
import pytest

import caps_ref
from conftest import REPO
from news_recommendation_project_v2_amd import _lib, data_utils, evaluation

HEADER = REPO / "include" / "newsrec_caps.h"
F32, BF16 = _lib.NR_F32, _lib.NR_BF16
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.is_file():
        pytest.skip("libnewsrec_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _better(a, b):
    """(key, row) a before b in the strict total order."""
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


# ------------------------------------------------------------------ the reference against brute force
def test_caps_ref_matches_brute_force():
    rng = np.random.default_rng(17)
    seen = {"short": 0, "bites": 0, "tie": 0}
    for i in range(60):
        U, N, K = int(rng.integers(1, 4)), int(rng.integers(1, 10)), int(rng.integers(1, 5))
        G, cap = int(rng.integers(1, 5)), int(rng.integers(1, 4))
        s = rng.standard_normal((U, N))
        if i % 2 == 0:
            s = np.round(s)  # ties
        groups = rng.integers(0, G, N)
        eidx = eoff = elig = None
        if i % 2:
            lens = rng.integers(0, 3, U)
            eoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            eidx = rng.integers(-1, N + 1, int(lens.sum())).astype(np.int32)
        if i % 3 == 0:
            elig = rng.random((U, N)) < 0.7
        got = caps_ref.capped_topk(s, K, groups, cap, elig, eidx, eoff)
        want = caps_ref.brute_force(s, K, groups, cap, elig, eidx, eoff)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), i
        idx, ky = got
        for u in range(U):
            rows = idx[u][idx[u] >= 0]
            assert len(rows) == 0 or np.bincount(groups[rows]).max() <= cap
            assert len(set(rows.tolist())) == len(rows)
        assert (ky[:, 1:] <= ky[:, :-1]).all() and np.isneginf(ky[idx < 0]).all()
        plain = caps_ref.capped_topk(s, K, groups, K, elig, eidx, eoff)[0]
        seen["short"] += int((idx < 0).any())
        seen["bites"] += int(not np.array_equal(plain, idx))
        seen["tie"] += int(((ky[:, 1:] == ky[:, :-1]) & (idx[:, 1:] >= 0)).any())
    assert all(v > 5 for v in seen.values()), seen
    # cap >= K is the uncapped reference
    import topk_ref
    s = np.round(rng.standard_normal((3, 30)) * 2) / 2
    assert np.array_equal(caps_ref.capped_topk(s, 7, rng.integers(0, 3, 30), 7)[0], topk_ref.topk(s, 7)[0])


# ------------------------------------------------------------------ the streaming rule and the capped merge
def _stream(keys, groups, rows, K, cap):
    """One running list over ``rows`` (ascending), as include/newsrec_caps.h's stage 1 keeps it:
    a row must beat the list's threshold (the worst entry once K are kept); a group at its cap
    gives up its worst member to a better row only; otherwise append, or replace the worst."""
    kept = []  # (key, row, group)
    for r in rows:
        cand = (keys[r], r, groups[r])
        if len(kept) == K and not _better(cand, min(kept, key=lambda e: (e[0], -e[1]))):
            continue
        mates = [e for e in kept if e[2] == cand[2]]
        if len(mates) >= cap:
            worst = min(mates, key=lambda e: (e[0], -e[1]))
            if _better(cand, worst):
                kept[kept.index(worst)] = cand
        elif len(kept) < K:
            kept.append(cand)
        else:
            kept[kept.index(min(kept, key=lambda e: (e[0], -e[1])))] = cand
    return sorted(kept, key=lambda e: (-e[0], e[1]))


def _merge(lists, K, cap):
    """Stage 2: the best head wins a round and is taken unless its group is at the cap."""
    heads, out, held = [0] * len(lists), [], {}
    while len(out) < K:
        live = [(l[h], c) for c, (l, h) in enumerate(zip(lists, heads)) if h < len(l)]
        if not live:
            break
        e, c = min(live, key=lambda t: (-t[0][0], t[0][1]))
        heads[c] += 1
        if held.get(e[2], 0) < cap:
            held[e[2]] = held.get(e[2], 0) + 1
            out.append(e)
    return out


def test_caps_streaming_and_merge_match_the_reference():
    rng = np.random.default_rng(23)
    seen = {"short": 0, "bites": 0, "replaced_in_group": 0}
    for i in range(400):
        N, K = int(rng.integers(1, 60)), int(rng.integers(1, 12))
        G, cap = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        keys = np.round(rng.standard_normal(N) * (2 if i % 2 else 50)) / 2  # heavy ties on odd rounds
        groups = rng.integers(0, G, N)
        ok = rng.random(N) < 0.8
        rows = np.nonzero(ok)[0].tolist()
        want_i, want_k = caps_ref.capped_topk(keys[None], K, groups, cap, ok[None])
        want = [int(r) for r in want_i[0] if r >= 0]
        one = _stream(keys, groups, rows, K, cap)
        assert [e[1] for e in one] == want, (i, "one running list")
        # random cuts into chunks: per-chunk capped lists, then the capped merge
        cuts = sorted(set(rng.integers(0, N + 1, int(rng.integers(0, 5))).tolist()) | {0, N})
        parts = [_stream(keys, groups, [r for r in rows if a <= r < b], K, cap) for a, b in zip(cuts[:-1], cuts[1:])]
        assert [e[1] for e in _merge(parts, K, cap)] == want, (i, "capped merge", cuts)
        seen["short"] += int(len(want) < K)
        seen["bites"] += int(want != [int(r) for r in caps_ref.capped_topk(keys[None], K, groups, K, ok[None])[0][0]
                                      if r >= 0])
        seen["replaced_in_group"] += int(len(want) < min(K, len(rows)))
    assert all(v > 20 for v in seen.values()), seen


# ------------------------------------------------------------------ dense_groups, group_cap_metrics
def test_dense_groups():
    ids, names = data_utils.dense_groups(np.array(["sports", "news", "sports", "tv", "news"]))
    assert ids.dtype == np.uint16 and ids.tolist() == [0, 1, 0, 2, 1] and names == ["sports", "news", "tv"]
    ids, names = data_utils.dense_groups([7, 7, (1, "a"), 7, None])
    assert ids.tolist() == [0, 0, 1, 0, 2] and names == [7, (1, "a"), None]
    ids, names = data_utils.dense_groups(np.zeros(0, np.int64))
    assert ids.shape == (0,) and names == []
    ids, names = data_utils.dense_groups(np.arange(1024)[::-1])
    assert ids.tolist() == list(range(1024)) and names[0] == 1023
    with pytest.raises(ValueError, match="more than 1024 distinct labels"):
        data_utils.dense_groups(np.arange(1025))
    with pytest.raises(ValueError, match="one-dimensional"):
        data_utils.dense_groups(np.zeros((3, 2), np.int64))


def test_group_cap_metrics():
    groups = np.array([0, 0, 0, 1, 1, 2])
    idx = np.array([[0, 1, 3, 5], [3, 4, -1, -1], [5, -1, -1, -1]])
    m = evaluation.group_cap_metrics(idx, groups, 2)
    assert m == {"lists": 3, "max_group_count": 2, "at_cap_share": 2 / 3, "distinct_groups": 5 / 3}
    assert evaluation.group_cap_metrics(idx, groups, 3)["at_cap_share"] == 0.0
    capped = np.array([[4., 3, 2, 1], [2, 1, -np.inf, -np.inf], [1, -np.inf, -np.inf, -np.inf]])
    plain = np.array([[4., 4, 2, 2], [2, 2, 2, 2], [1, 1, 1, 1]])
    m = evaluation.group_cap_metrics(idx, groups, 2, capped, plain)
    assert m["score_given_up"] == pytest.approx(((3 - 2.5) + (2 - 1.5) + 0) / 3)
    empty = evaluation.group_cap_metrics(np.zeros((0, 4), np.int64), groups, 2)
    assert empty["lists"] == 0 and empty["max_group_count"] == 0 and np.isnan(empty["at_cap_share"])
    assert evaluation.group_cap_metrics(np.full((2, 3), -1), groups, 1)["max_group_count"] == 0
    with pytest.raises(IndexError, match="has no group"):
        evaluation.group_cap_metrics(np.array([[6]]), groups, 2)
    with pytest.raises(ValueError, match="go together"):
        evaluation.group_cap_metrics(idx, groups, 2, scores_capped=capped)
    with pytest.raises(ValueError, match="cap = 0"):
        evaluation.group_cap_metrics(idx, groups, 0)


# ------------------------------------------------------------------ the C entry
def test_caps_signatures_cover_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(nr_[a-z0-9_]+)\s*\(", text)))
    assert fns == sorted(_lib.CAPS_SIGNATURES) == ["nr_topk_users_capped", "nr_topk_users_capped_workspace_bytes"]
    for f in fns:
        assert hasattr(lib, f), f
    assert int(re.search(r"#define NR_CAP_GROUPS_MAX (\d+)", text).group(1)) == _lib.NR_CAP_GROUPS_MAX == 1024
    P, L = ctypes.c_void_p, ctypes.c_int64
    # news_group and cap behind user_gain, everything else nr_topk_users_prior's in its order
    a, b = _lib.PRIOR_SIGNATURES["nr_topk_users_prior"][1], _lib.CAPS_SIGNATURES["nr_topk_users_capped"][1]
    assert b[:17] == a[:17] and b[17:19] == [P, L] and b[19:] == a[17:]
    assert (_lib.CAPS_SIGNATURES["nr_topk_users_capped_workspace_bytes"]
            == _lib.PRIOR_SIGNATURES["nr_topk_users_prior_workspace_bytes"])
    assert "newsrec_caps.h" in [p.name for p in _lib.hip_source_files()]
    assert "caps.hip" in [p.name for p in _lib.hip_source_files()]
    mk = (REPO / "news_recommendation_project_v2_amd" / "csrc" / "Makefile").read_text()
    assert "newsrec_caps.h" in mk and "caps.hip" in mk


def test_caps_workspace_bytes(lib):
    for dt in (F32, BF16):
        for U, N, K in ((1, 1, 1), (130, 16384 + 300, 64), (5000, 100000, 10)):
            assert (lib.nr_topk_users_capped_workspace_bytes(dt, U, N, K)
                    == lib.nr_topk_users_prior_workspace_bytes(dt, U, N, K))
    for bad in ((2, 4, 100, 5), (F32, 0, 100, 5), (F32, 1 << 31, 100, 5), (F32, 4, 0, 5), (F32, 4, (1 << 22) + 1, 5),
                (F32, 4, 100, 0), (F32, 4, 100, 65)):
        assert lib.nr_topk_users_capped_workspace_bytes(*bad) == -1, bad


def test_caps_refusals_on_the_host(lib):
    """Every refusal returns its code and message before any device call (this host has no
    device; a launch would fail differently)."""
    raw = np.zeros(1 << 20, dtype=np.uint8)
    P = raw.ctypes.data + (-raw.ctypes.data) % 256
    WS = 1 << 40
    err = lambda: lib.nr_last_error().decode()

    def call(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=None, qm=None, pr=None, ga=None, grp=P, cap=2, K=5, ti=P, ts=P, tk=None, ws=P,
             wsb=WS):
        return lib.nr_topk_users_capped(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, pr, ga,
                                        grp, cap, K, ti, ts, tk, ws, wsb, None)

    # this entry's own
    for cap in (0, -1, 65):
        assert call(cap=cap) == INVALID and f"cap = {cap} outside [1, 64]" in err()
    assert call(grp=None) == INVALID and "news_group is required" in err()
    assert "nr_topk_users_capped" in err()
    assert call() == INVALID and "not device memory" in err()  # a host news_group among them
    assert call(cap=64, K=5) == INVALID and "not device memory" in err()  # cap >= K: refused here, not by the base
    # the base entry's, with its codes and messages
    for half in ({"pr": P}, {"ga": P}):
        assert call(**half) == INVALID and "news_prior and user_gain go together" in err(), half
    for half in ({"nt": P}, {"lo": P, "hi": P}):
        assert call(**half) == INVALID and "news_time, q_time_lo and q_time_hi go together" in err(), half
    for half in ({"nc": P}, {"qm": P}):
        assert call(**half) == INVALID and "news_cat and q_cat_mask go together" in err(), half
    assert call(dim=512) == UNSUPPORTED and "dim 512 unsupported" in err()
    assert call(dtype=_lib.NR_F16) == INVALID and "bad dtype" in err()
    assert call(U=0) == INVALID and "U = 0" in err()
    assert call(N=0) == INVALID and "N = 0 < 1" in err()
    assert call(N=(1 << 22) + 1) == UNSUPPORTED and "unsupported" in err()
    assert call(ld=1016) == INVALID and "cand_ld = 1016 < dim" in err()
    assert call(table=P + 4) == INVALID and "16-byte" in err()
    assert call(eidx=P) == INVALID and "excl_idx and excl_off go together" in err()
    for k in (0, -1, 65):
        assert call(K=k) == INVALID and f"K = {k} outside [1, 64]" in err()
    for null in ("users", "table", "inv", "ws", "ti", "ts"):
        assert call(**{null: None}) == INVALID and "null pointer" in err(), null
    # top_keys: required with a prior only
    assert call(pr=P, ga=P, tk=None) == INVALID and "null pointer" in err()
    assert call(pr=P, ga=P, tk=P) == INVALID and "not device memory" in err()
    assert call(ws=P + 16) == INVALID and "256-byte aligned" in err()
    need = lib.nr_topk_users_capped_workspace_bytes(F32, 4, 100, 5)
    assert call(wsb=need - 1) == INVALID and "workspace too small" in err()
    assert call(wsb=need) == INVALID and "not device memory" in err()


# ------------------------------------------------------------------ the Python layers
def test_ops_caps_checks_on_the_host():
    import torch
    from news_recommendation_project_v2_amd import ops
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.topk_users_capped(torch.zeros(2, 1024), torch.zeros(5, 1024), torch.ones(5), 3,
                              torch.zeros(5, dtype=torch.int16), 2)
    g = torch.tensor([0, 5, 1023, 7, 7], dtype=torch.int16)
    assert ops._check_groups("t", 5, g, 3) == 3
    for bad in (g[:4], g.int(), g.reshape(5, 1), g.tolist()):
        with pytest.raises(_lib.NewsRecHIPError, match=r"news_group must be contiguous 16-bit integers \[5\]"):
            ops._check_groups("t", 5, bad, 3)
    for bad in (torch.tensor([0, 1, 1024, 2, 3], dtype=torch.int16), torch.tensor([0, -1, 4, 2, 3], dtype=torch.int16)):
        with pytest.raises(_lib.NewsRecHIPError, match=r"labels must lie in \[0, 1024\)"):
            ops._check_groups("t", 5, bad, 3)
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(_lib.NewsRecHIPError, match="cap = .* outside"):
            ops._check_groups("t", 5, g, bad)
    with pytest.raises(_lib.NewsRecHIPError, match="unsupported shape"):
        ops.topk_users_capped_workspace_bytes(torch.float32, 4, 100, 65)
    assert (ops.topk_users_capped_workspace_bytes(torch.bfloat16, 4, 100, 16)
            == ops.topk_users_prior_workspace_bytes(torch.bfloat16, 4, 100, 16))


def test_engine_and_helper_refuse_bad_caps_on_the_host():
    """The argument checks run ahead of any device work: no GPU is needed to be refused."""
    import torch
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd import engine
    eng = engine.PoolScoreEngine.__new__(engine.PoolScoreEngine)
    eng.news_cat = eng.news_time = eng.news_prior = eng.news_group = None
    eng.device = torch.device("cpu")
    eng.cand_table = torch.zeros(10, 1024)
    eng.n_imp, eng.user_idx = 3, None
    for bad in (np.r_[np.zeros(9, np.int64), 1024], np.r_[np.zeros(9, np.int64), -1]):
        with pytest.raises(ValueError, match=r"labels must lie in \[0, 1024\)"):
            eng.set_catalogue(news_group=bad)
    for bad in (np.zeros(9, np.int64), np.zeros((10, 1), np.int64), 3):
        with pytest.raises(ValueError, match=r"one entry per news \(10\)"):
            eng.set_catalogue(news_group=bad)
    with pytest.raises(ValueError, match="integer labels"):
        eng.set_catalogue(news_group=np.zeros(10))
    assert eng.news_group is None
    with pytest.raises(ValueError, match=r"group_cap needs set_catalogue\(news_group"):
        eng.recommend(4, group_cap=2)
    eng.set_catalogue(news_group=torch.arange(10, dtype=torch.int64) % 3)  # a tensor is taken too
    assert eng.news_group.dtype == torch.int16 and eng.news_group.tolist() == [0, 1, 2] * 3 + [0]
    ids, _ = data_utils.dense_groups(list("abcabcabca"))
    eng.set_catalogue(news_group=ids)
    assert eng.news_group.tolist() == [0, 1, 2] * 3 + [0]
    for bad in (0, 65, 2.0, True, "2"):
        with pytest.raises(ValueError, match="group_cap = .* must be an integer in 1 .. 64"):
            eng.recommend(4, group_cap=bad)
    # the modes without caps name the argument (recommend_explained takes neither it nor prior_gain)
    eng.news_cat = torch.zeros(10, dtype=torch.uint8)
    for call in (lambda: eng.recommend_sections(2, [[0], [1]], group_cap=2),
                 lambda: eng.recommend_diverse(4, 0.5, group_cap=2),
                 lambda: eng.rank_targets([], [0, 0, 0], group_cap=2),
                 lambda: eng.recommend_explained_filtered(4, group_cap=2)):
        with pytest.raises(ValueError, match="group_cap"):
            call()
    eng.set_catalogue()  # None drops the attribute
    assert eng.news_group is None
    # get_top_k_recommendations
    table, hist, hl = torch.zeros(10, 1024), np.zeros(3, np.int32), np.ones(3, np.int32)
    top = lambda **kw: dmh.get_top_k_recommendations(hist, hl, table, None, 4, **kw)
    grp = np.arange(10) % 3
    for kw in ({"groups": grp}, {"group_cap": 2}):
        with pytest.raises(ValueError, match="groups and group_cap go together"):
            top(**kw)
    for kw in ({"sections": [[0], [1]]}, {"diversify": 0.5}, {"explain": 2}, {"diversify": 0.5, "pool": 32}):
        with pytest.raises(ValueError, match="group_cap cannot be combined with sections, diversify or explain"):
            top(groups=grp, group_cap=2, **kw)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 1024\)"):
        top(groups=np.arange(10) + 1020, group_cap=2)
    with pytest.raises(ValueError, match=r"one entry per news \(10\)"):
        top(groups=grp[:9], group_cap=2)
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match="group_cap = .* must be an integer in 1 .. 64"):
            top(groups=grp, group_cap=bad)
