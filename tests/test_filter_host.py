"""The catalogue-filter entries of the C ABI (include/newsrec_filter.h) on the host:
signature table, the refusals that need no device, the float64 reference of the GPU
tests (tests/filter_ref.py) against brute force, and the host helpers of time-aware
retrieval (data_utils.catalogue_first_seen, data_utils.read_behavior_times,
synthetic.catalogue_attributes)."""
import ctypes
import io
import re

import numpy as np
import pytest

import filter_ref
import fullrank_ref
import topk_ref
from conftest import REPO
from news_recommendation_project_v2_amd import _lib, data_utils, synthetic

HEADER = REPO / "include" / "newsrec_filter.h"
F32, BF16 = _lib.NR_F32, _lib.NR_BF16
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.is_file():
        pytest.skip("libnewsrec_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_filter_signatures_cover_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(nr_[a-z0-9_]+)\s*\(", text)))
    assert fns == sorted(_lib.FILTER_SIGNATURES) == ["nr_rank_targets_filtered", "nr_topk_users_filtered"]
    for f in fns:
        assert hasattr(lib, f), f
    # five pointers more than the unfiltered entries, in the same places
    for plain, flt in (("nr_topk_users", "nr_topk_users_filtered"), ("nr_rank_targets", "nr_rank_targets_filtered")):
        a = {**_lib.TOPK_SIGNATURES, **_lib.FULLRANK_SIGNATURES}[plain][1]
        b = _lib.FILTER_SIGNATURES[flt][1]
        assert b[:10] == a[:10] and b[15:] == a[10:] and all(t is ctypes.c_void_p for t in b[10:15])
        assert len(b) == len(a) + 5
    names = [p.name for p in _lib.hip_source_files()]
    assert "newsrec_filter.h" in names
    mk = (REPO / "news_recommendation_project_v2_amd" / "csrc" / "Makefile").read_text()
    assert "newsrec_filter.h" in mk


def test_filter_refusals_on_the_host(lib):
    """Every refusal of the contract returns its code and message before any device call
    (this host has none; a launch would fail differently)."""
    raw = np.zeros(1 << 20, dtype=np.uint8)
    P = raw.ctypes.data + (-raw.ctypes.data) % 256
    WS = 1 << 40
    err = lambda: lib.nr_last_error().decode()

    def topk(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=None, qm=None, K=5, ti=P, ts=P, ws=P, wsb=WS):
        return lib.nr_topk_users_filtered(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, K,
                                          ti, ts, ws, wsb, None)

    def rank(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=None, qm=None, T=6, tidx=P, toff=P, out=P, ws=P, wsb=WS):
        return lib.nr_rank_targets_filtered(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, T,
                                            tidx, toff, out, ws, wsb, None)

    for call, name in ((topk, "nr_topk_users_filtered"), (rank, "nr_rank_targets_filtered")):
        # the pairing rule
        for half in ({"nt": P}, {"lo": P}, {"hi": P}, {"nt": P, "lo": P}, {"nt": P, "hi": P}, {"lo": P, "hi": P}):
            assert call(**half) == INVALID and "news_time, q_time_lo and q_time_hi go together" in err(), half
            assert name in err()
        for half in ({"nc": P}, {"qm": P}):
            assert call(**half) == INVALID and "news_cat and q_cat_mask go together" in err(), half
        assert call(nt=P, lo=P, hi=P, nc=P) == INVALID and "news_cat and q_cat_mask go together" in err()
        # the unfiltered entries' refusals
        assert call(dim=512) == UNSUPPORTED and "dim 512 unsupported" in err()
        assert call(dtype=_lib.NR_F16) == INVALID and "bad dtype" in err()
        assert call(U=0) == INVALID and "U = 0" in err()
        assert call(N=0) == INVALID and "N = 0 < 1" in err()
        assert call(N=(1 << 22) + 1) == UNSUPPORTED and "unsupported" in err()
        assert call(ld=1016) == INVALID and "cand_ld = 1016 < dim" in err()
        assert call(ld=1026) == INVALID and "16-byte" in err()
        assert call(dtype=BF16, ld=1028) == INVALID and "16-byte" in err()
        assert call(table=P + 4) == INVALID and "16-byte" in err()
        assert call(eidx=P) == INVALID and "excl_idx and excl_off go together" in err()
        assert call(eoff=P) == INVALID and "excl_idx and excl_off go together" in err()
        for null in ("users", "table", "inv", "ws"):
            assert call(**{null: None}) == INVALID and "null pointer" in err(), null
        assert call(ws=P + 16, wsb=WS) == INVALID and "256-byte aligned" in err()
        # host pointers, filter pointers included, stop at the residency check
        assert call() == INVALID and "not device memory" in err()
        assert call(nt=P, lo=P, hi=P, nc=P, qm=P) == INVALID and "not device memory" in err()
    for k in (0, -1, 65):
        assert topk(K=k) == INVALID and f"K = {k} outside [1, 64]" in err()
    for null in ("ti", "ts"):
        assert topk(**{null: None}) == INVALID and "null pointer" in err(), null
    need = lib.nr_topk_workspace_bytes(F32, 4, 100, 5)
    assert topk(wsb=need - 1) == INVALID and "workspace too small" in err()
    assert topk(wsb=need, nt=P, lo=P, hi=P) == INVALID and "not device memory" in err()  # the filter needs no workspace
    assert rank(T=-1) == INVALID and "T = -1" in err()
    for null in ("tidx", "toff", "out"):
        assert rank(**{null: None}) == INVALID and "null pointer" in err(), null
    need = lib.nr_rank_targets_workspace_bytes(F32, 4, 100, 6)
    assert rank(wsb=need - 1) == INVALID and "workspace too small" in err()
    assert rank(wsb=need, nc=P, qm=P) == INVALID and "not device memory" in err()


def test_ops_filter_checks_on_the_host():
    """ops refuses non-device tensors (no CPU fallback) before anything else."""
    import torch
    from news_recommendation_project_v2_amd import ops
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.topk_users_filtered(torch.zeros(2, 1024), torch.zeros(5, 1024), torch.ones(5), 3,
                                news_time=torch.zeros(5, dtype=torch.int32))
    assert ops._check_filter("t", 2, 5, None, None, None, None, None) == [None] * 5
    t5, t2 = torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.NewsRecHIPError, match="go together"):
        ops._check_filter("t", 2, 5, t5, t2, None, None, None)
    with pytest.raises(_lib.NewsRecHIPError, match="go together"):
        ops._check_filter("t", 2, 5, None, None, None, torch.zeros(5, dtype=torch.uint8), None)
    with pytest.raises(_lib.NewsRecHIPError, match="time_hi must be contiguous torch.int32 \\[2\\]"):
        ops._check_filter("t", 2, 5, t5, t2, t5, None, None)
    with pytest.raises(_lib.NewsRecHIPError, match="news_cat must be contiguous torch.uint8"):
        ops._check_filter("t", 2, 5, None, None, None, t5, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_lib.NewsRecHIPError, match="cat_mask must be contiguous torch.int64"):
        ops._check_filter("t", 2, 5, None, None, None, torch.zeros(5, dtype=torch.uint8), t2)
    assert len(ops._check_filter("t", 2, 5, t5, t2, t2, torch.zeros(5, dtype=torch.uint8),
                                 torch.zeros(2, dtype=torch.int64))) == 5


# ------------------------------------------------------------------ the reference against brute force
def test_filter_ref_matches_brute_force():
    rng = np.random.default_rng(11)
    seen = {"empty": 0, "cat64": 0, "short": 0, "minus1": 0}
    for i in range(24):
        U, N, K = int(rng.integers(1, 6)), int(rng.integers(1, 40)), int(rng.integers(1, 12))
        s = rng.standard_normal((U, N))
        if i % 2 == 0:
            s = np.round(s * 2) / 2  # ties
        news_time = rng.integers(-50, 50, N).astype(np.int32) if i % 3 != 1 else None
        lo = rng.integers(-60, 40, U).astype(np.int32)
        hi = (lo + rng.integers(-5, 60, U)).astype(np.int32)
        news_cat = rng.integers(0, 80, N).astype(np.uint8) if i % 3 != 2 else None
        mask = rng.integers(0, 1 << 63, U, dtype=np.uint64) | (rng.integers(0, 2, U).astype(np.uint64) << np.uint64(63))
        if i % 4 == 0:
            mask[0] = 0
        elig = filter_ref.eligible(U, N, news_time, lo, hi, news_cat, mask)
        assert np.array_equal(elig, filter_ref.eligible_brute(U, N, news_time, lo, hi, news_cat, mask)), i
        seen["empty"] += int(news_time is not None and (lo > hi).any())
        seen["cat64"] += int(news_cat is not None and (news_cat >= 64).any())
        eidx = eoff = None
        if i % 2:
            lens = rng.integers(0, 5, U)
            eoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            eidx = rng.integers(0, N, int(lens.sum())).astype(np.int32)
        # top-K and ranks on the equivalent exclusion lists == a plain sort of the eligible rows
        gi, gs = filter_ref.topk(s, K, elig, eidx, eoff)
        toff = np.arange(U + 1, dtype=np.int64) * N
        tidx = np.tile(np.arange(N, dtype=np.int32), U)
        gr = filter_ref.rank_targets(s, tidx, toff, elig, eidx, eoff).reshape(U, N)
        for u in range(U):
            banned = set() if eidx is None else {int(r) for r in eidx[eoff[u]:eoff[u + 1]]}
            order = sorted((-float(s[u, r]), r) for r in range(N) if elig[u, r] and r not in banned)
            rows = [r for _, r in order]
            assert gi[u, :len(rows[:K])].tolist() == rows[:K] and (gi[u, len(rows[:K]):] == -1).all(), (i, u)
            assert np.isneginf(gs[u, len(rows[:K]):]).all()
            place = {r: j for j, r in enumerate(rows)}
            assert gr[u].tolist() == [place.get(r, -1) for r in range(N)], (i, u)
            seen["short"] += int(len(rows) < K)
            seen["minus1"] += int(len(rows) < N)
    assert all(v > 0 for v in seen.values()), seen
    # the helper appends to a user's own list and keeps it
    elig = np.array([[True, False, True], [True, True, True]])
    idx, off = filter_ref.as_exclusions(elig, np.array([2, 2, 0], np.int32), np.array([0, 2, 3], np.int64))
    assert idx.tolist() == [2, 2, 1, 0] and off.tolist() == [0, 3, 4]
    assert topk_ref.topk(np.zeros((2, 3)), 2, idx, off)[0].tolist() == [[0, -1], [1, 2]]
    assert fullrank_ref.rank_targets(np.zeros((2, 3)), np.array([0, 1], np.int32), np.array([0, 2, 2], np.int64), idx,
                                     off).tolist() == [0, -1]


# ------------------------------------------------------------------ first-seen times, the Time column
def test_catalogue_first_seen_matches_a_loop():
    rng = np.random.default_rng(3)
    n_news, n_imp = 60, 25
    hl = rng.integers(0, 6, n_imp)
    cl = rng.integers(1, 7, n_imp)
    ci = rng.integers(0, n_news - 3, int(cl.sum())).astype(np.int32)
    when = rng.integers(-1000, 100000, n_imp).astype(np.int32)  # not sorted: the minimum is what counts
    hl[4] = max(hl[4], 1)
    hi = rng.integers(0, n_news - 3, int(hl.sum())).astype(np.int32)
    hi[int(hl[:4].sum())] = n_news - 2  # a news seen only in a history; news n_news - 1 and n_news - 3 nowhere
    ci[ci == n_news - 2] = 0
    got = data_utils.catalogue_first_seen(when, hi, hl, ci, cl, n_news)
    want = [np.iinfo(np.int32).max] * n_news
    ho, co = np.concatenate([[0], np.cumsum(hl)]), np.concatenate([[0], np.cumsum(cl)])
    for i in range(n_imp):
        for r in list(hi[ho[i]:ho[i + 1]]) + list(ci[co[i]:co[i + 1]]):
            want[r] = min(want[r], int(when[i]))
    assert got.dtype == np.int32 and got.tolist() == want
    assert got[n_news - 2] == when[4] and got[n_news - 1] == np.iinfo(np.int32).max == got[n_news - 3]
    with pytest.raises(ValueError):
        data_utils.catalogue_first_seen(when[:-1], hi, hl, ci, cl, n_news)
    with pytest.raises(IndexError):
        data_utils.catalogue_first_seen(when, hi, hl, ci, cl, n_news - 2)


def test_read_behavior_times():
    text = ("7\tU13740\t11/11/2019 9:05:58 AM\tN55189 N42782\tN55689-1 N35729-0\n"
            "3\tU91836\t11/12/2019 6:11:30 PM\t\tN20678-0 N39317-1\n"
            "9\tU73700\t11/11/2019 12:00:00 AM\tN10732\tN50014-0\n")
    ids, secs = data_utils.read_behavior_times(io.StringIO(text))
    assert ids.tolist() == [7, 3, 9] and secs.dtype == np.int32
    assert secs.tolist() == [9 * 3600 + 5 * 60 + 58, 86400 + 18 * 3600 + 11 * 60 + 30, 0]


# ------------------------------------------------------------------ synthetic attributes
def test_synthetic_attributes_leave_the_set_unchanged():
    before = synthetic.mind_impressions(500, 300, seed=1234, users=40)
    when, cats = synthetic.catalogue_attributes(500, 300, seed=1234)
    after = synthetic.mind_impressions(500, 300, seed=1234, users=40)
    for name in ("hist_idx", "hist_len", "cand_idx", "cand_len", "labels"):
        a, b = getattr(before, name), getattr(after, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    # pinned: the set the earlier tests and benchmarks use (first rows of the seed-1234 draw)
    plain = synthetic.mind_impressions(500, 300, seed=1234)
    assert np.array_equal(plain.cand_idx, before.cand_idx) and np.array_equal(plain.labels, before.labels)
    assert when.dtype == np.int32 and when.shape == (300,) and (np.diff(when) >= 0).all()
    assert 0 <= when.min() and when.max() < 7 * 86400
    assert cats.dtype == np.uint8 and cats.shape == (500,) and cats.max() < 18 and len(np.unique(cats)) == 18
    again = synthetic.catalogue_attributes(500, 300, seed=1234)
    assert np.array_equal(again[0], when) and np.array_equal(again[1], cats)
    other = synthetic.catalogue_attributes(500, 300, seed=1235)
    assert not np.array_equal(other[0], when)
