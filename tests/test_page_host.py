"""Cursors for top-K retrieval (include/newsrec_page.h) on the host: the float64 reference of
the GPU tests (tests/page_ref.py) against brute force -- concatenated pages are one long list;
the C entry's signature, workspace function and the refusals that need no device; the Python
layers' argument checks."""
import ctypes
import re

import numpy as np
import pytest

import page_ref
import topk_ref
from conftest import REPO
from news_recommendation_project_v2_amd import _lib

HEADER = REPO / "include" / "newsrec_page.h"
F32, BF16 = _lib.NR_F32, _lib.NR_BF16
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.is_file():
        pytest.skip("libnewsrec_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


# ------------------------------------------------------------------ the reference against brute force
def _csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    idx = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists]) if off[-1] else np.zeros(0, np.int32)
    return idx, off


def _pages_equal_one_list(s, k, P, excl=None):
    ei, eo = _csr(excl) if excl is not None else (None, None)
    got_i, got_s = page_ref.pages(s, k, P, ei, eo)
    want_i, want_s = topk_ref.brute_force(s, P * k, ei, eo)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
    return got_i


def test_page_ref_pages_are_one_brute_force_list():
    rng = np.random.default_rng(31)
    seen = {"tie_on_boundary": 0, "short": 0, "excluded": 0}
    for i in range(60):
        U, N, k, P = int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(1, 6)), int(rng.integers(1, 6))
        s = rng.standard_normal((U, N))
        if i % 2 == 0:
            s = np.round(s)  # heavy ties
        excl = None
        if i % 3 == 0:
            excl = [rng.integers(-1, N + 1, int(rng.integers(0, 5))) for _ in range(U)]
            seen["excluded"] += 1
        idx = _pages_equal_one_list(s, k, P, excl)
        seen["short"] += int((idx < 0).any())
        for p in range(1, P):
            a, b = idx[:, p * k - 1], idx[:, p * k]
            ok = b >= 0
            rows = np.arange(U)[ok]
            seen["tie_on_boundary"] += int((s[rows, a[ok]] == s[rows, b[ok]]).any())
    assert all(v > 5 for v in seen.values()), seen


def test_page_ref_named_cases():
    # a tie group straddling a page boundary: five equal best rows, pages of 2
    s = np.full((1, 12), -1.0)
    s[0, [1, 4, 6, 9, 10]] = 2.0
    s[0, 3] = 1.0
    idx = _pages_equal_one_list(s, 2, 3)
    assert idx.tolist() == [[1, 4, 6, 9, 10, 3]]
    # a zero user (all scores 0) with exclusions walks the eligible rows in row order
    z = np.zeros((1, 9))
    idx = _pages_equal_one_list(z, 3, 4, [[0, 4, 4, 8]])
    assert idx.tolist() == [[1, 2, 3, 5, 6, 7, -1, -1, -1, -1, -1, -1]]
    # a table shorter than P * k: the short page returns the end cursor, the page behind it is all pads
    rng = np.random.default_rng(2)
    s = rng.standard_normal((2, 7))
    _pages_equal_one_list(s, 3, 4)
    i1, _, c1 = page_ref.topk_after(s, 5)
    i2, t2, c2 = page_ref.topk_after(s, 5, *c1)
    assert (i2[:, 2:] == -1).all() and np.isneginf(t2[:, 2:]).all() and (i2[:, :2] >= 0).all()
    assert np.isneginf(c2[0]).all() and (c2[1] == np.iinfo(np.int32).max).all()
    i3, t3, c3 = page_ref.topk_after(s, 5, *c2)
    assert (i3 == -1).all() and np.isneginf(t3).all() and np.isneginf(c3[0]).all()
    # the start cursor is no cursor; a NaN key makes nothing eligible
    a = page_ref.topk_after(s, 4)
    b = page_ref.topk_after(s, 4, np.full(2, np.inf), np.full(2, -1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (page_ref.topk_after(s, 4, np.full(2, np.nan), np.zeros(2, np.int32))[0] == -1).all()
    # the cursor's own row is left out, an equal score with a larger row is not
    t = np.array([[3.0, 1.0, 3.0, 3.0]])
    assert page_ref.topk_after(t, 4, [3.0], [2])[0].tolist() == [[3, 1, -1, -1]]


# ------------------------------------------------------------------ the C entry
def test_page_signatures_cover_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(nr_[a-z0-9_]+)\s*\(", text)))
    assert fns == sorted(_lib.PAGE_SIGNATURES) == ["nr_topk_users_after", "nr_topk_users_after_workspace_bytes"]
    for f in fns:
        assert hasattr(lib, f), f
    P = ctypes.c_void_p
    # after_key, after_row, next_key, next_row behind user_gain, everything else nr_topk_users_prior's in its order
    a, b = _lib.PRIOR_SIGNATURES["nr_topk_users_prior"][1], _lib.PAGE_SIGNATURES["nr_topk_users_after"][1]
    assert b[:17] == a[:17] and b[17:21] == [P, P, P, P] and b[21:] == a[17:]
    assert _lib.PAGE_SIGNATURES["nr_topk_users_after"][0] == _lib.PRIOR_SIGNATURES["nr_topk_users_prior"][0]
    assert (_lib.PAGE_SIGNATURES["nr_topk_users_after_workspace_bytes"]
            == _lib.PRIOR_SIGNATURES["nr_topk_users_prior_workspace_bytes"])
    # the header's argument list, counted: one type per parameter
    proto = re.search(r"int nr_topk_users_after\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(b)
    names = [p.split()[-1].lstrip("*") for p in proto.split(",")]
    assert names[17:21] == ["after_key", "after_row", "next_key", "next_row"]
    assert "newsrec_page.h" in [p.name for p in _lib.hip_source_files()]
    mk = (REPO / "news_recommendation_project_v2_amd" / "csrc" / "Makefile").read_text()
    assert "newsrec_page.h" in mk
    assert _lib.NR_DEEP_MAX == 1024


def test_page_workspace_bytes(lib):
    for dt in (F32, BF16):
        for U, N, K in ((1, 1, 1), (130, 16384 + 300, 64), (5000, 100000, 10)):
            assert (lib.nr_topk_users_after_workspace_bytes(dt, U, N, K)
                    == lib.nr_topk_users_prior_workspace_bytes(dt, U, N, K) > 0)
    for bad in ((2, 4, 100, 5), (F32, 0, 100, 5), (F32, 1 << 31, 100, 5), (F32, 4, 0, 5), (F32, 4, (1 << 22) + 1, 5),
                (F32, 4, 100, 0), (F32, 4, 100, 65)):
        assert lib.nr_topk_users_prior_workspace_bytes(*bad) == -1, bad
        assert lib.nr_topk_users_after_workspace_bytes(*bad) == -1, bad


def test_page_refusals_on_the_host(lib):
    """Every refusal returns its code and message before any device call (this host has no
    device; a launch would fail differently)."""
    raw = np.zeros(1 << 20, dtype=np.uint8)
    P = raw.ctypes.data + (-raw.ctypes.data) % 256
    WS = 1 << 40
    err = lambda: lib.nr_last_error().decode()

    def call(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
             lo=None, hi=None, nc=None, qm=None, pr=None, ga=None, ak=None, ar=None, nk=None, nr=None, K=5, ti=P,
             ts=P, tk=None, ws=P, wsb=WS):
        return lib.nr_topk_users_after(dtype, dim, U, users, N, table, ld, inv, eidx, eoff, nt, lo, hi, nc, qm, pr, ga,
                                       ak, ar, nk, nr, K, ti, ts, tk, ws, wsb, None)

    # this entry's own
    for half in ({"ak": P}, {"ar": P}):
        assert call(**half) == INVALID and "after_key and after_row go together" in err(), half
    for half in ({"nk": P}, {"nr": P}):
        assert call(**half) == INVALID and "next_key and next_row go together" in err(), half
    assert "nr_topk_users_after" in err()
    for k in (0, -1, 65):
        assert call(K=k) == INVALID and f"K = {k} outside [1, 64]" in err()
        assert call(K=k, ak=P, ar=P, nk=P, nr=P) == INVALID and f"K = {k} outside [1, 64]" in err()
    # host pointers in the four new arrays are caught by the device-pointer checks
    assert call(ak=P, ar=P, nk=P, nr=P) == INVALID and "not device memory" in err()
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
    for null in ("users", "table", "inv", "ws", "ti", "ts"):
        assert call(**{null: None}) == INVALID and "null pointer" in err(), null
    # top_keys is nullable here, with a prior too: the call gets as far as the device-pointer checks
    assert call(pr=P, ga=P, tk=None) == INVALID and "not device memory" in err()
    assert call(ws=P + 16) == INVALID and "256-byte aligned" in err()
    for U, N, K in ((4, 100, 5), (300, 40000, 64)):
        need = lib.nr_topk_users_after_workspace_bytes(F32, U, N, K)
        assert call(U=U, N=N, K=K, wsb=need - 1) == INVALID and "workspace too small" in err()
        assert call(U=U, N=N, K=K, wsb=need) == INVALID and "not device memory" in err()


# ------------------------------------------------------------------ the Python layers
def test_ops_page_checks_on_the_host():
    import torch
    from news_recommendation_project_v2_amd import ops
    users, table, inv = torch.zeros(2, 1024), torch.zeros(5, 1024), torch.ones(5)
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.topk_users_after(users, table, inv, 3)
    key, row = ops.start_cursor(4, "cpu")
    assert key.dtype == torch.float32 and row.dtype == torch.int32 and key.tolist() == [float("inf")] * 4
    assert row.tolist() == [-1] * 4
    assert ops._check_cursor("t", "after", 4, None) == [None, None]
    assert [p.value for p in ops._check_cursor("t", "after", 4, (key, row))] == [key.data_ptr(), row.data_ptr()]
    for bad in ((key,), (row, key), (key[:3], row[:3]), (key.double(), row), (key, row.long()), (key[::2], row[::2]),
                key, (key.tolist(), row.tolist())):
        with pytest.raises(_lib.NewsRecHIPError, match=r"after must be \(key contiguous torch.float32 \[4\]"):
            ops._check_cursor("t", "after", 4, bad)
    with pytest.raises(_lib.NewsRecHIPError, match="unsupported shape"):
        ops.topk_users_after_workspace_bytes(torch.float32, 4, 100, 65)
    assert (ops.topk_users_after_workspace_bytes(torch.bfloat16, 4, 100, 16)
            == ops.topk_users_prior_workspace_bytes(torch.bfloat16, 4, 100, 16))


def test_engine_and_helper_refuse_bad_pages_on_the_host(lib):
    """The argument checks run ahead of any device work: no GPU is needed to be refused."""
    import torch
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd import engine
    eng = engine.PoolScoreEngine.__new__(engine.PoolScoreEngine)
    eng.news_cat = eng.news_time = eng.news_prior = eng.news_group = None
    eng.device, eng.dtype = torch.device("cpu"), torch.float32
    eng.cand_table = torch.zeros(10, 1024)
    eng.n_imp, eng.user_idx = 3, None
    cur = (np.full(3, np.inf, np.float32), np.full(3, -1, np.int32))
    eng.set_catalogue(news_group=np.arange(10) % 3, news_cat=np.zeros(10, np.int64))
    for kw in ({"after": cur}, {"want_cursor": True}, {"after": cur, "want_cursor": True}):
        with pytest.raises(ValueError, match="cannot be combined with group_cap"):
            eng.recommend(4, group_cap=2, **kw)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match=r"k = .* must be an integer in 1 \.\. 64 with a cursor"):
            eng.recommend(bad, after=cur)
    for bad in ((cur[0],), (cur[0][:2], cur[1][:2]), (cur[1], cur[0]), cur[0], None if False else "ab"):
        with pytest.raises(ValueError, match="after must"):
            eng.recommend(4, after=bad)
    # the modes without cursors name the argument
    for call in (lambda: eng.recommend_sections(2, [[0], [1]], after=cur),
                 lambda: eng.recommend_diverse(4, 0.5, after=cur),
                 lambda: eng.recommend_explained_filtered(4, after=cur)):
        with pytest.raises(ValueError, match="after is recommend's alone"):
            call()
    for bad in (0, 1025, -1, 10.0, True):
        with pytest.raises(ValueError, match=r"recommend_deep: k = .* must be an integer in 1 \.\. 1024"):
            eng.recommend_deep(bad)
    for bad in (0, 65, 2.5, False):
        with pytest.raises(ValueError, match=r"recommend_deep: page = .* must be an integer in 1 \.\. 64"):
            eng.recommend_deep(100, page=bad)
    with pytest.raises(TypeError):
        eng.recommend_deep(100, group_cap=2)
    # k = 65 without a cursor: still the entry's own refusal
    with pytest.raises(_lib.NewsRecHIPError, match=r"topk_users: unsupported shape .*k = 65; k in \[1, 64\]"):
        eng.recommend(65)
    # get_top_k_recommendations
    table, hist, hl = torch.zeros(10, 1024), np.zeros(3, np.int32), np.ones(3, np.int32)
    top = lambda k=4, **kw: dmh.get_top_k_recommendations(hist, hl, table, None, k, **kw)
    for kw in ({"sections": [[0], [1]]}, {"diversify": 0.5}, {"explain": 2}, {"diversify": 0.5, "pool": 32},
               {"groups": np.arange(10) % 3, "group_cap": 2}):
        with pytest.raises(ValueError, match="page cannot be combined with sections, diversify, explain or group_cap"):
            top(100, page=32, **kw)
    with pytest.raises(ValueError, match=r"k = 1025 must be an integer in 1 \.\. 1024"):
        top(1025, page=32)
    with pytest.raises(ValueError, match=r"k = 0 must be an integer in 1 \.\. 1024"):
        top(0, page=32)
    with pytest.raises(ValueError, match=r"page = 65 must be an integer in 1 \.\. 64"):
        top(100, page=65)
    with pytest.raises(ValueError, match=r"page = 0 must be an integer in 1 \.\. 64"):
        top(100, page=0)
    with pytest.raises(_lib.NewsRecHIPError, match=r"topk_users: unsupported shape .*k = 65; k in \[1, 64\]"):
        top(65)
