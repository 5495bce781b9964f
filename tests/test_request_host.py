"""The request path of retrieval (include/newsrec_request.h) on the host: the C entry's
signature, its run length and workspace functions, the refusals that need no device, and the
Python layers' argument checks."""
import inspect
import re

import numpy as np
import pytest

from conftest import REPO
from news_recommendation_project_v2_amd import _lib

HEADER = REPO / "include" / "newsrec_request.h"
F32, BF16 = _lib.NR_F32, _lib.NR_BF16
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------ the C entry
def test_request_signatures_cover_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(nr_[a-z0-9_]+)\s*\(", text)))
    assert fns == sorted(_lib.REQUEST_SIGNATURES) == ["nr_topk_request", "nr_topk_request_run_rows",
                                                      "nr_topk_request_workspace_bytes"]
    for f in fns:
        assert hasattr(lib, f), f
        assert getattr(lib, f).argtypes == _lib.REQUEST_SIGNATURES[f][1], "load() binds the table"
        assert getattr(lib, f).restype == _lib.REQUEST_SIGNATURES[f][0]
    # exactly nr_topk_users_after's argument list, names included
    assert _lib.REQUEST_SIGNATURES["nr_topk_request"] == _lib.PAGE_SIGNATURES["nr_topk_users_after"]
    assert (_lib.REQUEST_SIGNATURES["nr_topk_request_workspace_bytes"]
            == _lib.PAGE_SIGNATURES["nr_topk_users_after_workspace_bytes"])
    page = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "newsrec_page.h").read_text(), flags=re.S)
    args = lambda t, fn: re.sub(r"\s+", " ", re.search(r"int %s\((.*?)\);" % fn, t, flags=re.S).group(1))
    assert args(text, "nr_topk_request") == args(page, "nr_topk_users_after")
    assert re.search(r"#define NR_REQUEST_MAX_USERS 32\b", text) and _lib.NR_REQUEST_MAX_USERS == 32
    assert _lib.NR_TOPK_MAX == 64 and lib.nr_topk_chunk_rows() == 16384, "the existing entries keep their limits"
    names = [p.name for p in _lib.hip_source_files()]
    assert "newsrec_request.h" in names and "request.hip" in names
    mk = (REPO / "news_recommendation_project_v2_amd" / "csrc" / "Makefile").read_text()
    assert "newsrec_request.h" in mk and "request.hip" in mk


def test_request_run_rows(lib):
    rr = lib.nr_topk_request_run_rows
    assert rr(72023) == 288 and -(-72023 // 288) == 251
    assert rr(1 << 22) == 16384
    assert rr(16384 + 300) == 96 and -(-(16384 + 300) // 96) == 174
    for n in (1, 31, 32, 33, 1000, 8191, 8192):
        assert rr(n) == 32, n
    assert rr(8193) == 64
    rng = np.random.default_rng(0)
    for n in [1, 2, 8192, 8193, 16384, 72023, (1 << 22) - 1, 1 << 22] + rng.integers(1, 1 << 22, 200).tolist():
        r = rr(n)
        assert r >= 32 and r % 32 == 0 and -(-n // r) <= 256, n
        assert r == 32 or -(-n // (r - 32)) > 256, "the shortest such run"


def test_request_workspace_bytes(lib):
    ws = lib.nr_topk_request_workspace_bytes
    for bad in ((2, 4, 100, 5), (F32, 0, 100, 5), (F32, 33, 100, 5), (F32, 4, 0, 5), (F32, 4, (1 << 22) + 1, 5),
                (F32, 4, 100, 0), (F32, 4, 100, 65), (BF16, 4, 100, -1), (BF16, 1 << 31, 100, 5), (-1, 4, 100, 5)):
        assert ws(*bad) == -1, bad
    a256 = lambda b: (b + 255) // 256 * 256
    for dt in (F32, BF16):
        for U in (1, 5, 16, 17, 32):
            for N in (1, 1000, 16384 + 300, 72023, 1 << 22):
                for K in (1, 10, 64):
                    R = -(-N // lib.nr_topk_request_run_rows(N))
                    want = 2 * a256(4 * U) + a256(8 * (U + 1)) + a256(8 * U * R * K) + a256(4 * U)
                    got = ws(dt, U, N, K)
                    assert got == want and got % 256 == 0, (dt, U, N, K)
    assert ws(F32, 32, 1 << 22, 64) < (4 << 20) + 4096, "about 4 MiB at the most"


def test_request_refusals_on_the_host(lib):
    """Every refusal returns nr_topk_users_after's code and message (under this entry's name)
    before any device call (this host has no device; a launch would fail differently)."""
    raw = np.zeros(1 << 20, dtype=np.uint8)
    P = raw.ctypes.data + (-raw.ctypes.data) % 256
    WS = 1 << 40
    err = lambda: lib.nr_last_error().decode()
    defaults = dict(dtype=F32, dim=1024, U=4, users=P, N=100, table=P, ld=1024, inv=P, eidx=None, eoff=None, nt=None,
                    lo=None, hi=None, nc=None, qm=None, pr=None, ga=None, ak=None, ar=None, nk=None, nr=None, K=7, ti=P,
                    ts=P, tk=None, ws=P, wsb=WS)

    def call(fn=None, **kw):
        a = dict(defaults)
        a.update(kw)
        return (fn or lib.nr_topk_request)(a["dtype"], a["dim"], a["U"], a["users"], a["N"], a["table"], a["ld"],
                                           a["inv"], a["eidx"], a["eoff"], a["nt"], a["lo"], a["hi"], a["nc"], a["qm"],
                                           a["pr"], a["ga"], a["ak"], a["ar"], a["nk"], a["nr"], a["K"], a["ti"],
                                           a["ts"], a["tk"], a["ws"], a["wsb"], None)

    for half in ({"ak": P}, {"ar": P}):
        assert call(**half) == INVALID and "after_key and after_row go together" in err(), half
    for half in ({"nk": P}, {"nr": P}):
        assert call(**half) == INVALID and "next_key and next_row go together" in err(), half
    assert err().startswith("nr_topk_request: ")
    assert call(ak=P, ar=P, nk=P, nr=P) == INVALID and "not device memory" in err()
    for null in ("users", "table", "inv", "ws", "ti", "ts"):
        assert call(**{null: None}) == INVALID and "null pointer" in err(), null
    # top_keys is nullable: the call gets as far as the device-pointer checks
    assert call(pr=P, ga=P, tk=None) == INVALID and "not device memory" in err()
    assert call(ws=P + 16) == INVALID and "256-byte aligned" in err()
    for k in (0, -1, 65, 256):
        assert call(K=k) == INVALID and f"nr_topk_request: K = {k} outside [1, 64]" in err()
    assert call(dim=512) == UNSUPPORTED and "dim 512 unsupported" in err()
    assert call(dtype=_lib.NR_F16) == INVALID and "bad dtype" in err()
    assert call(U=0) == INVALID and "U = 0" in err()
    assert call(N=0) == INVALID and "N = 0 < 1" in err()
    assert call(N=(1 << 22) + 1) == UNSUPPORTED and "unsupported" in err()
    # more users than the request path takes: the bulk entry is named
    for U in (33, 128, 100000):
        assert call(U=U) == UNSUPPORTED and err().startswith("nr_topk_request: U = %d unsupported" % U)
        assert "nr_topk_users_after" in err()
    assert call(U=32) == INVALID and "not device memory" in err(), "32 users get as far as the device checks"
    for U, N, K in ((1, 100, 5), (32, 72023, 64), (17, 1000, 10)):
        need = lib.nr_topk_request_workspace_bytes(F32, U, N, K)
        assert call(U=U, N=N, K=K, wsb=need - 1) == INVALID and f"workspace too small ({need - 1} < {need})" in err()
        assert call(U=U, N=N, K=K, wsb=need) == INVALID and "not device memory" in err()
    # the same call against the cursor entry: the same code, the same message behind the name
    # (a workspace that is too small names each entry's own size)
    cases = [{"ak": P}, {"ar": P}, {"nk": P}, {"nr": P}, {"dim": 512}, {"dtype": 2}, {"dtype": -1}, {"U": 0}, {"U": -3},
             {"N": 0}, {"N": (1 << 22) + 1}, {"K": 0}, {"K": 65}, {"ld": 1016}, {"ld": 1026}, {"table": P + 4},
             {"users": P + 8}, {"users": None}, {"table": None}, {"inv": None}, {"ti": None}, {"ts": None},
             {"ws": None}, {"ws": P + 16}, {"eidx": P}, {"eoff": P}, {"nt": P}, {"lo": P, "hi": P}, {"nc": P}, {"qm": P},
             {"pr": P}, {"ga": P}, {"ak": P, "ar": P, "nk": P, "nr": P}, {"pr": P, "ga": P}, {"wsb": 10}, {}]
    for kw in cases:
        rc, mine = call(**kw), err()
        rc2, theirs = call(lib.nr_topk_users_after, **kw), err()
        size = r"\(\d+ < \d+\)" if "wsb" in kw else None
        strip = (lambda s: re.sub(size, "", s)) if size else (lambda s: s)
        assert rc == rc2 != 0 and strip(mine) == strip(theirs.replace("nr_topk_users_after", "nr_topk_request")), kw


# ------------------------------------------------------------------ the Python layers
def test_ops_request_checks_on_the_host():
    import torch
    from news_recommendation_project_v2_amd import ops
    table, inv = torch.zeros(5, 1024), torch.ones(5)
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.topk_request(torch.zeros(2, 1024), table, inv, 3)
    with pytest.raises(_lib.NewsRecHIPError, match=r"topk_request: 33 users \(at most 32; topk_users_after takes more\)"):
        ops.topk_request(torch.zeros(33, 1024), table, inv, 3)
    for k in (0, 65):
        with pytest.raises(_lib.NewsRecHIPError, match=r"topk_request: unsupported shape .*k in \[1, 64\]"):
            ops.topk_request_workspace_bytes(torch.float32, 4, 100, k)
    with pytest.raises(_lib.NewsRecHIPError, match=r"topk_request: unsupported shape .*topk_users_after"):
        ops.topk_request_workspace_bytes(torch.float32, 33, 100, 5)
    assert ops.topk_request_workspace_bytes(torch.bfloat16, 32, 72023, 64) == \
        _lib.load().nr_topk_request_workspace_bytes(BF16, 32, 72023, 64)
    assert ([p for p in inspect.signature(ops.topk_request).parameters]
            == [p for p in inspect.signature(ops.topk_users_after).parameters if not p.startswith("_")])
    assert ([p.default for p in inspect.signature(ops.topk_request).parameters.values()]
            == [p.default for n, p in inspect.signature(ops.topk_users_after).parameters.items()
                if not n.startswith("_")])


def test_engine_request_checks_on_the_host(lib):
    """The argument checks run ahead of any device work: no GPU is needed to be refused."""
    import torch
    from news_recommendation_project_v2_amd import engine
    eng = engine.PoolScoreEngine.__new__(engine.PoolScoreEngine)
    eng.news_cat = eng.news_time = eng.news_prior = eng.news_group = None
    eng.device, eng.dtype = torch.device("cpu"), torch.float32
    eng.cand_table = eng.hist_src = torch.zeros(10, 1024)
    h = lambda *rows: np.array(rows, dtype=np.int64)
    with pytest.raises(ValueError, match=r"recommend_request: 33 histories \(at most 32; load_impressions and "
                                         r"recommend serve more\)"):
        eng.recommend_request([h(1)] * 33, 5)
    with pytest.raises(ValueError, match="at least one reader"):
        eng.recommend_request([], 5)
    with pytest.raises(ValueError, match="sequence of integer arrays"):
        eng.recommend_request(h(1, 2), 5)
    for bad in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match=r"recommend_request: k = .* must be an integer in 1 \.\. 64"):
            eng.recommend_request([h(1)], bad)
    with pytest.raises(IndexError, match="history index 10 is out of bounds for dimension 0 with size 10"):
        eng.recommend_request([h(1), h(3, 10)], 5)
    with pytest.raises(IndexError, match="history index -1 is out of bounds"):
        eng.recommend_request([h(-1)], 5)
    with pytest.raises(IndexError, match="exclude index 11 is out of bounds for dimension 0 with size 10"):
        eng.recommend_request([h(1), h()], 5, exclude=[h(), h(11)])
    with pytest.raises(ValueError, match="exclude must hold one array of rows per reader"):
        eng.recommend_request([h(1), h()], 5, exclude=[h()])
    with pytest.raises(ValueError, match="1-D integer arrays"):
        eng.recommend_request([np.array([0.5])], 5)
    with pytest.raises(ValueError, match=r"after must hold one \(key, row\) per impression \(2\)"):
        eng.recommend_request([h(1), h(2)], 5, after=(np.zeros(3, np.float32), np.zeros(3, np.int32)))
    with pytest.raises(ValueError, match="time_window needs set_catalogue"):
        eng.recommend_request([h(1)], 5, time_window=(0, 1))
    with pytest.raises(ValueError, match="categories needs set_catalogue"):
        eng.recommend_request([h(1)], 5, categories=1)
    with pytest.raises(ValueError, match="prior_gain needs set_catalogue"):
        eng.recommend_request([h(1)], 5, prior_gain=0.5)
    with pytest.raises(TypeError):
        eng.recommend_request([h(1)], 5, group_cap=2)
    assert ([p for p in inspect.signature(eng.recommend_request).parameters]
            == ["histories", "k", "exclude_history", "exclude", "time_window", "categories", "prior_gain", "want_keys",
                "after", "want_cursor"])
