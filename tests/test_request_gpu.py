"""The request path of top-K retrieval (include/newsrec_request.h; csrc/request.hip) on the GPU.

No test here uses a tolerance.  nr_topk_request promises nr_topk_users_after's outputs bit for
bit, so every comparison is torch.equal / np.array_equal on raw bits: against the bulk entry,
against itself under another grouping of users or another cut of the table into runs, or against
a planted case (tests/retrieval_cases.py) whose float64 reference scores are asserted >= 1e-2
apart on the CPU before any call.

Shapes, the smallest at which the kernel can go wrong: N = 1,000 (32 runs of 32 rows, the last
holds 8: a ragged final tile, and workgroups whose later waves have no tile), N = 16,384 + 300
(174 runs of 96 rows: one and a half rounds of bf16 tiles, three quarters of an f32 round, and
two chunks of the bulk kernel), U in {1, 5, 16, 17, 32} (one wave with users, the bf16 kernel's
one and two blocks of 16 users, every wave with 8), K in {1, 10, 64}.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import retrieval_cases
from news_recommendation_project_v2_amd import weights as W
from retrieval_cases import _csr, _model, _random_users_table

D = 1024
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
I32_MAX = np.iinfo(np.int32).max
N_SMALL, N_LARGE = 1000, 16384 + 300
US, KS = (1, 5, 16, 17, 32), (1, 10, 64)


def _run_rows(n):
    from news_recommendation_project_v2_amd import _lib
    return int(_lib.load().nr_topk_request_run_rows(n))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """Two (idx, scores, keys, next) results, bit for bit."""
    flat = lambda r: list(r[:3]) + (list(r[3]) if r[3] is not None else [])
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(fa, fb))


class Case(retrieval_cases.Case):
    def up(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def kw(self, U, excl=None, flt=None, prior=None, gain=None):
        """Host arrays of 32 users to the keyword arguments of the first U."""
        kw = {}
        for name, v in (flt or {}).items():
            kw[name] = self.up(v[:U] if name in ("time_lo", "time_hi", "cat_mask") else v)
        if excl is not None:
            kw.update(zip(("excl_idx", "excl_off"), _csr(excl[:U], self.dev)[2:]))
            kw["excl_checked"] = True  # the lists hold rows outside the table on purpose
        if prior is not None:
            kw.update(news_prior=self.up(prior), user_gain=self.up(gain[:U]))
        return kw

    def both(self, U, k, after=None, **kw):
        from news_recommendation_project_v2_amd import ops
        u = self.users[:U].contiguous()
        a = ops.topk_request(u, self.table, self.inv, k, after=after, **kw)
        b = ops.topk_users_after(u, self.table, self.inv, k, after=after, **kw)
        return a, b


@functools.lru_cache(maxsize=None)
def _case(dtype, n, dev):
    """32 random users (user 3 zero) against n random rows, and the host arrays of every
    configuration; built once per (dtype, n) and never written to."""
    rng, users, table = _random_users_table(32, n, seed=31 + n, zero_user=3)
    case = Case(users, table, dtype, dev, want_ref=False)
    r = _run_rows(n)
    excl = [rng.integers(0, n, m) for m in rng.integers(0, 12, 32)]
    # reader 0: 40 entries inside run 2 (more than 32, with duplicates), some outside the table
    excl[0] = np.concatenate([rng.integers(2 * r, 3 * r, 40), [-5, n, n + 7, I32_MAX, -I32_MAX], rng.integers(0, n, 9)])
    # reader 4: a few hundred, as a long history
    excl[4] = np.concatenate([rng.integers(0, n, 300), [n - 1, 0, n - 1]])
    excl[2] = np.zeros(0, np.int64)
    cat = rng.integers(0, 70, n).astype(np.uint8)  # 64 .. 69 never match
    cat[cat == 7] = 8
    cat[rng.permutation(n)[:6]] = 7                # category 7: six rows
    lo = rng.integers(0, 400, 32).astype(np.int32)
    hi = (lo + rng.integers(200, 600, 32)).astype(np.int32)
    lo[1], hi[1] = 500, 499                        # an empty window
    mask = rng.integers(1, 1 << 62, 32).astype(np.int64)
    mask[2] = 1 << 7                               # fewer than K rows for K = 10 and 64
    flt = dict(news_time=rng.integers(0, 1000, n).astype(np.int32), time_lo=lo, time_hi=hi, news_cat=cat, cat_mask=mask)
    prior = rng.random(n).astype(np.float32)
    gain = rng.uniform(-1.0, 2.0, 32).astype(np.float32)
    gain[0] = gain[5] = 0.0
    return case, excl, flt, prior, gain


# ------------------------------------------------------------------ 1. equal to the bulk entry, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [N_SMALL, N_LARGE])
@pytest.mark.parametrize("mode", ["plain", "excl", "filter", "prior", "all"])
def test_gpu_request_equals_bulk_entry(gpu_device, mode, n, dtype):
    case, excl, flt, prior, gain = _case(dtype, n, gpu_device)
    for U in US:
        kw = case.kw(U, excl if mode in ("excl", "all") else None, flt if mode in ("filter", "all") else None,
                     *((prior, gain) if mode in ("prior", "all") else (None, None)))
        for k in KS:
            got, want = case.both(U, k, **kw)
            assert _same(got, want), (U, k)
            idx = got[0].cpu().numpy()
            if mode == "plain":
                assert (idx >= 0).all() and got[3] is not None
            if mode in ("excl", "all"):
                for u in range(U):
                    assert not np.isin(idx[u][idx[u] >= 0], excl[u]).any(), (U, k, u)
            if mode == "filter" and U > 2:
                assert (idx[1] == -1).all(), "the empty window"
                assert (idx[2] >= 0).sum() == min(k, int(((flt["news_cat"] == 7) & (flt["news_time"] >= flt["time_lo"][2])
                                                           & (flt["news_time"] <= flt["time_hi"][2])).sum()))
            if mode == "all":  # and the page behind it, from the cursor either entry returned
                got2, want2 = case.both(U, k, after=want[3], **kw)
                assert _same(got2, want2), (U, k, "page 2")
                i2 = got2[0].cpu().numpy()
                for u in range(U):
                    assert not (set(idx[u][idx[u] >= 0]) & set(i2[u][i2[u] >= 0]))


# ------------------------------------------------------------------ 2. cursors
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_request_cursor_chain(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    case, _, flt, _, _ = _case(dtype, N_SMALL, gpu_device)
    U, k, dev = 3, 10, gpu_device
    users = case.users[[0, 1, 2]].contiguous()  # (no zero user: every row in the window has a finite key)
    t = flt["news_time"]
    window = dict(news_time=case.up(t), time_lo=case.up(np.array([100, 300, 0], np.int32)),
                  time_hi=case.up(np.array([144, 345, 40], np.int32)))
    eligible = [set(np.nonzero((t >= a) & (t <= b))[0].tolist()) for a, b in ((100, 144), (300, 345), (0, 40))]
    assert all(30 <= len(e) <= 70 for e in eligible)
    seen = [set() for _ in range(U)]
    cur, pages = None, 0
    while True:
        got = ops.topk_request(users, case.table, case.inv, k, after=cur, **window)
        want = ops.topk_users_after(users, case.table, case.inv, k, after=cur, **window)
        assert _same(got, want), pages
        idx = got[0].cpu().numpy()
        for u in range(U):
            rows = set(idx[u][idx[u] >= 0].tolist())
            assert not (rows & seen[u]), "pages are disjoint"
            seen[u] |= rows
        cur, pages = got[3], pages + 1
        ended = torch.isinf(cur[0]) & (cur[0] < 0) & (cur[1] == I32_MAX)
        if bool(ended.all()):
            break
        assert pages < 10
    assert seen == eligible and pages >= 4
    # behind the end cursor: nothing
    got = ops.topk_request(users, case.table, case.inv, k, after=cur, **window)
    assert bool((got[0] == -1).all()) and torch.equal(got[3][0], cur[0]) and torch.equal(got[3][1], cur[1])
    # a cursor of one entry continues identically in the other; a start cursor is no cursor
    p1r = ops.topk_request(users, case.table, case.inv, k, **window)
    p1a = ops.topk_users_after(users, case.table, case.inv, k, after=ops.start_cursor(U, dev), **window)
    assert _same(p1r, p1a)
    p2 = [fn(users, case.table, case.inv, k, after=c[3], **window)
          for fn in (ops.topk_request, ops.topk_users_after) for c in (p1r, p1a)]
    assert all(_same(p2[0], p) for p in p2[1:])
    # next_* may alias after_*
    at = (p1r[3][0].clone(), p1r[3][1].clone())
    alias = ops.topk_request(users, case.table, case.inv, k, after=at, next_out=at, **window)
    assert alias[3][0] is at[0] and _same(alias, p2[0])


# ------------------------------------------------------------------ 3. against float64, independent of the bulk kernel
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [10, 64])
def test_gpu_request_planted_exact(gpu_device, k, dtype):
    from news_recommendation_project_v2_amd import ops
    case, where, excl = retrieval_cases._planted(Case, k, 2000, dtype, gpu_device, seed=40 + k, n_users=3)
    _, _, eidx, eoff = _csr(excl, gpu_device)
    idx, scores, keys, _ = ops.topk_request(case.users, case.table, case.inv, k, excl_idx=eidx, excl_off=eoff)
    assert np.array_equal(idx.cpu().numpy(), where[:, :k]), "the planted rows, best first"
    off = torch.arange(4, dtype=torch.int64, device=gpu_device) * k
    want = ops.score_users(case.users, torch.arange(3, dtype=torch.int32, device=gpu_device), case.table, case.inv,
                           idx.reshape(-1).contiguous(), off, 3 * k)
    assert torch.equal(_bits(scores.reshape(-1)), _bits(want)) and torch.equal(_bits(keys), _bits(scores))


# ------------------------------------------------------------------ 4. ties and run boundaries
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_request_ties_across_runs(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    n = N_SMALL
    r = _run_rows(n)
    _, users, table = _random_users_table(5, n, seed=44)
    at = [r - 1, r, 2 * r - 1, 2 * r]
    table[at] = 3.0 * users[0]  # identical rows at cosine 1 with user 0, on both sides of two run boundaries
    case = Case(users, table, dtype, gpu_device, want_ref=False)
    idx, scores, _, _ = ops.topk_request(case.users, case.table, case.inv, 10)
    assert idx[0, :4].tolist() == at and len(set(_bits(scores[0, :4]).tolist())) == 1
    assert float(scores[0, 4]) < float(scores[0, 3])
    got, want = case.both(5, 2)
    assert got[0][0].tolist() == at[:2] and _same(got, want), "the lower two survive"
    assert got[3][1][0].item() == r, "and the cursor stands behind the second"
    nxt = ops.topk_request(case.users, case.table, case.inv, 2, after=got[3])
    assert nxt[0][0].tolist() == at[2:]


# ------------------------------------------------------------------ 5. position independence
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_request_position_independence(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    n, extra, k = 8000, 5000, 64
    assert _run_rows(n) == 32 and _run_rows(n + extra) == 64, "the extension is another cut into runs"
    rng, users, table = _random_users_table(32, n, seed=45)
    low = -2.0 * users[31] + 0.1 * rng.standard_normal((extra, D)).astype(np.float32)  # cosine near -1 with the reader
    case = Case(users, table, dtype, gpu_device, want_ref=False)
    big = Case(users, np.concatenate([table, low]), dtype, gpu_device, want_ref=False)
    prior = rng.random(n + extra).astype(np.float32)
    for pr in (None, prior):
        res = {}
        for name, c, rows in (("alone", case, [31]), ("last", case, list(range(32))), ("big", big, [31])):
            u = c.users[rows].contiguous()
            kw = {} if pr is None else dict(news_prior=c.up(pr[:c.N]),
                                            user_gain=torch.full((len(rows),), 0.01, device=gpu_device))
            idx, sc, ky, nxt = ops.topk_request(u, c.table, c.inv, k, **kw)
            res[name] = tuple(_bits(t[-1]) for t in (idx, sc, ky, nxt[0], nxt[1]))
        assert all(torch.equal(a, b) for a, b in zip(res["alone"], res["last"])), "row 31 of 32 users"
        assert all(torch.equal(a, b) for a, b in zip(res["alone"], res["big"])), "the extended table"
        assert int(res["big"][0].max()) < n


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_request_deterministic(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    case, excl, flt, prior, gain = _case(dtype, N_LARGE, gpu_device)
    kw = case.kw(32, excl, flt, prior, gain)
    a = ops.topk_request(case.users, case.table, case.inv, 64, **kw)
    b = ops.topk_request(case.users, case.table, case.inv, 64, **kw)
    assert _same(a, b) and a[0].data_ptr() != b[0].data_ptr()


# ------------------------------------------------------------------ 7. engine
@pytest.mark.gpu
@pytest.mark.parametrize("pooler,dtype", [("latent", torch.float32), ("final", torch.bfloat16),
                                          ("latent", torch.bfloat16), ("final", torch.float32)])
def test_gpu_engine_recommend_request(gpu_device, pooler, dtype):
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    rng = np.random.default_rng(47)
    n_news, k = 700, 9
    hists = [rng.integers(0, n_news, m).astype(np.int32) for m in (5, 1, 11, 0, 7, 3, 4)]
    hists[5] = hists[0].copy()  # two readers share a history; reader 3 is cold
    hl = np.array([len(h) for h in hists], dtype=np.int32)
    hi = np.concatenate(hists).astype(np.int32)
    eng = PoolScoreEngine(_model(pooler, gpu_device), dtype=dtype, device=gpu_device)
    eng.load_news(W.news_table(5, n_news, 1024, name="request"))
    eng.set_catalogue(news_time=rng.integers(0, 1000, n_news).astype(np.int32),
                      news_cat=rng.integers(0, 20, n_news).astype(np.uint8), news_prior=rng.random(n_news).astype(np.float32))
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(7, np.int32))
    same = lambda a, b: len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    lo, hi_t = np.array([0, 100, 0, 200, 0, 300, 600]), np.array([999, 700, 500, 900, 50, 800, 599])
    masks = [0xFFFFF, 0x3, 0xF0, 0xFFFFF, 0x1, 0xFF00, 0xFFFFF]
    gains = np.array([0.5, 0.0, -0.3, 1.5, 0.2, 0.5, 0.1], dtype=np.float32)
    assert same(eng.recommend_request(hists, k), eng.recommend(k))
    assert same(eng.recommend_request(hists, k, exclude_history=False), eng.recommend(k, exclude_history=False))
    assert same(eng.recommend_request(hists, 64), eng.recommend(64))
    assert same(eng.recommend_request(hists, k, time_window=(lo, hi_t), categories=masks),
                eng.recommend(k, time_window=(lo, hi_t), categories=masks))
    got = eng.recommend_request(hists, k, prior_gain=gains, want_keys=True)
    assert len(got) == 3 and same(got, eng.recommend(k, prior_gain=gains, want_keys=True))
    # two pages
    r1, b1 = eng.recommend_request(hists, k, want_cursor=True), eng.recommend(k, want_cursor=True)
    assert same(r1[:2], b1[:2]) and same(r1[2], b1[2])
    r2 = eng.recommend_request(hists, k, after=r1[2], want_cursor=True, want_keys=True)
    b2 = eng.recommend(k, after=b1[2], want_cursor=True, want_keys=True)
    assert same(r2[:3], b2[:3]) and same(r2[3], b2[3])
    p1, p2 = r1[0].cpu().numpy(), r2[0].cpu().numpy()
    assert all(not np.isin(p2[i], p1[i][p1[i] >= 0]).any() for i in range(7)), "the second page is disjoint"
    # the lists of a single reader are the lists it has among the seven
    one = eng.recommend_request([hists[2]], k)
    assert same([t[0] for t in one], [t[2] for t in r1[:2]])
    # exclude= removes exactly the listed rows
    base = eng.recommend_request(hists, k)[0].cpu().numpy()
    shown = [base[i][base[i] >= 0][:3] for i in range(7)]
    less = eng.recommend_request(hists, k, exclude=shown)[0].cpu().numpy()
    wide = eng.recommend_request(hists, k + 3)[0].cpu().numpy()
    for i in range(7):  # the rows left stay, and what moves up comes from the next three in selection order
        assert not np.isin(less[i], shown[i]).any()
        assert np.isin(np.setdiff1d(base[i], shown[i]), less[i]).all() and np.isin(less[i], wide[i]).all()
    # another table: prepare_requests builds its tables again
    of = eng._req_of
    eng.recommend_request(hists, k)
    assert eng._req_of == of, "nothing is rebuilt between calls on one table"
    eng.load_news(W.news_table(6, n_news, 1024, name="request-2"))
    assert same(eng.recommend_request(hists, k), eng.recommend(k))
    assert not np.array_equal(eng.recommend_request(hists, k)[0].cpu().numpy(), base)
    eng.cand_table.mul_(-1.0)  # written in place: the version moves
    assert same(eng.recommend_request(hists, k), eng.recommend(k))
