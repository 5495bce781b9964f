"""Cursors for top-K retrieval (include/newsrec_page.h; csrc/topk.hip) on the GPU.

No test here uses a tolerance.  Each is an exact identity between two GPU paths -- a page
against the exclusion route (the earlier pages on the exclusion lists of nr_topk_users*), the
union of the pages against one longer call, a deep list against the full-table ranks of an
independent kernel -- or a planted case (tests/retrieval_cases.py) whose reference scores are
asserted >= 1e-2 apart on the CPU before any call, against a selection error <= 1e-4
(tests/test_topk_gpu.py).

Shapes, the smallest at which the kernels can go wrong: N = 700 (five full tiles and a
partial one), N = one chunk + 300 (two workgroup runs side by side, a page boundary between
rows of different chunks), U = 65536 x N = two chunks + 77 (one workgroup walks several
chunks), N = k + 3 (short pages), both dtypes.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import retrieval_cases
from news_recommendation_project_v2_amd import weights as W
from retrieval_cases import _chunk, _csr, _model, _random_users_table

D = 1024
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
I32_MAX = np.iinfo(np.int32).max


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.view(np.int32) if a.dtype == np.float32 else a


class Case(retrieval_cases.Case):
    def _up(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def kw(self, excl=None, flt=None, prior=None, gain=None):
        """Host arrays to the keyword arguments the ops share."""
        kw = {k: self._up(v) for k, v in (flt or {}).items()}
        if excl is not None:
            kw.update(zip(("excl_idx", "excl_off"), _csr(excl, self.dev)[2:]))
        if prior is not None:
            kw.update(news_prior=self._up(prior), user_gain=self._up(gain))
        return kw

    def page(self, k, after=None, **kw):
        """One cursor call: (idx, score bits, key bits, (next key bits, next row)) on the host, the
        device cursor for the next call."""
        from news_recommendation_project_v2_amd import ops
        idx, sc, ky, nxt = ops.topk_users_after(self.users, self.table, self.inv, k, after=after, **kw)
        torch.cuda.synchronize()
        return (idx.cpu().numpy(), _bits(sc), _bits(ky), (_bits(nxt[0]), nxt[1].cpu().numpy())), nxt

    def walk(self, k, n_pages, **kw):
        out, cur = [], None
        for _ in range(n_pages):
            pg, cur = self.page(k, cur, **kw)
            out.append(pg)
        return out


def _random_case(dtype, dev, U=5, N=700, seed=21, zero_user=None):
    rng, users, table = _random_users_table(U, N, seed, zero_user)
    return rng, Case(users, table, dtype, dev, want_ref=False)


def _planted(*args, **kw):
    return retrieval_cases._planted(Case, *args, **kw)


def _rows(idx):
    return [set(r[r >= 0].tolist()) for r in idx]


# ------------------------------------------------------------------ 1. planted pages, exact
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_page_planted_exact(gpu_device, dtype):
    case, where, excl = _planted(24, 700, dtype, gpu_device, seed=24)
    assert where.shape == (3, 32)
    pages = case.walk(8, 5, **case.kw(excl))
    for p in range(4):
        assert np.array_equal(pages[p][0], where[:, 8 * p:8 * p + 8]), p
    last = pages[4][0]
    for u in range(3):  # only the background is left
        assert (last[u] >= 0).all() and not np.isin(last[u], where).any()


# ------------------------------------------------------------------ 2. a page == the exclusion route
def _page_equals_exclusion_route(case, k, n_pages, excl, flt=None, prior=None, gain=None, users=None):
    """Page p of a cursor walk against nr_topk_users / _filtered / _prior with the pages before
    it appended to the exclusion lists, bit for bit (rows ``users`` of the case: all)."""
    from news_recommendation_project_v2_amd import ops
    pages = case.walk(k, n_pages + 1, **case.kw(excl, flt, prior, gain))
    sel = np.arange(case.U) if users is None else np.asarray(users)
    small = case if users is None else case.rows(sel)
    lists = [np.asarray(excl[u], dtype=np.int64) for u in sel]
    pick = lambda d: None if d is None else {n: (v[sel] if n in ("time_lo", "time_hi", "cat_mask") else v)
                                             for n, v in d.items()}
    for p in range(n_pages + 1):
        idx = pages[p][0][sel]
        kw = small.kw(lists, pick(flt), prior, None if gain is None else gain[sel])
        if prior is not None:
            want = ops.topk_users_prior(small.users, small.table, small.inv, k, **kw)
        elif flt is not None:
            want = ops.topk_users_filtered(small.users, small.table, small.inv, k, **kw)
        else:
            want = ops.topk_users(small.users, small.table, small.inv, k, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(idx, want[0].cpu().numpy()), p
        assert np.array_equal(pages[p][1][sel], _bits(want[1])), p
        if prior is not None:
            assert np.array_equal(pages[p][2][sel], _bits(want[2])), p
        else:  # without a prior the keys are the scores
            assert np.array_equal(pages[p][2][sel], pages[p][1][sel]), p
        # the next cursor's row is one of the page's rows (its last in selection order); full pages here
        assert (idx >= 0).all() and all(r in row for r, row in zip(pages[p][3][1][sel], idx))
        lists = [np.concatenate([l, r]) for l, r in zip(lists, idx)]
    return pages


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", ["plain", "prior", "window"])
def test_gpu_page_equals_exclusion_route(gpu_device, mode, dtype):
    """k = 7, pages 0 .. 5: by page 5 a user has 35 rows on its list, more than the 32 the
    kernel stages per chunk and user, so the overflow path runs as well."""
    rng, case = _random_case(dtype, gpu_device)
    excl = [rng.integers(0, case.N, n) for n in (0, 3, 9, 1, 5)]
    flt = prior = gain = None
    if mode == "prior":
        prior = rng.random(case.N).astype(np.float32)
        gain = np.array([0.5, 0.0, -0.25, 2.0, 0.1], dtype=np.float32)
    if mode == "window":
        flt = dict(news_time=rng.integers(0, 1000, case.N).astype(np.int32),
                   time_lo=np.array([0, 100, 200, 0, 500], dtype=np.int32),
                   time_hi=np.array([999, 800, 900, 400, 999], dtype=np.int32))
    _page_equals_exclusion_route(case, 7, 5, excl, flt, prior, gain)


# ------------------------------------------------------------------ 3. the union of the pages == one call
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pages,k", [(4, 16), (8, 8), (64, 1)])
def test_gpu_page_union_is_one_call(gpu_device, pages, k, dtype):
    from news_recommendation_project_v2_amd import ops
    rng, case = _random_case(dtype, gpu_device)
    excl = [rng.integers(0, case.N, n) for n in (0, 3, 40, 1, 5)]
    kw = case.kw(excl)
    one, _ = ops.topk_users(case.users, case.table, case.inv, 64, **kw)
    want = _rows(one.cpu().numpy())
    assert all(len(w) == 64 for w in want)
    got = [set() for _ in range(case.U)]
    for pg in case.walk(k, pages, **kw):
        for u, rows in enumerate(_rows(pg[0])):
            assert len(rows) == k and not (rows & got[u]), "pages overlap"
            got[u] |= rows
    assert got == want


# ------------------------------------------------------------------ 4. across runs and chunks
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_page_boundary_between_chunks(gpu_device, dtype):
    """U = 3 over two chunks: two workgroup runs side by side, merged in stage 2.  The planted
    rows alternate between the first and the last rows of the table, so every page boundary
    falls between rows of different chunks."""
    c = _chunk()
    N = c + 300
    case, where, excl = _planted(24, N, dtype, gpu_device, seed=12, spread=190)
    assert (where[:, 0::2] < c).all() and (where[:, 1::2] >= c).all()
    pages = case.walk(8, 4, **case.kw(excl))
    for p in range(4):
        assert np.array_equal(pages[p][0], where[:, 8 * p:8 * p + 8]), p
    # an odd page size moves the boundary to the other side
    pages = case.walk(5, 6, **case.kw(excl))
    for p in range(6):
        assert np.array_equal(pages[p][0], where[:, 5 * p:5 * p + 5]), p


class _DeviceCase(Case):
    """A case made on the device (no host copy of a large operand)."""

    def __init__(self, users, table, inv, dtype, dev):
        self.users, self.table, self.inv, self.dtype, self.dev = users, table, inv, dtype, dev
        self.U, self.N = users.shape[0], table.shape[0]

    def rows(self, sel):
        return _DeviceCase(self.users[torch.as_tensor(sel, device=self.dev)].contiguous(), self.table, self.inv,
                           self.dtype, self.dev)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_page_many_users_walk_chunks_in_sequence(gpu_device, dtype):
    """With enough user blocks to fill the device a workgroup walks several chunks with one
    running list and one cursor; identity 2 for 64 sampled users, who run alone (chunk by
    chunk in parallel) on the exclusion route."""
    from news_recommendation_project_v2_amd import ops
    c, U = _chunk(), 65536
    N = 2 * c + 77
    gen = torch.Generator(device=gpu_device).manual_seed(9)
    table = torch.randn((N, D), generator=gen, device=gpu_device).to(dtype)
    users = torch.randn((U, D), generator=gen, device=gpu_device)
    case = _DeviceCase(users, table, ops.row_inv_norm(table, 1e-8), dtype, gpu_device)
    rng = np.random.default_rng(10)
    sel = np.unique(np.concatenate([[0, 127, 128, 40000, U - 1], rng.integers(0, U, 80)]))[:64]
    assert len(sel) == 64
    lists = {int(u): np.array([c - 1, c, c + 5, 2 * c, 2 * c + 76, c - 1]) for u in sel[::2]}
    excl = [lists.get(u, ()) for u in range(U)]
    _page_equals_exclusion_route(case, 7, 5, excl, users=sel)


# ------------------------------------------------------------------ 5. ties
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_page_ties_across_pages_and_chunks(gpu_device, dtype):
    c = _chunk()
    N = c + 300
    rng = np.random.default_rng(3)
    table = rng.standard_normal((N, D)).astype(np.float32)
    dup = [5, 300, c - 1, c, c + 200]  # five equal best rows, two of them in the second chunk
    nb = 77                           # the next best, far from both
    table[dup] = table[5]
    table[nb] = 0.6 * table[5] + 0.8 * table[nb]
    users = (table[5] * 0.8 + 0.02 * rng.standard_normal(D)).astype(np.float32)[None, :]
    case = Case(users, table, dtype, gpu_device)
    ref = case.ref[0]
    assert len(set(ref[dup].tolist())) == 1 and ref[dup[0]] > ref[nb] + 0.1
    assert ref[nb] > np.delete(ref, dup + [nb]).max() + 0.1
    pages = case.walk(2, 3)
    assert [pg[0].tolist() for pg in pages] == [[[5, 300]], [[c - 1, c]], [[c + 200, nb]]]
    assert len({int(pg[1][0, 0]) for pg in pages} | {int(pages[0][1][0, 1]), int(pages[1][1][0, 1])}) == 1
    # the cursors inside the tie group: one key, the rows of the pages' last entries
    assert pages[0][3][0][0] == pages[1][3][0][0] and [pg[3][1][0] for pg in pages] == [300, c, nb]
    # a page of one: every tie is settled on the row alone
    assert [pg[0][0, 0] for pg in case.walk(1, 6)] == dup + [nb]


# ------------------------------------------------------------------ 6. zero user and exhaustion
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_page_zero_user_and_exhaustion(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    k = 5
    N = k + 3
    rng = np.random.default_rng(6)
    users = rng.standard_normal((3, D)).astype(np.float32)
    users[1] = 0.0
    case = Case(users, rng.standard_normal((N, D)).astype(np.float32), dtype, gpu_device)
    excl = [[], [0, 3, 3], [7]]
    kw = case.kw(excl)
    p0, p1, p2 = case.walk(k, 3, **kw)
    NINF = _bits(np.array([-np.inf], dtype=np.float32))[0]
    # the zero user walks its eligible rows in row order, score 0
    assert p0[0][1].tolist() == [1, 2, 4, 5, 6] and p1[0][1].tolist() == [7, -1, -1, -1, -1]
    assert not p0[1][1].view(np.float32).any() and p1[1][1, 0].view(np.float32) == 0
    assert p0[3][1][1] == 6 and p0[3][0][1].view(np.float32) == 0
    # every user: a full page, a short one that ends in (-1, -inf) with the end cursor, then pads alone
    left = [N - k, N - 2 - k, N - 1 - k]
    for u in range(3):
        assert (p0[0][u] >= 0).all()
        assert (p1[0][u, :left[u]] >= 0).all() and (p1[0][u, left[u]:] == -1).all()
        assert (p1[1][u, left[u]:] == NINF).all() and (p1[2][u, left[u]:] == NINF).all()
        assert _rows(p0[0])[u] | _rows(p1[0])[u] == set(range(N)) - set(excl[u])
    for pg in (p1, p2):
        assert (pg[3][0] == NINF).all() and (pg[3][1] == I32_MAX).all()
    assert (p2[0] == -1).all() and (p2[1] == NINF).all() and (p2[2] == NINF).all()
    # a start cursor is no cursor, bit for bit
    s0, _ = case.page(k, ops.start_cursor(3, gpu_device), **kw)
    for a, b in zip(p0[:3] + p0[3], s0[:3] + s0[3]):
        assert np.array_equal(a, b)
    # no cursor in, a cursor out: nr_topk_users' lists bit for bit
    base = ops.topk_users(case.users, case.table, case.inv, k, **kw)
    assert np.array_equal(p0[0], base[0].cpu().numpy()) and np.array_equal(p0[1], _bits(base[1]))
    # neither: the same again, and no cursor is returned
    none = ops.topk_users_after(case.users, case.table, case.inv, k, want_next=False, **kw)
    torch.cuda.synchronize()
    assert none[3] is None and np.array_equal(p0[0], none[0].cpu().numpy()) and np.array_equal(p0[1], _bits(none[1]))
    # a NaN key makes nothing eligible
    nan = (torch.full((3,), float("nan"), device=gpu_device), torch.zeros(3, dtype=torch.int32, device=gpu_device))
    pn, _ = case.page(k, nan, **kw)
    assert (pn[0] == -1).all() and (pn[3][1] == I32_MAX).all()


# ------------------------------------------------------------------ 7. a deep list against the ranks
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_prior", [False, True], ids=["plain", "prior"])
def test_gpu_page_deep_list_equals_ranks(gpu_device, with_prior, dtype):
    """Every row is a target of the full-table ranks (csrc/fullrank.hip, which counts on the
    same selection keys): the rows of 150 paged entries are exactly the targets of rank < 150."""
    from news_recommendation_project_v2_amd import ops
    rng, case = _random_case(dtype, gpu_device, U=3, seed=33)
    excl = [rng.integers(0, case.N, n) for n in (0, 4, 40)]
    prior = rng.random(case.N).astype(np.float32) if with_prior else None
    gain = np.array([0.5, -0.25, 1.0], dtype=np.float32) if with_prior else None
    kw = case.kw(excl, None, prior, gain)
    tgt = torch.arange(case.N, dtype=torch.int32, device=gpu_device).repeat(case.U)
    off = torch.arange(case.U + 1, dtype=torch.int64, device=gpu_device) * case.N
    rank = (ops.rank_targets_prior if with_prior else ops.rank_targets)(case.users, case.table, case.inv, tgt, off, **kw)
    rank = rank.cpu().numpy().reshape(case.U, case.N)
    want = [set(np.nonzero((r >= 0) & (r < 150))[0].tolist()) for r in rank]
    assert all(len(w) == 150 for w in want)
    for k, n_pages in ((50, 3), (64, 3)):
        got = [set() for _ in range(case.U)]
        for p, pg in enumerate(case.walk(k, n_pages, **kw)):
            take = min(k, 150 - p * k)  # the last page of 64 is cut in SELECTION order: by rank
            for u in range(case.U):
                rows = pg[0][u]
                assert sorted(rank[u, rows].tolist()) == list(range(p * k, p * k + k)), "a page is a slice of the ranks"
                got[u] |= set(rows[rank[u, rows] < p * k + take].tolist())
        assert got == want


# ------------------------------------------------------------------ 8. engine and helper
def _engine(pooler, dtype, dev, n_news=300, n_imp=40, seed=8):
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    rng = np.random.default_rng(seed)
    distinct = [rng.integers(0, n_news, n).astype(np.int32) for n in rng.integers(1, 12, 12)]
    if pooler == "final":  # an empty history (a zero user) among them; the latent pooler's 0 / 0 is not finite
        distinct[3] = np.zeros(0, np.int32)
    pick = rng.integers(0, 12, n_imp)  # repeated histories: the deduplicated path
    pick[:2] = 5
    hl = np.array([len(distinct[p]) for p in pick], dtype=np.int32)
    hi = np.concatenate([distinct[p] for p in pick]).astype(np.int32)
    eng = PoolScoreEngine(_model(pooler, dev), dtype=dtype, device=dev)
    eng.load_news(W.news_table(5, n_news, 1024, name="page"))
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(n_imp, np.int32))
    return eng, hi, hl


@pytest.mark.gpu
@pytest.mark.parametrize("pooler,dtype", [("latent", torch.float32), ("final", torch.bfloat16)])
def test_gpu_engine_pages_and_deep_lists(gpu_device, pooler, dtype):
    eng, hi, hl = _engine(pooler, dtype, gpu_device)
    k, n_imp = 9, len(hl)
    # three chained pages == recommend_deep(3 k, page = k) as sets; its order is (score desc, row asc)
    chain, cur = [], None
    for _ in range(3):
        idx, sc, cur = eng.recommend(k, after=cur, want_cursor=True)
        assert idx.shape == sc.shape == (n_imp, k) and cur[0].shape == cur[1].shape == (n_imp,)
        chain.append(idx.cpu().numpy())
    deep_i, deep_s = eng.recommend_deep(3 * k, page=k)
    torch.cuda.synchronize()
    di, ds = deep_i.cpu().numpy(), deep_s.cpu().numpy()
    assert di.shape == ds.shape == (n_imp, 3 * k) and (di >= 0).all()
    for i in range(n_imp):
        rows = [set(c[i].tolist()) for c in chain]
        assert not (rows[0] & rows[1]) and not (rows[0] & rows[2]) and not (rows[1] & rows[2])
        assert rows[0] | rows[1] | rows[2] == set(di[i].tolist()) and len(set(di[i].tolist())) == 3 * k
    assert (ds[:, 1:] <= ds[:, :-1]).all()
    tie = ds[:, 1:] == ds[:, :-1]
    assert (di[:, 1:][tie] > di[:, :-1][tie]).all()
    # the first page is recommend itself; recommend_deep(k <= 64, page = k) is recommend bit for bit
    r_i, r_s = eng.recommend(k)
    assert np.array_equal(chain[0], r_i.cpu().numpy())
    for kk in (k, 64):
        a, b = eng.recommend_deep(kk, page=kk, want_keys=True), eng.recommend(kk, want_keys=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3
    off = np.concatenate([[0], np.cumsum(hl)])
    for i in range(n_imp):
        assert not np.isin(di[i], hi[off[i]:off[i + 1]]).any(), "an impression's own history in its list"
    # impressions 0 and 1 share a history; with different cursors they get different pages
    _, _, c1 = eng.recommend(k, want_cursor=True)
    start = (torch.full((n_imp,), float("inf"), device=gpu_device),
             torch.full((n_imp,), -1, dtype=torch.int32, device=gpu_device))
    mixed = (torch.where(torch.arange(n_imp, device=gpu_device) == 1, c1[0], start[0]),
             torch.where(torch.arange(n_imp, device=gpu_device) == 1, c1[1], start[1]))
    m_i, _ = eng.recommend(k, after=mixed)
    m_i = m_i.cpu().numpy()
    assert np.array_equal(m_i[0], chain[0][0]) and np.array_equal(m_i[1], chain[1][1])
    assert np.array_equal(chain[0][0], chain[0][1]) and not np.array_equal(m_i[0], m_i[1])
    assert np.array_equal(np.delete(m_i, 1, axis=0), np.delete(chain[0], 1, axis=0))
    # user_block does not change a deep list
    b_i, b_s = eng.recommend_deep(3 * k, page=k, user_block=5)
    assert torch.equal(b_i, deep_i) and torch.equal(b_s, deep_s)


@pytest.mark.gpu
@pytest.mark.parametrize("pooler", ["final", "latent"])
def test_gpu_get_top_k_recommendations_paged(gpu_device, pooler):
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    rng = np.random.default_rng(8)
    n_news, n_imp = 96, 12
    hl = rng.integers(1, 9, n_imp).astype(np.int32)
    hi = rng.integers(0, n_news, int(hl.sum())).astype(np.int32)
    table = W.news_table(5, n_news, 1024, name="page-api")
    m = _model(pooler, gpu_device)
    got = dmh.get_top_k_recommendations(hi, hl, table, m, 100, page=32)
    gi, gs = got["news_index"], got["scores"]
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gi.shape == gs.shape == (n_imp, 100)
    assert set(got) == {"news_index", "scores"}
    off = np.concatenate([[0], np.cumsum(hl)])
    for i in range(n_imp):
        own = set(hi[off[i]:off[i + 1]].tolist())
        n = n_news - len(own)
        assert set(gi[i, :n].tolist()) == set(range(n_news)) - own
        assert (gi[i, n:] == -1).all() and np.isneginf(gs[i, n:]).all() and np.isfinite(gs[i, :n]).all()
    assert (gs[:, 1:] <= gs[:, :-1]).all()
    # the first 64 in one call: the same rows (pages are slices of one ordering)
    one = dmh.get_top_k_recommendations(hi, hl, table, m, 64)
    paged = dmh.get_top_k_recommendations(hi, hl, table, m, 64, page=16)
    assert [set(r) for r in one["news_index"].tolist()] == [set(r) for r in paged["news_index"].tolist()]
    # under a prior the result has keys, ordered
    pri = rng.random(n_news).astype(np.float32)
    got = dmh.get_top_k_recommendations(hi, hl, table, m, 70, page=64, prior=pri, prior_gain=0.5)
    ky = got["keys"]
    assert ky.shape == (n_imp, 70) and (ky[:, 1:] <= ky[:, :-1]).all()
    have = got["news_index"] >= 0
    want = (got["scores"] + np.float32(0.5) * pri[np.maximum(got["news_index"], 0)]).astype(np.float32)
    assert np.array_equal(ky[have], want[have])


# ------------------------------------------------------------------ 9. determinism
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_page_deterministic(gpu_device, dtype):
    rng = np.random.default_rng(5)
    case = Case(rng.standard_normal((257, D)), rng.standard_normal((1000, D)), dtype, gpu_device, want_ref=False)
    excl = [rng.integers(0, 1000, rng.integers(0, 40)) for _ in range(257)]
    kw = case.kw(excl)
    a, b = case.walk(64, 3, **kw), case.walk(64, 3, **kw)
    for pa, pb in zip(a, b):
        for x, y in zip(pa[:3] + pa[3], pb[:3] + pb[3]):
            assert np.array_equal(x, y)
