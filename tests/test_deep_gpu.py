"""Deep retrieval (include/newsrec_deep.h; csrc/deep.hip) on the GPU: up to 256 rows per user
from one walk over the table.

No test here uses a tolerance.  Each is an exact identity between two GPU paths -- a deep call
against the ceil(K / 64) cursor pages of nr_topk_users_after from the same cursor, ordered as
one list; a deep list against the full-table ranks of an independent kernel -- or a planted case.

Shapes, the smallest at which the kernels can go wrong: N = 700 (five full tiles and a partial
one: a log of 512 pairs fills, and is compacted, after the fourth), N = one chunk + 300 (two
runs side by side: the deep merge), rows in ascending score order (every row passes the
threshold: the most appends and compactions a walk can see), U = 131 (a user block of three
users: dead users' threads take the compaction barriers), U = 65536 x N = two chunks + 77 (one
workgroup walks several chunks), N = K + 3 (short lists), both dtypes.
"""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from retrieval_cases import _chunk, _random_users_table
from test_page_gpu import DTYPES, I32_MAX, IDS, Case, _bits, _DeviceCase, _engine, _random_case, _rows

D = 1024
NINF_BITS = int(np.array([-np.inf], dtype=np.float32).view(np.int32)[0])


def _deep(case, k, after=None, **kw):
    """One deep call, on the device: (idx, scores, keys, (next key, next row))."""
    from news_recommendation_project_v2_amd import ops
    return ops.topk_users_deep(case.users, case.table, case.inv, k, after=after, **kw)


def _paged(case, k, after=None, **kw):
    """The same list by the paged route: ceil(k / 64) cursor calls from ``after``, the last
    asking for the remainder, concatenated and ordered by (key descending, row ascending); the
    cursor behind the last page."""
    from news_recommendation_project_v2_amd import ops
    sizes = [64] * (k // 64) + ([k % 64] if k % 64 else [])
    pages, cur = [], after
    for p in sizes:
        idx, sc, ky, cur = ops.topk_users_after(case.users, case.table, case.inv, p, after=cur, **kw)
        pages.append((idx, sc, ky))
    idx, sc, ky = (torch.cat([pg[i] for pg in pages], dim=1) for i in range(3))
    if len(sizes) > 1:
        # two stable sorts: rows first, then keys (a pad, row -1 and key -inf, ends up last)
        by_row = torch.sort(idx, dim=1, stable=True).indices
        by_key = torch.sort(ky.gather(1, by_row), dim=1, descending=True, stable=True).indices
        order = by_row.gather(1, by_key)
        idx, sc, ky = (t.gather(1, order) for t in (idx, sc, ky))
    return idx, sc, ky, cur


def _same(got, want, what=""):
    """idx, score bits, key bits and the next cursor's bits."""
    for name, a, b in zip(("idx", "scores", "keys", "next_key", "next_row"), (*got[:3], *got[3]), (*want[:3], *want[3])):
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(a, b), (what, name, int((a != b).sum()))


def _excl(rng, case, sizes):
    """Exclusion lists of the given lengths, a duplicate in each that has room for one."""
    lists = [rng.integers(0, case.N, n) for n in sizes]
    for l in lists:
        if len(l) > 1:
            l[-1] = l[0]
    return lists


def _filter(rng, case, kind):
    """The scan's other axes for a case of 5 users.  Wide windows and masks: most users keep more
    than 384 of 700 rows, so their logs still fill and are compacted."""
    flt = prior = gain = None
    if kind in ("filter", "both"):
        flt = dict(news_time=rng.integers(0, 1000, case.N).astype(np.int32),
                   time_lo=np.array([0, 100, 0, 0, 500], dtype=np.int32),
                   time_hi=np.array([999, 999, 900, 999, 999], dtype=np.int32),
                   news_cat=rng.integers(0, 20, case.N).astype(np.uint8),
                   cat_mask=np.array([-1, -1, -1 ^ 0b11, 0xFFFFF ^ 0b100, -1], dtype=np.int64))
    if kind in ("prior", "both"):
        prior = rng.random(case.N).astype(np.float32)
        gain = np.array([0.5, 0.0, -0.25, 2.0, 0.1], dtype=np.float32)
    return flt, prior, gain


# ------------------------------------------------------------------ 1. a deep call == the sorted pages
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_deep_equals_sorted_pages(gpu_device, dtype):
    from news_recommendation_project_v2_amd import ops
    rng, case = _random_case(dtype, gpu_device, zero_user=3)
    kw = case.kw(_excl(rng, case, (0, 4, 40, 4, 0)))
    for k in (1, 64, 65, 100, 192, 256):
        got = _deep(case, k, **kw)
        _same(got, _paged(case, k, **kw), k)
        assert (got[0] >= 0).all()
        if k <= 64:
            _same(got, ops.topk_users_after(case.users, case.table, case.inv, k, **kw), k)
    # the zero user walks its eligible rows in row order
    zero = got[0][3].cpu().numpy()
    assert (np.diff(zero) > 0).all() and not got[1][3].any()
    # no cursor wanted: none returned, the same lists
    none = _deep(case, 256, want_next=False, **kw)
    assert none[3] is None and all(torch.equal(a, b) for a, b in zip(none[:3], got[:3]))


# ------------------------------------------------------------------ 2. every axis of the scan, K = 256
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["filter", "prior", "both"])
def test_gpu_deep_scan_axes(gpu_device, kind, dtype):
    from news_recommendation_project_v2_amd import ops
    rng, case = _random_case(dtype, gpu_device, seed=22)
    flt, prior, gain = _filter(rng, case, kind)
    kw = case.kw(_excl(rng, case, (0, 4, 40, 1, 5)), flt, prior, gain)
    got = _deep(case, 256, **kw)
    _same(got, _paged(case, 256, **kw), "from the start")
    n = (got[0] >= 0).sum(1).cpu().numpy()
    assert n.max() == 256 and (n > 100).all(), n
    # from a cursor in the middle of the list: behind row 37 of a previous call
    mid = ops.topk_users_after(case.users, case.table, case.inv, 37, **kw)[3]
    got = _deep(case, 256, after=mid, **kw)
    _same(got, _paged(case, 256, after=mid, **kw), "from a cursor")
    # a start cursor is no cursor
    _same(_deep(case, 256, after=ops.start_cursor(case.U, gpu_device), **kw), _deep(case, 256, **kw), "start cursor")
    # a NaN cursor and the end cursor: nothing is eligible
    nan = (torch.full((case.U,), float("nan"), device=gpu_device),
           torch.zeros(case.U, dtype=torch.int32, device=gpu_device))
    end = (torch.full((case.U,), float("-inf"), device=gpu_device),
           torch.full((case.U,), I32_MAX, dtype=torch.int32, device=gpu_device))
    for cur in (nan, end):
        idx, sc, ky, nxt = _deep(case, 256, after=cur, **kw)
        assert (idx == -1).all() and (_bits(sc) == NINF_BITS).all() and (_bits(ky) == NINF_BITS).all()
        assert (_bits(nxt[0]) == NINF_BITS).all() and (nxt[1] == I32_MAX).all()


# ------------------------------------------------------------------ 3. compaction under pressure
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("U", [5, 131])
def test_gpu_deep_compaction_under_pressure(gpu_device, U, dtype):
    """The table's rows in ascending order of user 0's score: every row of a run beats user 0's
    threshold (a full log at every fourth tile, the most compactions a walk can see); user 1 =
    -user 0 sees them descending (nothing passes once the log was cut).  Two runs: the deep
    merge.  U = 131: a second user block of three users."""
    c = _chunk()
    N = c + 300
    rng = np.random.default_rng(31)
    table = rng.standard_normal((N, D)).astype(np.float32) * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    users = (rng.standard_normal((U, D)) * 0.7).astype(np.float32)
    s0 = (table.astype(np.float64) @ users[0].astype(np.float64)) / np.linalg.norm(table.astype(np.float64), axis=1)
    table = np.ascontiguousarray(table[np.argsort(s0, kind="stable")])
    users[1] = -users[0]
    case = Case(users, table, dtype, gpu_device, want_ref=False)
    excl = [rng.integers(0, N, n) for n in rng.integers(0, 6, U)]
    excl[0] = np.array([N - 1, N - 2, c - 1, c, 5])  # user 0's very best rows, and a chunk boundary
    kw = case.kw(excl)
    got = _deep(case, 256, **kw)
    _same(got, _paged(case, 256, **kw), U)
    idx = got[0].cpu().numpy()
    assert (idx >= 0).all()
    # user 0's list is the top of the table minus its exclusions, user 1's the bottom (ranks may
    # differ from the float64 order by a selection error: the rows lie well inside)
    assert idx[0].min() > N - 400 and idx[1].max() < 400 and not np.isin(idx[0], excl[0]).any()


# ------------------------------------------------------------------ 4. ties across the K-th boundary
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_deep_ties_across_the_boundary(gpu_device, dtype):
    """Rows 300 .. 339 are copies of the row at reference rank 240 of user 0: the tie group
    covers ranks 240 .. 280, so lists of 250 and 256 rows end inside it."""
    rng, users, table = _random_users_table(3, 700, 41)
    t64 = table.astype(np.float64)
    src = int(np.argsort(-(t64 @ users[0].astype(np.float64)) / np.linalg.norm(t64, axis=1), kind="stable")[240])
    table[300:340] = table[src]
    tied = Case(users, table, dtype, gpu_device, want_ref=False)
    copies = np.array(sorted(set(range(300, 340)) | {src}))
    for k in (250, 256):
        got = _deep(tied, k)
        _same(got, _paged(tied, k), k)
        rows = got[0][0].cpu().numpy()
        inside = np.sort(rows[np.isin(rows, copies)])
        assert 0 < len(inside) < len(copies), "the list must end inside the tie group"
        assert np.array_equal(inside, copies[:len(inside)]), "ties go by ascending row"
        # one score for the copies, and the cursor on the last copy taken
        sc = _bits(got[1])[0][np.isin(rows, copies)]
        assert len(set(sc.tolist())) == 1
        assert int(got[3][1][0]) == inside[-1]
        # the next call starts at the next copy
        more = _deep(tied, 65, after=got[3])[0][0].cpu().numpy()
        rest = copies[len(inside):]
        assert np.array_equal(np.sort(more[np.isin(more, copies)]), rest)


# ------------------------------------------------------------------ 5. short lists
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_deep_short_lists(gpu_device, dtype):
    k = 256
    N = k + 3
    rng, case = _random_case(dtype, gpu_device, U=3, N=N, seed=51)
    excl = [np.array([0, 7, 7, 100, N - 1, 200]), np.array([], dtype=np.int64), np.array([1, 2, 3, 4, 5])]
    kw = case.kw(excl)
    got = _deep(case, k, **kw)
    _same(got, _paged(case, k, **kw))
    idx, sc, ky = got[0].cpu().numpy(), _bits(got[1]), _bits(got[2])
    left = [N - 5, k, N - 5]
    for u in range(3):
        assert (idx[u, :left[u]] >= 0).all() and (idx[u, left[u]:] == -1).all()
        assert (sc[u, left[u]:] == NINF_BITS).all() and (ky[u, left[u]:] == NINF_BITS).all()
        assert _rows(idx)[u] <= set(range(N)) - set(excl[u].tolist())
        short = left[u] < k
        assert (int(got[3][1][u]) == I32_MAX) == short and (_bits(got[3][0])[u] == NINF_BITS) == short
    # from those cursors: nothing for the exhausted users, the last three rows for the other
    idx2, sc2, ky2, nxt2 = _deep(case, k, after=got[3], **kw)
    idx2 = idx2.cpu().numpy()
    assert (idx2[[0, 2]] == -1).all() and (idx2[1, :3] >= 0).all() and (idx2[1, 3:] == -1).all()
    assert _rows(idx)[1] | _rows(idx2)[1] == set(range(N))
    assert (_bits(sc2)[[0, 2]] == NINF_BITS).all() and (nxt2[1] == I32_MAX).all()


# ------------------------------------------------------------------ 6. a deep list against the ranks
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_prior", [False, True], ids=["plain", "prior"])
def test_gpu_deep_list_equals_ranks(gpu_device, with_prior, dtype):
    """Every row is a target of the full-table ranks (csrc/fullrank.hip, which counts on the
    same selection keys): the rows of a deep call of 150 are exactly the targets of rank < 150."""
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
    got = _deep(case, 150, **kw)
    assert _rows(got[0].cpu().numpy()) == want
    # and the cursor is the target of rank 149
    assert [int(rank[u, int(r)]) for u, r in enumerate(got[3][1].cpu().numpy())] == [149] * 3


# ------------------------------------------------------------------ 7. one workgroup over several chunks
@pytest.mark.gpu
def test_gpu_deep_many_users_walk_chunks_in_sequence(gpu_device):
    """bf16, U = 65536: enough user blocks to fill the device, so a workgroup walks two chunks
    with one log per user; the same users in a call of 128 run chunk by chunk side by side."""
    from news_recommendation_project_v2_amd import ops
    c, U, dtype = _chunk(), 65536, torch.bfloat16
    N = 2 * c + 77
    gen = torch.Generator(device=gpu_device).manual_seed(9)
    table = torch.randn((N, D), generator=gen, device=gpu_device).to(dtype)
    users = torch.randn((U, D), generator=gen, device=gpu_device)
    case = _DeviceCase(users, table, ops.row_inv_norm(table, 1e-8), dtype, gpu_device)
    got = _deep(case, 256)
    _same(got, _paged(case, 256), "all users")
    assert (got[0] >= 0).all()
    small = _deep(case.rows(np.arange(128)), 256)
    _same(tuple(t[:128] for t in got[:3]) + ((got[3][0][:128], got[3][1][:128]),), small, "position independence")


# ------------------------------------------------------------------ 8. chained deep calls
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_deep_calls_chain(gpu_device, dtype):
    rng, case = _random_case(dtype, gpu_device, seed=81)
    kw = case.kw(_excl(rng, case, (0, 4, 40, 1, 5)))
    a = _deep(case, 200, **kw)
    b = _deep(case, 200, after=a[3], **kw)
    want = _paged(case, 400, **kw)
    ra, rb, rw = (_rows(t[0].cpu().numpy()) for t in (a, b, want))
    for u in range(case.U):
        assert len(ra[u]) == len(rb[u]) == 200 and not (ra[u] & rb[u])
        assert ra[u] | rb[u] == rw[u]
    assert torch.equal(b[3][1], want[3][1]) and torch.equal(b[3][0].view(torch.int32), want[3][0].view(torch.int32))


# ------------------------------------------------------------------ 9. engine, helper, script
@pytest.mark.gpu
@pytest.mark.parametrize("pooler,dtype", [("latent", torch.float32), ("final", torch.bfloat16)])
def test_gpu_engine_walks_equal_pages(gpu_device, pooler, dtype):
    eng, hi, hl = _engine(pooler, dtype, gpu_device, n_news=1200)
    n_news = 1200
    rng = np.random.default_rng(9)
    eng.set_catalogue(news_time=rng.integers(0, 1000, n_news).astype(np.int32),
                      news_prior=rng.random(n_news).astype(np.float32))
    same = lambda a, b: len(a) == len(b) and all(
        torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                    y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
    for k, w, p in ((300, 256, 64), (300, 100, 50), (1024, 256, 64), (40, 40, 40)):
        a, b = eng.recommend_deep(k, walk=w, want_keys=True), eng.recommend_deep(k, page=p, want_keys=True)
        assert len(a) == 3 and a[0].shape == (len(hl), k) and same(a, b), (k, w, p)
        assert same(eng.recommend_deep(k, walk=w), b[:2]), (k, w, p)
    base = eng.recommend_deep(300, page=64, want_keys=True)
    assert same(eng.recommend_deep(300, walk=256, want_keys=True, user_block=5), base)
    gains = np.linspace(-0.5, 1.0, len(hl)).astype(np.float32)
    for kw in ({"time_window": (100, 800)}, {"prior_gain": 0.5}, {"prior_gain": gains, "time_window": (0, 900)}):
        a = eng.recommend_deep(300, walk=256, want_keys=True, **kw)
        assert same(a, eng.recommend_deep(300, page=64, want_keys=True, **kw)), kw
        assert not same(a, base), kw
    # impressions 0 and 1 share a history (the deduplicated path): one list for both
    assert torch.equal(base[0][0], base[0][1])
    off = np.concatenate([[0], np.cumsum(hl)])
    got = eng.recommend_deep(300, walk=256)[0].cpu().numpy()
    for i in range(len(hl)):
        assert not np.isin(got[i], hi[off[i]:off[i + 1]]).any(), "an impression's own history in its list"


@pytest.mark.gpu
def test_gpu_get_top_k_recommendations_walk(gpu_device):
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd import weights as W
    from retrieval_cases import _model
    rng = np.random.default_rng(8)
    n_news, n_imp = 500, 12
    hl = rng.integers(1, 9, n_imp).astype(np.int32)
    hi = rng.integers(0, n_news, int(hl.sum())).astype(np.int32)
    table = W.news_table(5, n_news, 1024, name="deep-api")
    m = _model("final", gpu_device)
    got = dmh.get_top_k_recommendations(hi, hl, table, m, 300, walk=256)
    want = dmh.get_top_k_recommendations(hi, hl, table, m, 300, page=64)
    assert set(got) == set(want) == {"news_index", "scores"} and got["news_index"].shape == (n_imp, 300)
    assert np.array_equal(got["news_index"], want["news_index"])
    assert np.array_equal(got["scores"].view(np.int32), want["scores"].view(np.int32))
    pri = rng.random(n_news).astype(np.float32)
    got = dmh.get_top_k_recommendations(hi, hl, table, m, 300, walk=200, prior=pri, prior_gain=0.5)
    want = dmh.get_top_k_recommendations(hi, hl, table, m, 300, page=64, prior=pri, prior_gain=0.5)
    for name in ("news_index", "scores", "keys"):
        assert np.array_equal(got[name].view(np.int32), want[name].view(np.int32)), name


@pytest.mark.gpu
def test_gpu_recommend_script_walk(tmp_path):
    """scripts/recommend.py --synthetic -k 256 --walk 256 writes what --page 64 writes (the
    script has no CPU path)."""
    recs = []
    for name, flag in (("walk", ["--walk", "256"]), ("page", ["--page", "64"])):
        cmd = [sys.executable, str(REPO / "scripts" / "recommend.py"), "--synthetic", "-k", "256", *flag,
               "--num-impressions", "200", "--out-dir", str(tmp_path / name)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line[name] == int(flag[1]) and line["k"] == 256 and ("page" in line) == (name == "page")
        recs.append(np.load(tmp_path / name / "recommendations.npy"))
    assert recs[0].shape == (200, 256) and (recs[0] >= 0).any() and np.array_equal(recs[0], recs[1])
