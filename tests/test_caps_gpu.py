"""Per-group caps of top-K retrieval (include/newsrec_caps.h; csrc/caps.hip) on the GPU.

What is compared with what.  Identities between GPU calls are bit for bit (torch.equal on
every output).  The float64 reference (tests/caps_ref.py: the greedy walk, checked there
against brute force) is compared exactly only on planted inputs, whose reference scores are
asserted >= 1e-2 apart on the CPU before any call (tests/retrieval_cases.py), or >= 1e-3 for
the keys of the composition test, and on duplicated rows, whose scores are equal bit for bit.
On random inputs the list has to be eps-stable: EPS = 1e-4 is tests/test_topk_gpu.py's, the
f32 accumulation bound of a 1024-term dot product on the cosine scale, derived there.

eps-stability under caps.  Every eligible row that was not returned must have a reason: its
group holds ``cap`` returned rows and the row is no more than eps above the worst of them, or
the list is full and the row is no more than eps above the list's worst.  A short list with
an eligible row of a group below its cap left out has neither and fails.  The list is asserted
to be exactly the reference's at every row whose score, in the order of ALL eligible rows, is
more than eps away from both neighbours: the rows ahead of it are then the same set for the
kernel and for the reference, and whether a row is taken, and how many are taken before it,
depends on that set alone (the walk takes sum over groups of min(cap, rows of the group in the
prefix) rows from a prefix, whatever their order).  So such a row is in the returned list if and
only if it is in the reference's.  Its POSITION is asserted in f32 only: lists are finally
ordered by the evaluation path's scores (include/newsrec_topk.h, "Returned scores"), which in
bf16 are taken from the unrounded f32 user row, while the reference scores here are the
selection's, of the user row rounded to bf16 (DESIGN.md section 3.8 has the band between them).

Shapes, as in tests/test_topk_gpu.py, the smallest at which each mechanism exists: 1x1000 and
257x1000 (one chunk; three user blocks, the last partial), 5x(2 chunk + 77) (three chunks side
by side, a partial last tile: per-chunk partials and the capped merge), and 65,536 users for
one running list over several chunks.
"""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import caps_ref
import retrieval_cases
from conftest import REPO
from news_recommendation_project_v2_amd import weights as W
from retrieval_cases import _chunk, _model, _random_users_table

D = 1024
EPS = 1e-4  # tests/test_topk_gpu.py
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
SHAPES = ["1x1000", "257x1000", "5x2c+77"]
NINF = float("-inf")


def _shape(name):
    return {"1x1000": (1, 1000), "257x1000": (257, 1000), "5x2c+77": (5, 2 * _chunk() + 77)}[name]


def _csr(lists):
    return retrieval_cases._csr(lists, "cpu")[:2]


class Case(retrieval_cases.Case):
    """Every call takes host arrays: ``flt`` = dict(news_time, time_lo, time_hi, news_cat, cat_mask)
    with None for a pair that is left out, ``excl`` = (idx, off), ``prior`` / ``gain`` f32 or None,
    ``groups`` any integers in [0, 1024)."""

    def _up(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _kw(self, flt, excl, prior, gain):
        kw = {k: self._up(v) for k, v in (flt or {}).items()}
        if excl is not None:
            kw.update(excl_idx=self._up(excl[0]), excl_off=self._up(excl[1]))
        kw.update(news_prior=self._up(prior), user_gain=self._up(gain))
        return kw

    def capped(self, k, groups, cap, flt=None, excl=None, prior=None, gain=None, users=None):
        """(idx, scores, keys) of nr_topk_users_capped, device tensors."""
        from news_recommendation_project_v2_amd import ops
        out = ops.topk_users_capped(self.users if users is None else users, self.table, self.inv, k,
                                    self._up(np.asarray(groups).astype(np.int16)), cap,
                                    **self._kw(flt, excl, prior, gain))
        torch.cuda.synchronize()
        return out

    def base(self, k, flt=None, excl=None, prior=None, gain=None):
        """(idx, scores, keys) of nr_topk_users_prior on the same operands."""
        from news_recommendation_project_v2_amd import ops
        out = ops.topk_users_prior(self.users, self.table, self.inv, k, **self._kw(flt, excl, prior, gain))
        torch.cuda.synchronize()
        return out

    def check_scores(self, idx, sc):
        """Returned scores are ops.score_users' bit for bit, (-1, -inf) pads."""
        from news_recommendation_project_v2_amd import ops
        U, k = idx.shape
        want = ops.score_users(self.users, torch.arange(U, dtype=torch.int32, device=self.dev), self.table, self.inv,
                               idx.clamp(min=0).reshape(-1).contiguous(),
                               torch.arange(U + 1, dtype=torch.int64, device=self.dev) * k, U * k).reshape(U, k)
        want = torch.where(idx >= 0, want, torch.full_like(want, NINF))
        torch.cuda.synchronize()
        assert torch.equal(sc, want), "top_scores differ from ops.score_users"


def _same(a, b, what):
    for x, y, name in zip(a, b, ("idx", "scores", "keys")):
        assert torch.equal(x, y), f"{what}: {name} differ"


def _random_filter(rng, U, N):
    """Both pairs, a window and a mask of its own per user; an empty window and an empty mask."""
    news_time = rng.integers(0, 1000, N).astype(np.int32)
    news_cat = rng.integers(0, 70, N).astype(np.uint8)  # some >= 64: eligible for nobody
    lo = rng.integers(0, 300, U).astype(np.int32)
    hi = (lo + rng.integers(400, 700, U)).astype(np.int32)
    mask = rng.integers(1 << 40, 1 << 62, U).astype(np.int64)
    hi[3::40] = lo[3::40] - 1
    mask[4::40] = 0
    return dict(news_time=news_time, time_lo=lo, time_hi=hi, news_cat=news_cat, cat_mask=mask)


def _eligible(flt, U, N):
    t, c = flt["news_time"].astype(np.int64), flt["news_cat"].astype(np.int64)
    ok = (t[None, :] >= flt["time_lo"][:, None]) & (t[None, :] <= flt["time_hi"][:, None])
    m = flt["cat_mask"].view(np.uint64)
    return ok & (c[None, :] < 64) & (((m[:, None] >> np.minimum(c, 63).astype(np.uint64)[None, :]) & np.uint64(1)) == 1)


def _check_caps(idx, groups, cap):
    for u, row in enumerate(idx):
        got = row[row >= 0]
        assert len(set(got.tolist())) == len(got), f"user {u}: a row twice"
        assert (row[len(got):] == -1).all(), f"user {u}: a pad inside the list"
        if len(got):
            assert np.bincount(groups[got]).max() <= cap, f"user {u}: a group above its cap"


def _check_stable(ref, idx, k, groups, cap, elig=None, excl=None, positions=True):
    """The caps, eps-stability and the exact entries (module docstring) of idx [U, k] against the
    float64 scores ref [U, N]; returns (entries asserted exactly, entries)."""
    U, N = ref.shape
    groups = np.asarray(groups, dtype=np.int64)
    _check_caps(idx, groups, cap)
    want, _ = caps_ref.capped_topk(ref, k, groups, cap, elig, None if excl is None else excl[0],
                                   None if excl is None else excl[1])
    n_exact = n_all = 0
    worst = 0.0
    for u in range(U):
        ok = caps_ref._ok_rows(u, N, elig, None if excl is None else excl[0], None if excl is None else excl[1])
        got = idx[u][idx[u] >= 0].astype(np.int64)
        assert ok[got].all(), f"user {u}: an ineligible row was returned"
        held = np.bincount(groups[got], minlength=1024)
        gmin = np.full(1024, np.inf)
        np.minimum.at(gmin, groups[got], ref[u, got])
        rest = np.setdiff1d(np.nonzero(ok)[0], got)
        full = len(got) == k
        lmin = ref[u, got].min() if len(got) else np.inf
        by_group = (held[groups[rest]] == cap) & (ref[u, rest] <= gmin[groups[rest]] + EPS)
        by_list = full & (ref[u, rest] <= lmin + EPS)
        bad = rest[~(by_group | by_list)]
        assert len(bad) == 0, (f"user {u}: eligible row {bad[0]} (group {groups[bad[0]]}, {held[groups[bad[0]]]} held, "
                               f"score {ref[u, bad[0]]:.6f}) left out without a reason; list {'full' if full else 'short'}")
        if len(rest):
            over = np.where(held[groups[rest]] == cap, ref[u, rest] - gmin[groups[rest]], np.inf)
            if full:  # (one reason is enough: the smaller excess counts)
                over = np.minimum(over, ref[u, rest] - lmin)
            worst = max(worst, float(over.max()))
        order = caps_ref.order_of(ref[u], ok)
        srt = ref[u, order]
        gap = np.diff(srt) < -EPS  # order[p] and order[p + 1] more than eps apart
        lone = np.r_[True, gap] & np.r_[gap, True]
        pos = np.empty(N, dtype=np.int64)
        pos[order] = np.arange(len(order))
        for r in got[lone[pos[got]]]:
            assert r in want[u], f"user {u}: row {r} was returned, the reference does not have it"
        for j in range(k):
            r = want[u, j]
            if r < 0:
                continue
            n_all += 1
            if lone[pos[r]]:
                assert r in idx[u], f"user {u}: the reference has row {r} (position {j}), it was not returned"
                if positions:
                    assert idx[u, j] == r, f"user {u}, position {j}: row {idx[u, j]}, the reference has {r}"
                n_exact += 1
    print(f"stability: a row left out lies at most {worst:.3e} above its bound (eps {EPS:.0e}); "
          f"{n_exact} of {n_all} reference entries asserted exactly")
    return n_exact, n_all


# ------------------------------------------------------------------ 1. degenerate identities
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", ["257x1000", "5x2c+77"])
def test_gpu_caps_degenerate_identities(gpu_device, shape, dtype):
    U, N = _shape(shape)
    rng, users, table = _random_users_table(U, N, seed=31)
    case = Case(users, table, dtype, gpu_device, want_ref=False)
    flt = _random_filter(rng, U, N)
    own = _csr([rng.integers(0, N, int(rng.integers(0, 40))).astype(np.int32) for _ in range(U)])
    prior = rng.random(N).astype(np.float32)
    gain = (rng.standard_normal(U) * 0.3).astype(np.float32)
    groups = rng.integers(0, 18, N)
    for f, e, p, g, what in ((None, None, None, None, "plain"), (flt, own, None, None, "filter"),
                             (None, own, prior, gain, "prior"), (flt, own, prior, gain, "filter + prior")):
        for k, c in ((10, 3), (64, 10)):
            base = case.base(k, f, e, p, g)
            # cap >= K is the base entry
            for cap in (k, 64):
                _same(case.capped(k, groups, cap, f, e, p, g), base, f"{what}, K = {k}, cap = {cap} >= K")
            # one group for all rows, cap = c < K: the base entry at K = c, then pads
            gi, gs, gk = case.capped(k, np.full(N, 7), c, f, e, p, g)
            _same((gi[:, :c], gs[:, :c], gk[:, :c]), case.base(c, f, e, p, g), f"{what}, K = {k}: one group, cap = {c}")
            assert (gi[:, c:] == -1).all() and torch.isneginf(gs[:, c:]).all() and torch.isneginf(gk[:, c:]).all()
            # every row its own group, cap = 1: uncapped
            if N <= 1024:
                _same(case.capped(k, np.arange(N), 1, f, e, p, g), base, f"{what}, K = {k}: a group per row, cap = 1")


# ------------------------------------------------------------------ 2. planted, exact
def _planted_groups(where, n_news, rng):
    """Planted ranks 0 .. 5 of user u in group u, every other planted row in a group of its
    own, the background in random groups >= 512."""
    n_users, P = where.shape
    groups = rng.integers(512, 1024, n_news)
    for u in range(n_users):
        groups[where[u, :6]] = u
        groups[where[u, 6:]] = 3 + u * P + np.arange(6, P)
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("n", ["1000", "2c+77"])
def test_gpu_caps_planted_exact(gpu_device, n, k, dtype):
    N = 1000 if n == "1000" else 2 * _chunk() + 77
    case, where, excl = retrieval_cases._planted(Case, k, N, dtype, gpu_device, seed=k + 100,
                                                 spread=None if n == "1000" else 300)
    if n != "1000":  # the capped group straddles the first chunk and the later ones
        c = _chunk()
        assert (where[:, :6] < c).any(axis=1).all() and (where[:, :6] >= c).any(axis=1).all()
    groups = _planted_groups(where, N, np.random.default_rng(k))
    cap = 2
    own = _csr(excl)
    idx, sc, _ = case.capped(k, groups, cap, excl=own)
    case.check_scores(idx, sc)
    want, _ = caps_ref.capped_topk(case.ref, k, groups, cap, None, *own)
    assert np.array_equal(idx.cpu().numpy(), want)
    # what the reference must have done: ranks 2 .. 5 of the capped group are skipped
    keep = [0, 1] + list(range(6, k + 8))
    assert np.array_equal(want, where[:, keep][:, :k])


# ------------------------------------------------------------------ 3. ties
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_caps_ties(gpu_device, dtype):
    c = _chunk()
    N = 2 * c + 77
    rng = np.random.default_rng(3)
    table = rng.standard_normal((N, D)).astype(np.float32)
    dup = [5, c - 1, c, 2 * c + 76]
    table[dup] = table[5]
    users = (table[5] * 0.8 + 0.02 * rng.standard_normal(D)).astype(np.float32)[None, :]
    case = Case(users, table, dtype, gpu_device)
    assert len(set(case.ref[0, dup].tolist())) == 1 and case.ref[0, dup[0]] > np.delete(case.ref[0], dup).max() + 0.5
    other = 1 + np.arange(N) % 900  # everything else: groups 1 .. 900
    # across chunks (the merge): all four in one group, cap = 2 -> the two lowest rows
    groups = other.copy()
    groups[dup] = 0
    idx, sc, _ = case.capped(4, groups, 2)
    case.check_scores(idx, sc)
    idx = idx.cpu().numpy()
    assert idx[0, :2].tolist() == [5, c - 1] and not np.isin([c, 2 * c + 76], idx).any()
    # two of them in another group, cap = 1 -> the lowest row of each; cap = 2 -> all four in row order
    groups[[c, 2 * c + 76]] = 901
    assert case.capped(4, groups, 1)[0].cpu().numpy()[0, :2].tolist() == [5, c]
    i2, s2, _ = case.capped(4, groups, 2)
    assert i2.cpu().numpy().tolist() == [dup] and len(set(s2.cpu().numpy()[0].tolist())) == 1
    # inside one running list (stage 1): a row that ties with its group's worst member arrives
    # later, in the same tile, in the next tile and far behind; it must not displace it
    table = rng.standard_normal((1000, D)).astype(np.float32)
    dup = [5, 6, 130, 700]
    table[dup] = table[5]
    users = (table[5] * 0.8 + 0.02 * rng.standard_normal(D)).astype(np.float32)[None, :]
    case = Case(users, table, dtype, gpu_device)
    assert len(set(case.ref[0, dup].tolist())) == 1 and case.ref[0, dup[0]] > np.delete(case.ref[0], dup).max() + 0.5
    groups = 1 + np.arange(1000) % 900
    groups[dup] = 0
    for cap, first in ((1, [5]), (2, [5, 6]), (3, [5, 6, 130])):
        idx = case.capped(5, groups, cap)[0].cpu().numpy()
        assert idx[0, :cap].tolist() == first and not np.isin(dup[cap:], idx).any(), cap
        want, _ = caps_ref.capped_topk(case.ref, 5, groups, cap)
        assert idx[0, :cap].tolist() == want[0, :cap].tolist()


# ------------------------------------------------------------------ 4. random, banded
@pytest.fixture(scope="module")
def random_cases(gpu_device):
    """The random operands with their float64 scores, per (shape, dtype); never written to."""
    cache = {}

    def get(shape, dtype):
        if (shape, dtype) not in cache:
            U, N = _shape(shape)
            _, users, table = _random_users_table(U, N, seed=U * 7 + 1)
            cache[shape, dtype] = Case(users, table, dtype, gpu_device)
        return cache[shape, dtype]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n_groups", [3, 18, 300])
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_caps_random_banded(gpu_device, random_cases, shape, n_groups, dtype):
    case = random_cases(shape, dtype)
    groups = np.random.default_rng(n_groups).integers(0, n_groups, case.N)
    exact = total = 0
    for k in (10, 64):
        for cap in (1, 3):
            idx, sc, ky = case.capped(k, groups, cap)
            case.check_scores(idx, sc)
            assert torch.equal(ky, sc), "without a prior the keys are the scores"
            idx = idx.cpu().numpy()
            fill = min(k, n_groups * cap)
            assert ((idx >= 0).sum(1) == fill).all(), f"K = {k}, cap = {cap}: {fill} rows can be taken"
            a, b = _check_stable(case.ref, idx, k, groups, cap, positions=dtype == torch.float32)
            exact, total = exact + a, total + b
    # (around rank 64 of these scores a neighbour is closer than eps for roughly every third row)
    assert 4 * exact > total, "the exact comparison must cover a good share of the entries"


# ------------------------------------------------------------------ 5. one running list against partials
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_caps_many_users_walk_chunks_in_sequence(gpu_device, dtype):
    """With enough user blocks to fill the device a workgroup walks several chunks with ONE
    running capped list; the same users alone run chunk by chunk in parallel, with per-chunk
    partials and the capped merge.  The two must agree bit for bit."""
    from news_recommendation_project_v2_amd import ops
    c, k, cap, U = _chunk(), 10, 2, 65536
    N = 2 * c + 77
    gen = torch.Generator(device=gpu_device).manual_seed(9)
    table = torch.randn((N, D), generator=gen, device=gpu_device).to(dtype)
    users = torch.randn((U, D), generator=gen, device=gpu_device)
    inv = ops.row_inv_norm(table, 1e-8)
    groups_h = np.random.default_rng(18).integers(0, 18, N)
    groups = torch.from_numpy(groups_h.astype(np.int16)).to(gpu_device)
    sel = [0, 127, 128, 40000, U - 1]
    small = users[sel].contiguous()
    top, _, _ = ops.topk_users_capped(small, table, inv, 3, groups, 1)
    lists = {u: np.concatenate([top[i].cpu().numpy(), [c - 1, c, c + 5, 2 * c, 2 * c + 76, c - 1]])
             for i, u in enumerate(sel)}
    _, _, ei_s, eo_s = retrieval_cases._csr([lists[u] for u in sel], gpu_device)
    _, _, ei_b, eo_b = retrieval_cases._csr([lists.get(u, ()) for u in range(U)], gpu_device)
    small_out = ops.topk_users_capped(small, table, inv, k, groups, cap, excl_idx=ei_s, excl_off=eo_s)
    big_out = ops.topk_users_capped(users, table, inv, k, groups, cap, excl_idx=ei_b, excl_off=eo_b)
    torch.cuda.synchronize()
    _same(tuple(t[sel] for t in big_out), small_out, "one running list against the capped merge")
    i_s = small_out[0].cpu().numpy()
    _check_caps(i_s, groups_h, cap)
    assert (i_s >= 0).all()
    for i, u in enumerate(sel):
        assert not np.isin(i_s[i], lists[u]).any()
    # the caps bite here: the uncapped lists differ
    plain, _ = ops.topk_users(small, table, inv, k, excl_idx=ei_s, excl_off=eo_s)
    assert not torch.equal(plain, small_out[0])


# ------------------------------------------------------------------ 6. composition
def _host_keys(idx, sc, gain, prior):
    """fl32(score + fl32(gain * prior)) in float32 numpy: two separately rounded operations; -inf pads."""
    prod = np.asarray(gain, dtype=np.float32)[:, None] * np.asarray(prior, dtype=np.float32)[np.maximum(idx, 0)]
    assert prod.dtype == np.float32 and sc.dtype == np.float32
    return np.where(idx >= 0, sc + prod, np.float32(-np.inf)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [10, 64])
def test_gpu_caps_compose_with_filter_exclusions_and_prior(gpu_device, k, dtype):
    c = _chunk()
    N, U, cap = 2 * c + 77, 3, 2
    case, where, excl = retrieval_cases._planted(Case, k, N, dtype, gpu_device, seed=k + 200, spread=300)
    rng = np.random.default_rng(k)
    groups = _planted_groups(where, N, rng)
    planted = np.zeros(N, dtype=bool)
    planted[where.reshape(-1)] = True
    # the window leaves out planted rank 2, the mask planted rank 3, the exclusion list rank 7
    news_time = rng.integers(0, 1000, N).astype(np.int32)
    news_cat = rng.integers(0, 64, N).astype(np.uint8)
    news_time[where[:, 2]] = 5000
    news_cat[where[:, 3]] = 70
    flt = dict(news_time=news_time, time_lo=np.zeros(U, np.int32), time_hi=np.full(U, 1000, np.int32),
               news_cat=news_cat, cat_mask=np.full(U, -1, np.int64))
    lists = [np.concatenate([excl[u], where[u, 7:8]]) for u in range(U)]
    # user 1: well over 32 excluded rows inside the first chunk (the overflow path)
    lists[1] = np.concatenate([lists[1], np.nonzero(~planted[:c])[0][:60]])
    assert ((lists[1] >= 0) & (lists[1] < c)).sum() > 32
    own = _csr(lists)
    # priors that are multiples of 1/64 up to 4/64 and gains that are powers of two: every
    # product is exact, and no key moves by more than 0.0079 < the planted 1e-2
    prior = (rng.integers(0, 5, N) / 64.0).astype(np.float32)
    gain = np.array([0.125, 0.0625, 0.0], dtype=np.float32)
    keys = case.ref + gain.astype(np.float64)[:, None] * prior.astype(np.float64)[None, :]
    elig = _eligible(flt, U, N)
    want, want_k = caps_ref.capped_topk(keys, k, groups, cap, elig, *own)
    for u in range(U):  # before any call: the reference list's keys are >= 1e-3 apart and above the rest
        ok = caps_ref._ok_rows(u, N, elig, *own)
        srt = keys[u, caps_ref.order_of(keys[u], ok)]
        last = int(np.nonzero(srt >= want_k[u, k - 1])[0].max())
        assert (srt[:last + 1] - srt[1:last + 2] >= 1e-3).all(), "reference keys closer than 1e-3"
    assert (want >= 0).all()
    idx, sc, ky = case.capped(k, groups, cap, flt, own, prior, gain)
    case.check_scores(idx, sc)
    idx, sc, ky = idx.cpu().numpy(), sc.cpu().numpy(), ky.cpu().numpy()
    assert np.array_equal(idx, want)
    assert np.array_equal(ky.view(np.int32), _host_keys(idx, sc, gain, prior).view(np.int32)), "top_keys"
    assert (ky[:, 1:] <= ky[:, :-1]).all()
    # ranks 2, 3 (ineligible) leave group u with ranks 0, 1, 4, 5: two taken, two skipped; rank 7 excluded
    keep = [0, 1] + [j for j in range(6, k + 8) if j != 7]
    assert np.array_equal(np.sort(idx, axis=1), np.sort(where[:, keep][:, :k], axis=1))


# ------------------------------------------------------------------ 7. lists that cannot fill
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_caps_cannot_fill_and_zero_user(gpu_device, dtype):
    U, N, k, cap = 5, 1000, 10, 2
    rng, users, table = _random_users_table(U, N, seed=12, zero_user=3)
    case = Case(users, table, dtype, gpu_device)
    groups = rng.integers(0, 2, N)
    idx, sc, ky = case.capped(k, groups, cap)
    case.check_scores(idx, sc)
    i = idx.cpu().numpy()
    assert ((i[:, :4] >= 0).all() and (i[:, 4:] == -1).all() and torch.isneginf(sc[:, 4:]).all()
            and torch.isneginf(ky[:, 4:]).all()), "2 groups x cap 2: four rows, six pads"
    live = [u for u in range(U) if u != 3]
    _check_stable(case.ref[live], i[live], k, groups, cap, positions=dtype == torch.float32)
    # the zero user: row order under the caps, score 0 (rows 0, 1 of group 0, then 4, 5, ...)
    by4 = np.arange(N) // 4
    idx, sc, _ = case.capped(k, by4, cap)
    assert idx[3].tolist() == [0, 1, 4, 5, 8, 9, 12, 13, 16, 17] and not sc[3].any()
    excl = _csr([[], [], [], [0, 5, 5, 999], []])
    idx, sc, _ = case.capped(k, by4, cap, excl=excl)
    assert idx[3].tolist() == [1, 2, 4, 6, 8, 9, 12, 13, 16, 17] and not sc[3].any()


# ------------------------------------------------------------------ 8. determinism
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_caps_deterministic(gpu_device, dtype):
    rng = np.random.default_rng(5)
    case = Case(rng.standard_normal((257, D)), rng.standard_normal((1000, D)), dtype, gpu_device, want_ref=False)
    excl = _csr([rng.integers(0, 1000, rng.integers(0, 40)).astype(np.int32) for _ in range(257)])
    groups = rng.integers(0, 18, 1000)
    a, b = case.capped(64, groups, 3, excl=excl), case.capped(64, groups, 3, excl=excl)
    _same(a, b, "two runs")


# ------------------------------------------------------------------ 9. engine, helper, script
def _impressions(rng, pooler, n_news, n_imp):
    distinct = [rng.integers(0, n_news, n).astype(np.int32) for n in rng.integers(1, 12, 40)]
    if pooler == "final":  # an empty history (a zero user); the latent pooler's 0 / 0 is not finite
        distinct[3] = np.zeros(0, np.int32)
    pick = rng.integers(0, 40, n_imp)  # repeated histories: the deduplicated path
    hl = np.array([len(distinct[p]) for p in pick], dtype=np.int32)
    return np.concatenate([distinct[p] for p in pick]).astype(np.int32), hl


@pytest.mark.gpu
@pytest.mark.parametrize("pooler,dtype", [("final", torch.float32), ("latent", torch.bfloat16)])
def test_gpu_engine_recommend_group_cap(gpu_device, pooler, dtype):
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd import ops
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    rng = np.random.default_rng(6)
    n_news, n_imp, k, cap = 300, 257, 10, 2
    hi, hl = _impressions(rng, pooler, n_news, n_imp)
    groups = rng.integers(0, 18, n_news)
    table = W.news_table(5, n_news, 1024, name="caps")
    model = _model(pooler, gpu_device)
    eng = PoolScoreEngine(model, dtype=dtype, device=gpu_device)
    eng.load_news(table)
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(n_imp, np.int32))
    eng.set_catalogue(news_group=groups)
    i0, s0 = eng.recommend(k, group_cap=cap)
    i1, s1, k1 = eng.recommend(k, group_cap=cap, user_block=64, want_keys=True)
    assert i0.shape == (n_imp, k) and torch.equal(i0, i1) and torch.equal(s0, s1) and torch.equal(k1, s1)
    # ops.topk_users_capped on the engine's pooled users, expanded to the impressions
    hidx, hoff = eng._distinct_hist()
    users = eng._pooled_users(hidx, hoff)
    di, ds, _ = ops.topk_users_capped(users, eng.cand_table, eng.cand_inv, k, eng.news_group, cap, excl_idx=hidx,
                                      excl_off=hoff)
    sel = eng.user_idx.long() if eng.user_idx is not None else slice(None)
    torch.cuda.synchronize()
    assert torch.equal(i0, di[sel]) and torch.equal(s0, ds[sel])
    i0h = i0.cpu().numpy()
    _check_caps(i0h, groups, cap)
    off = np.concatenate([[0], np.cumsum(hl)])
    for i in range(n_imp):
        assert not np.isin(i0h[i], hi[off[i]:off[i + 1]]).any(), "an impression's own history in its list"
    plain, _ = eng.recommend(k)
    assert not torch.equal(plain, i0), "the caps must bite in this case"
    # cap >= k is recommend itself
    same_i, same_s = eng.recommend(k, group_cap=k)
    assert torch.equal(same_i, plain)
    # with a mask and a prior: the caps, the mask and the order by key hold together
    cats = rng.integers(0, 8, n_news).astype(np.uint8)
    eng.set_catalogue(news_cat=cats, news_prior=rng.random(n_news).astype(np.float32), news_group=groups)
    ci, cs, ck = eng.recommend(k, group_cap=cap, categories=0b00111111, prior_gain=0.25, want_keys=True)
    ui, us, uk = eng.recommend(k, categories=0b00111111, prior_gain=0.25, want_keys=True)
    cih = ci.cpu().numpy()
    _check_caps(cih, groups, cap)
    assert (cats[cih[cih >= 0]] < 6).all() and (ck[:, 1:] <= ck[:, :-1]).all() and not torch.equal(ci, ui)
    # the helper agrees with the engine
    got = dmh.get_top_k_recommendations(hi, hl, table, model, k, dtype=dtype, groups=groups, group_cap=cap)
    assert np.array_equal(got["news_index"], i0h) and np.array_equal(got["scores"], s0.cpu().numpy())
    assert "keys" not in got


@pytest.mark.gpu
def test_gpu_recommend_script_cap(tmp_path):
    """scripts/recommend.py --synthetic --cap 2 (the script has no CPU path)."""
    cmd = [sys.executable, str(REPO / "scripts" / "recommend.py"), "--synthetic", "--cap", "2", "--num-impressions",
           "200", "-k", "10", "--out-dir", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["cap"] == 2 and line["cap_by"] == "category"
    assert 1 <= line["max_group_count"] <= 2 and 0.0 <= line["at_cap_share"] <= 1.0 and line["distinct_groups"] >= 1.0
    rec = np.load(tmp_path / "recommendations.npy")
    assert rec.shape == (200, 10)
