"""Column-sliced pool+score (nr_slice_table, nr_pool_score_sliced; ops.pool_score(sliced=...)).

The sliced path is held to the bound tests/test_gpu_parity.py holds pool_score_kernel to
against a float64 re-pool of the same device tables (2e-5, f32 and bf16 tables alike), and to
at most twice today's kernel's own maximum error on the same inputs.
"""
import numpy as np
import pytest
import torch

from news_recommendation_project_v2_amd import engine, ops

N_NEWS = 300  # more rows than lanes
BOUND = 2e-5  # test_gpu_parity.test_pool_score_ragged_edges / test_full_size_mind_large_properties
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _impressions(n_imp: int, seed: int = 0):
    """Ragged CSR: the edge lengths first, then random ones; rows 0 and N - 1 and duplicate
    ids inside a segment are there by construction."""
    rng = np.random.default_rng(seed)
    hl = ([0, 1, 7, 8, 9, 63, 64, 65] + [int(v) for v in rng.integers(1, 90, 64)])[:n_imp]
    cl = ([2, 63, 64, 65, 130] * 13)[:n_imp]
    if n_imp == 1:
        hl, cl = [9], [65]
    hl, cl = np.array(hl, dtype=np.int64), np.array(cl, dtype=np.int64)
    hi = rng.integers(0, N_NEWS, int(hl.sum())).astype(np.int32)
    ci = rng.integers(0, N_NEWS, int(cl.sum())).astype(np.int32)
    hi[0], hi[-1] = 0, N_NEWS - 1
    ci[0], ci[-1] = N_NEWS - 1, 0
    if len(hi) > 12:
        hi[3] = hi[2]   # a duplicate inside the 7-row history
        hi[11] = hi[10]
    ci[1] = ci[0]       # and inside the first candidate list
    off = lambda l: np.concatenate([[0], np.cumsum(l)]).astype(np.int64)
    return hi, off(hl), ci, off(cl)


_CASES = {}


def _case(dev, pooler: str, dt: str, n_imp: int = 40):
    """Device tables, CSR and the float64 re-pool of them, made once per (pooler, dtype, I)."""
    key = (pooler, dt, n_imp)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(7)
    cand = torch.randn((N_NEWS, 1024), generator=g).to(DTYPES[dt])
    x = torch.randn((N_NEWS, 1024), generator=g)
    if pooler == "final":
        hist = torch.cat([x, torch.exp(0.5 * torch.randn((N_NEWS, 1024), generator=g))], dim=1).to(DTYPES[dt])
    else:
        hist = x.to(DTYPES[dt])
    hi, ho, ci, co = _impressions(n_imp)
    tab, cd = hist.double(), cand.double()
    ref = np.empty(int(co[-1]))
    for i in range(n_imp):
        rows = tab[torch.as_tensor(hi[ho[i]:ho[i + 1]], dtype=torch.long)]
        if pooler == "final":
            xx, p = rows[:, :1024], rows[:, 1024:]
            u = (xx * p).sum(0) / (p.sum(0) + 1e-10)
        else:
            u = rows.mean(0)  # NaN for an empty history, as the kernels give
            if pooler == "latent":
                u = u / u.norm().clamp_min(1e-12)
        e = cd[torch.as_tensor(ci[co[i]:co[i + 1]], dtype=torch.long)]
        ref[co[i]:co[i + 1]] = ((e @ u) / u.norm().clamp_min(1e-8) / e.norm(dim=1).clamp_min(1e-8)).numpy()
    cand_d = cand.to(dev)
    c = dict(hist=hist.to(dev), cand=cand_d, inv=ops.row_inv_norm(cand_d, 1e-8),
             csr=tuple(torch.as_tensor(a).to(dev) for a in (hi, ho, ci, co)), n_cand=int(co[-1]), ref=ref)
    _CASES[key] = c
    return c


def _run(c, pooler, sliced):
    hi, ho, ci, co = c["csr"]
    s, _ = ops.pool_score(pooler, c["hist"], c["cand"], c["inv"], hi, ho, ci, co, c["n_cand"], sliced=sliced)
    torch.cuda.synchronize()
    return s.cpu().numpy()


def _max_err(got, ref):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    return float(np.abs(got.astype(np.float64) - ref)[~nan].max())


@pytest.mark.gpu
@pytest.mark.parametrize("w", [64, 128])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("pooler", ["latent", "mean", "final"])
def test_sliced_matches_float64(gpu_device, pooler, dt, w):
    c = _case(gpu_device, pooler, dt)
    today = _max_err(_run(c, pooler, False), c["ref"])
    got = _run(c, pooler, w)
    err = _max_err(got, c["ref"])
    print(f"pooler={pooler} dtype={dt} W={w}: max err sliced {err:.3e}, today's kernel {today:.3e}")
    assert err <= BOUND, (err, BOUND)
    assert err <= 2 * today, (err, today)
    assert np.array_equal(got, _run(c, pooler, w), equal_nan=True)  # same bits from run to run


@pytest.mark.gpu
@pytest.mark.parametrize("n_imp", [1, 33])  # one impression; one more than a workgroup's 4 waves x 8
@pytest.mark.parametrize("pooler", ["latent", "final"])
def test_sliced_impression_counts(gpu_device, pooler, n_imp):
    c = _case(gpu_device, pooler, "bf16", n_imp)
    today = _max_err(_run(c, pooler, False), c["ref"])
    for w in ops.SLICE_WIDTHS:
        err = _max_err(_run(c, pooler, w), c["ref"])
        print(f"pooler={pooler} I={n_imp} W={w}: max err sliced {err:.3e}, today's kernel {today:.3e}")
        assert err <= BOUND and err <= 2 * today, (err, today)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [64, 128])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("parts", [1, 2])
def test_slice_table_is_a_permutation(gpu_device, dt, parts, w):
    g = torch.Generator().manual_seed(3)
    big = torch.randn((N_NEWS, parts * 1024 + 64), generator=g).to(DTYPES[dt]).to(gpu_device)
    table = big[:, :parts * 1024]  # a row stride wider than the row
    img = ops.slice_table(table, w, parts)
    want = table.reshape(N_NEWS, parts, 1024 // w, w).permute(2, 0, 1, 3).reshape(1024 // w, N_NEWS, parts * w)
    assert torch.equal(img.view(torch.uint8), want.contiguous().view(torch.uint8))
    back = ops.unslice_table(img, parts)
    assert torch.equal(back.view(torch.uint8), table.contiguous().view(torch.uint8))


@pytest.mark.gpu
def test_engine_sliced_path_reuses_its_buffers(gpu_device, monkeypatch):
    """The engine's sliced branch (forced at a small table): the scores of ops.pool_score on the
    same images, the same bits on a second step, no new buffers."""
    from news_recommendation_project_v2_amd import weights as W
    from news_recommendation_project_v2_amd.latent_attention import LatentAttentionModel
    m = LatentAttentionModel()
    m.load_state_dict(W.latent_attention_state_dict(5))
    monkeypatch.setattr(engine, "SLICED_W", 64)
    monkeypatch.setattr(engine, "SLICED_MIN_TABLE_BYTES", 0)
    hi, ho, ci, co = _impressions(40)
    eng = engine.PoolScoreEngine(m.to(gpu_device).eval(), dtype=torch.bfloat16, device=gpu_device)
    eng.load_news(W.news_table(3, N_NEWS, 1024, name="sliced"))
    eng.load_impressions(hi, np.diff(ho), ci, np.diff(co))
    assert eng._cand_image is not None and eng.user_idx is None
    s1 = eng.step()[0].clone()
    bufs = (eng._hist_image.data_ptr(), eng._cand_image.data_ptr(), eng._sliced_ws.data_ptr())
    s2 = eng.step()[0]
    assert bufs == (eng._hist_image.data_ptr(), eng._cand_image.data_ptr(), eng._sliced_ws.data_ptr())
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    today, _ = ops.pool_score("latent", eng.hist_table, eng.cand_table, eng.cand_inv, eng.hist_idx, eng.hist_off,
                              eng.cand_idx, eng.cand_off, eng.n_cand)
    ok = ~torch.isnan(today)
    assert torch.equal(torch.isnan(s2), ~ok) and float((s2 - today)[ok].abs().max()) <= 2 * BOUND
    _, users = eng.step(want_users=True)  # want_users: today's kernel
    assert users is not None and users.shape == (40, 1024)
    eng.load_impressions(hi, np.diff(ho), ci, np.diff(co), dedupe=False)  # the fused pass asked for: its bits
    assert torch.equal(eng.step()[0].view(torch.int32), today.view(torch.int32))


def test_dispatch_rule(monkeypatch):
    """Small tables, want_users and deduplicated histories go to today's kernels whatever
    the width; so does everything while SLICED_W is 0."""
    big = -(-engine.SLICED_MIN_TABLE_BYTES // 2048)  # the fewest bf16 rows of a table that large
    assert engine.SLICED_W in (0,) + ops.SLICE_WIDTHS and engine.SLICED_W_FINAL in (0,) + ops.SLICE_WIDTHS
    for w in (engine.SLICED_W, 64, 128):
        monkeypatch.setattr(engine, "SLICED_W", w)
        assert engine.sliced_width(big, torch.bfloat16, False, False) == w
        assert engine.sliced_width(big, torch.bfloat16, True, False) == 0
        assert engine.sliced_width(big, torch.bfloat16, False, True) == 0
        assert engine.sliced_width(big - 1, torch.bfloat16, False, False) == 0
        assert engine.sliced_width(4 * big, torch.float32, False, False) == 0  # f32 tables: not measured
        # the shapes the suite's other tests run at (up to 8,192 news; MIND-small-dev in f32)
        for n, dt in ((300, torch.float32), (700, torch.bfloat16), (8192, torch.float32), (42_416, torch.bfloat16)):
            assert engine.sliced_width(n, dt, False, False) == 0
        monkeypatch.setattr(engine, "SLICED_W_FINAL", w)
        assert engine.sliced_width(big, torch.bfloat16, False, False, "final") == w
        assert engine.sliced_width(big - 1, torch.bfloat16, False, False, "final") == 0
        assert engine.sliced_width(big, torch.bfloat16, True, False, "final") == 0
    monkeypatch.setattr(engine, "SLICED_W", 0)
    assert engine.sliced_width(10 ** 7, torch.bfloat16, False, False) == 0


def test_sliced_argument():
    assert ops.slice_width(False) == 0 and ops.slice_width(None) == 0 and ops.slice_width(0) == 0
    assert ops.slice_width(True) == ops.SLICE_W and ops.slice_width(64) == 64 and ops.slice_width(128) == 128
    with pytest.raises(Exception):
        ops.slice_width(32)


def test_dedupe_and_users_stay_on_todays_kernels(monkeypatch):
    """PoolScoreEngine.pool_score with a deduplicated history CSR never asks for a slice width."""
    monkeypatch.setattr(engine, "SLICED_W", 64)
    monkeypatch.setattr(engine, "SLICED_MIN_TABLE_BYTES", 0)
    calls = []
    eng = engine.PoolScoreEngine.__new__(engine.PoolScoreEngine)
    eng.user_idx = torch.zeros(2, dtype=torch.int32)
    eng.uhist_idx = eng.uhist_off = eng.cand_table = eng.cand_inv = eng.cand_idx = eng.cand_off = None
    eng.n_cand = 0
    monkeypatch.setattr(eng, "_pooled_users", lambda *a: torch.zeros((1, 1024)), raising=False)
    monkeypatch.setattr(ops, "score_users", lambda *a, **k: calls.append("score_users") or torch.zeros(0))
    monkeypatch.setattr(ops, "pool_score", lambda *a, **k: calls.append("pool_score"))
    eng.pool_score()
    assert calls == ["score_users"]


def test_header_and_bindings_agree():
    """include/newsrec_sliced.h declares what _lib.SLICED_SIGNATURES binds, argument for argument,
    and is part of the library's source hash and the Makefile's header list."""
    import re
    from pathlib import Path
    from news_recommendation_project_v2_amd import _lib
    text = (Path(_lib.INCLUDE) / "newsrec_sliced.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(nr_\w+)\s*\(([^)]*)\)\s*;", body)}
    assert sorted(decls) == sorted(_lib.SLICED_SIGNATURES)
    for name, args in decls.items():
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SLICED_SIGNATURES[name][1]), name
    assert "newsrec_sliced.h" in [p.name for p in _lib.hip_source_files()]
    assert "newsrec_sliced.h" in (Path(_lib.CSRC) / "Makefile").read_text()
