"""The per-click attribution entry of the C ABI (include/newsrec_explain.h) on the host:
signature table, the refusals that need no device, the float64 reference of the GPU tests
(tests/explain_ref.py) against the oracle's cosine scores and on the contract's corner
cases, evaluation.explanation_metrics, and the new Python surface."""
import inspect
import re

import numpy as np
import pytest
import torch

import explain_ref
from conftest import REPO
from news_recommendation_project_v2_amd import _lib
from news_recommendation_project_v2_amd import weights as W
from news_recommendation_project_v2_amd.evaluation import explanation_metrics
from oracle import pool_ref

HEADER = REPO / "include" / "newsrec_explain.h"
F32, BF16 = _lib.NR_F32, _lib.NR_BF16
FINAL, LATENT, MEAN = _lib.NR_POOL_FINAL, _lib.NR_POOL_LATENT, _lib.NR_POOL_MEAN
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.is_file():
        pytest.skip("libnewsrec_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_explain_signatures_cover_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = dict(re.findall(r"\b(nr_[a-z0-9_]+)\s*\(([^)]*)\)", text))
    assert sorted(decls) == sorted(_lib.EXPLAIN_SIGNATURES)
    for f, args in decls.items():
        assert hasattr(lib, f), f
        assert len(args.split(",")) == len(_lib.EXPLAIN_SIGNATURES[f][1]), f
    assert int(re.search(r"#define NR_EXPLAIN_TOP_MAX (\d+)", text).group(1)) == _lib.NR_EXPLAIN_TOP_MAX == 8
    assert explain_ref.TOP_MAX == _lib.NR_EXPLAIN_TOP_MAX
    # the build hash covers the new sources
    names = [p.name for p in _lib.hip_source_files()]
    assert "explain.hip" in names and "newsrec_explain.h" in names
    mk = (REPO / "news_recommendation_project_v2_amd" / "csrc" / "Makefile").read_text()
    assert "explain.hip" in mk and "newsrec_explain.h" in mk


def test_explain_refusals_on_the_host(lib):
    """Every refusal of the contract returns its code and message before any device call
    (this host has none; a launch would fail differently)."""
    raw = np.zeros(1 << 16, dtype=np.uint8)
    P = raw.ctypes.data + (-raw.ctypes.data) % 256
    err = lambda: lib.nr_last_error().decode()

    def call(pooler=LATENT, dtype=F32, dim=1024, ht=P, hld=1024, N=100, ct=P, cld=1024, inv=P, U=4, hi=P, ho=P, li=P,
             K=10, T=3, tp=P, tv=P, so=None, co=None):
        return lib.nr_explain_scores(pooler, dtype, dim, ht, hld, N, ct, cld, inv, U, hi, ho, li, K, T, tp, tv, so, co,
                                     None)

    assert call(dim=512) == UNSUPPORTED and "dim 512 unsupported" in err()
    for pooler in (_lib.NR_POOL_NONE, 3):
        assert call(pooler=pooler) == INVALID and "bad pooler" in err()
    for dtype in (_lib.NR_F16, 7):
        assert call(dtype=dtype) == INVALID and "bad dtype" in err()
    for k in (0, -1, 65):
        assert call(K=k) == INVALID and f"K = {k} outside [1, 64]" in err()
    for t in (0, -1, 9):
        assert call(T=t) == INVALID and f"T = {t} outside [1, 8]" in err()
    assert call(T=0, tp=None, tv=None, so=P) == INVALID and "not device memory" in err()  # T is unused without the top lists
    assert call(tp=None) == INVALID and "go together" in err()
    assert call(tv=None) == INVALID and "go together" in err()
    assert call(tp=None, tv=None) == INVALID and "no output" in err()
    for u in (0, -1, 1 << 31):
        assert call(U=u) == INVALID and f"U = {u}" in err()
    for n in (0, 1 << 31):
        assert call(N=n) == INVALID and f"N = {n}" in err()
    assert call(hld=1016) == INVALID and "leading dimension" in err()
    assert call(cld=1016) == INVALID and "leading dimension" in err()
    assert call(pooler=FINAL, hld=1024) == INVALID and "leading dimension" in err()  # a FINAL row is x | p
    assert call(pooler=MEAN, hld=1026) == INVALID and "16-byte" in err()             # f32 rows of 4104 bytes
    assert call(dtype=BF16, cld=1028) == INVALID and "16-byte" in err()              # bf16 rows of 2056 bytes
    assert call(ht=P + 4) == INVALID and "16-byte" in err()
    assert call(ct=P + 8) == INVALID and "16-byte" in err()
    for null in ("ht", "ct", "inv", "hi", "ho", "li"):
        assert call(**{null: None}) == INVALID and "null pointer" in err(), null
    # host pointers, through the residency check
    assert call() == INVALID and "not device memory" in err()
    assert call(pooler=FINAL, hld=2048, K=64, T=8, so=P, co=P) == INVALID and "not device memory" in err()


def _case(rng, n_news, lens, k):
    hist_idx = rng.integers(0, n_news, int(np.sum(lens)))
    hist_off = np.concatenate([[0], np.cumsum(lens)])
    return hist_idx, hist_off, rng.integers(0, n_news, (len(lens), k))


@pytest.mark.parametrize("pooler", ["final", "latent"])
def test_reference_sums_are_the_oracle_scores(pooler):
    """The decomposition is the score: on an N(0, 1) news table, through the pooler's own
    per-news transform, the contributions of a history add up to the evaluation oracle's
    cosine of (user, listed news)."""
    rng = np.random.default_rng(31)
    n_news, k = 60, 7
    table = torch.from_numpy(rng.standard_normal((n_news, 1024)).astype(np.float32))
    sd = W.final_attention_state_dict(5) if pooler == "final" else W.latent_attention_state_dict(5, ln_random=True)
    lens = np.array([1, 2, 5, 17, 33])
    hist_idx, hist_off, lst = _case(rng, n_news, lens, k)
    want = pool_ref.cos_sim_scores_per_news(pooler, sd, hist_idx, lens, lst.reshape(-1), np.full(len(lens), k),
                                            table).numpy().reshape(len(lens), k)
    htab = pool_ref.per_news_tables(pooler, sd, table).double().numpy()
    ctab = table.double().numpy()
    cinv = 1.0 / np.maximum(np.linalg.norm(ctab, axis=1), 1e-8)
    ref = explain_ref.explain(pooler, htab, ctab, cinv, hist_idx, hist_off, lst, top=3)
    diff = float(np.abs(ref["sums"] - want).max())
    print(f"{pooler}: max |sum of contributions - oracle cosine| = {diff:.3e}")
    assert diff <= 1e-6
    # ... and the share rows add up to the pooled user
    g, u = explain_ref.shares(pooler, htab[hist_idx[hist_off[3]:hist_off[4]]])
    assert np.allclose(g.sum(axis=0), u, rtol=0, atol=1e-12)
    if pooler == "latent":
        assert abs(np.linalg.norm(u) - 1.0) < 1e-12


def test_reference_ties_and_pads():
    rng = np.random.default_rng(32)
    n_news = 20
    htab = rng.standard_normal((n_news, 1024))
    ctab = rng.standard_normal((n_news, 1024))
    cinv = 1.0 / np.linalg.norm(ctab, axis=1)
    # news 4 three times, news 9 twice: equal contributions, ascending position
    hist = np.array([4, 7, 9, 4, 2, 9, 4])
    lst = np.array([[3, -1, 11, n_news, 5, -7]])
    ref = explain_ref.explain("latent", htab, ctab, cinv, hist, np.array([0, len(hist)]), lst, top=8)
    assert ref["valid"].tolist() == [[True, False, True, False, True, False]]
    a = ref["a"]
    assert np.array_equal(a[0], a[3]) and np.array_equal(a[0], a[6]) and np.array_equal(a[2], a[5])
    for j in (1, 3, 5):  # pads: column 0, sum 0, positions -1, values -inf
        assert not a[:, j].any() and ref["sums"][0, j] == 0.0
        assert (ref["top_pos"][0, j] == -1).all() and np.isneginf(ref["top_val"][0, j]).all()
    for j in (0, 2, 4):
        pos, val, gaps = ref["top_pos"][0, j], ref["top_val"][0, j], ref["gaps"][0, j]
        assert sorted(pos[:7].tolist()) == list(range(7)) and pos[7] == -1 and np.isneginf(val[7])
        assert (np.diff(val[:7]) <= 0).all() and np.array_equal(val[:7], a[pos[:7], j])
        where = {int(p): i for i, p in enumerate(pos[:7])}
        assert where[0] + 1 == where[3] and where[3] + 1 == where[6] and where[2] + 1 == where[5]
        # a zero gap between two occurrences of one news is decidable; the others are real gaps
        assert np.isinf(gaps[where[0]]) and np.isinf(gaps[where[3]]) and np.isinf(gaps[where[2]])
        assert np.isinf(gaps[6]) and np.isinf(gaps[7])  # nothing follows the last entry
        real = [i for i in range(6) if i not in (where[0], where[3], where[2])]
        assert all(gaps[i] == val[i] - val[i + 1] and gaps[i] > 0 for i in real)
    # a tie between different news is a zero gap, resolved by position
    pos, val, gaps = explain_ref.top_t(np.array([0.5, 1.0, 0.5, 1.0]), np.array([1, 2, 3, 4]), 3)
    assert pos.tolist() == [1, 3, 0] and gaps.tolist() == [0.0, 0.5, 0.0]
    # an empty history: nothing but pads' values
    ref = explain_ref.explain("final", np.zeros((n_news, 2048)), ctab, cinv, np.zeros(0, int), np.array([0, 0]), lst)
    assert (ref["top_pos"] == -1).all() and np.isneginf(ref["top_val"]).all() and not ref["sums"].any()
    assert ref["a"].shape == (0, 6)
    # the three poolers on one history: FINAL with p = 1 is MEAN; LATENT is MEAN rescaled, so its
    # contributions are MEAN's (the cosine does not see the user's length)
    rows = np.concatenate([htab, np.ones_like(htab)], axis=1)
    h3, off3 = np.array([1, 5, 8]), np.array([0, 3])
    fin = explain_ref.explain("final", rows, ctab, cinv, h3, off3, lst, top=2)
    mean = explain_ref.explain("mean", htab, ctab, cinv, h3, off3, lst, top=2)
    lat = explain_ref.explain("latent", htab, ctab, cinv, h3, off3, lst, top=2)
    assert np.allclose(fin["a"], mean["a"], rtol=0, atol=1e-12) and np.allclose(lat["a"], mean["a"], rtol=0, atol=1e-12)
    assert np.array_equal(fin["top_pos"], mean["top_pos"])
    u = htab[h3].mean(axis=0)
    want = (u @ ctab[3]) / np.linalg.norm(u) * cinv[3]
    assert abs(mean["sums"][0, 0] - want) < 1e-12


def test_explanation_metrics():
    ninf = -np.inf
    why = np.array([[[0.6, 0.3, 0.1], [0.2, 0.1, ninf]],
                    [[-0.1, -0.2, -0.3], [ninf, ninf, ninf]],
                    [[0.5, 0.25, 0.0], [0.4, ninf, ninf]]])
    scores = np.array([[1.0, 0.4], [-0.8, ninf], [0.5, 0.4]])
    m = explanation_metrics(why, scores)
    assert m["recommendations"] == 5
    assert m["negative_top"] == pytest.approx(1 / 5)
    assert m["top1_share"] == pytest.approx((0.6 + 0.5 + 1.0 + 1.0) / 4)
    assert m["topT_share"] == pytest.approx((1.0 + 0.75 + 1.5 + 1.0) / 4)
    assert all(isinstance(v, float) for k, v in m.items() if k != "recommendations")
    # float32 inputs as the API returns them
    m32 = explanation_metrics(why.astype(np.float32), scores.astype(np.float32))
    assert m32["top1_share"] == pytest.approx(m["top1_share"], abs=1e-6)
    empty = explanation_metrics(np.full((2, 3, 2), ninf), np.full((2, 3), ninf))
    assert empty["recommendations"] == 0 and np.isnan(empty["top1_share"]) and np.isnan(empty["negative_top"])
    with pytest.raises(ValueError):
        explanation_metrics(why, scores[:, :1])
    with pytest.raises(ValueError):
        explanation_metrics(why[:, :, 0], scores)
    with pytest.raises(ValueError):
        explanation_metrics(why[:, :, :0], scores)


def test_new_symbols_and_old_errors():
    import news_rec_utils.data_model_helper as alias
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    from news_recommendation_project_v2_amd import evaluation, ops
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    assert callable(ops.explain_scores) and callable(evaluation.explanation_metrics)
    assert callable(PoolScoreEngine.explain) and callable(PoolScoreEngine.recommend_explained)
    assert alias.get_top_k_recommendations is dmh.get_top_k_recommendations
    sig = inspect.signature(ops.explain_scores)
    assert list(sig.parameters) == ["pooler", "hist_table", "cand_table", "cand_inv_norm", "hist_idx", "hist_off",
                                    "list_idx", "top", "want_sum", "want_matrix", "out"]
    assert sig.parameters["top"].default == 3
    sig = inspect.signature(PoolScoreEngine.recommend_explained)
    assert [(n, p.default) for n, p in sig.parameters.items()][2:] == [
        ("top", 3), ("lam", None), ("pool", 64), ("exclude_history", True), ("user_block", None)]
    sig = inspect.signature(dmh.get_top_k_recommendations)
    assert sig.parameters["explain"].default is None and list(sig.parameters)[-1] == "explain"
    # the helper's argument errors come before anything touches a device
    hl, hi = np.array([2, 1]), np.array([0, 1, 2])
    table = torch.zeros((4, 1024))
    with pytest.raises(ValueError, match="pool needs diversify"):
        dmh.get_top_k_recommendations(hi, hl, table, None, 3, pool=32)
    with pytest.raises(ValueError, match="pool needs diversify"):
        dmh.get_top_k_recommendations(hi, hl, table, None, 3, pool=32, explain=3)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="explain"):
            dmh.get_top_k_recommendations(hi, hl, table, None, 3, explain=bad)
    # the wrapper refuses host tensors and bad arguments before the library is reached
    li = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(_lib.NewsRecHIPError, match="device tensors"):
        ops.explain_scores("latent", table, table, torch.ones(4), torch.as_tensor(hi, dtype=torch.int32),
                           torch.as_tensor([0, 2, 3]), li)
