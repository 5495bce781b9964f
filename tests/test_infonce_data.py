"""The InfoNCE training data (data_utils.py:275-334, 512-578, 794-817) against the
reference's own outputs (tests/golden/infonce_dataset.npz, written by
tests/golden/make_golden_infonce.py), the loss reference against the reference's
commented loss (trainer.py:612-625), and the in-batch mask."""
from __future__ import annotations

import io
import sqlite3

import numpy as np
import torch
import torch.nn.functional as F

import contrastive_ref as cref
from conftest import golden, unflat
from news_recommendation_project_v2_amd import data_utils


def _labels(g):
    rows = unflat(g["labels_flat"], g["cand_len"])
    lab = np.empty(len(rows), dtype=object)
    lab[:] = [tuple(int(x) for x in r) for r in rows]
    return lab


def _dataset(g):
    return data_utils.FinalAttentionTrainInfoNCEDataset(
        g["hist"], g["hist_len"], g["cand"], g["cand_len"], _labels(g), batch_size=int(g["batch_size"]),
        num_neg_per_pos=int(g["num_neg_per_pos"]), rng=np.random.default_rng(int(g["rng_seed"])))


def test_infonce_dataset_and_collate_match_reference():
    g = golden("infonce_dataset")
    ds = _dataset(g)
    want = g["pos_neg_indices"]
    assert (want[:, 1:-1] < 0).any() and want.shape[1] == int(g["num_neg_per_pos"]) + 2
    assert ds.pos_neg_indices.dtype == want.dtype and np.array_equal(ds.pos_neg_indices, want)
    assert len(ds) == len(want)
    bs = int(g["batch_size"])
    assert ds.batches()[0] == (0, bs) and ds.batches()[-1][1] == len(ds)
    out = data_utils.final_attention_train_infonce_collate_fn([ds[i] for i in range(bs)])
    for got, key in zip(out, ("b0_hidx", "b0_hmask", "b0_hrev", "b0_pn")):
        assert got.dtype == torch.int32, key
        assert np.array_equal(got.numpy(), g[key]), key
    ds.reset()
    assert np.array_equal(ds.pos_neg_indices, g["pos_neg_indices_after_reset"])


def test_split_infonce_pads_and_draws():
    """Fewer than K negatives: all of them, then -1, and no generator call."""
    rng = np.random.default_rng(3)
    state = rng.bit_generator.state
    cands = np.empty(2, dtype=object)
    cands[:] = [np.array([7, 8, 9], dtype=np.int32), np.array([4], dtype=np.int32)]
    out = data_utils.split_impressions_pos_neg_infonce(rng, cands, [(1, 0, 1), (1,)], num_neg_per_pos=2)
    assert rng.bit_generator.state == state
    assert out.dtype == np.int32
    assert out.tolist() == [[7, 9, 4], [8, 8, -1], [-1, -1, -1], [0, 0, 1]]


def test_loss_reference_equals_the_commented_form():
    """Sampled form, tau = 1: tests/contrastive_ref.py's loss = CrossEntropyLoss()(res
    with -inf pads, zeros) computed as trainer.py:612-625 writes it."""
    gen = torch.Generator().manual_seed(5)
    B, K, U, D = 6, 4, 9, 32
    users = torch.randn((B, D), generator=gen)
    emb = torch.randn((U, D), generator=gen)
    rng = np.random.default_rng(8)
    pn = rng.integers(0, U, (B, 1 + K))
    pn[1, 3:] = -1
    pn[4, 1:] = -1  # a row whose only column is its positive
    pn_t = torch.as_tensor(pn)
    rev = torch.arange(B)
    res = F.cosine_similarity(users[rev.unsqueeze(-1)], emb[pn_t], dim=-1)
    res[pn_t < 0] = torch.tensor(float("-inf"))
    want = torch.nn.CrossEntropyLoss()(res, torch.zeros(len(res), dtype=torch.int64))
    cand, target, mask = cref.sampled_spec(pn)
    got = cref.infonce_loss(users, emb, cand, target, mask, 1.0)
    assert abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want))), (float(got), float(want))
    z = cref.infonce_logits(users, emb, cand, mask, 1.0)
    for b in range(B):
        assert torch.equal(torch.isinf(z[b, b * (1 + K):(b + 1) * (1 + K)]), pn_t[b] < 0)


def _token_db(n_news, D=1024):
    conn = sqlite3.connect(":memory:")
    conn.execute("CREATE TABLE tensors (id INTEGER PRIMARY KEY, data BLOB)")
    for i in range(n_news):
        buf = io.BytesIO()
        torch.save(torch.full((1 + i % 3, D), float(i)).half(), buf)
        conn.execute("INSERT INTO tensors (data) VALUES (?)", (buf.getvalue(),))
    return conn


def test_in_batch_mask_excludes_pads_and_other_clicks():
    """Three impressions, K = 2.  Impression 0 clicked news 10 and 11 (two rows), 1
    clicked 12 with one negative only (a pad), 2 clicked 13.  Row b leaves out exactly
    the pads and the columns, other than its target, that hold a clicked news of its
    own impression."""
    conn = _token_db(20)
    h = [np.array([1, 2]), np.array([1, 2]), np.array([3]), np.array([4, 5, 6])]
    rows = [(h[0], np.array([10, 14, 15], dtype=np.int32)), (h[1], np.array([11, 15, 10], dtype=np.int32)),
            (h[2], np.array([12, 11, -1], dtype=np.int32)), (h[3], np.array([13, 10, 12], dtype=np.int32))]
    clicks = [np.array([10, 11]), np.array([10, 11]), np.array([12]), np.array([13])]
    last, hidx, hoff, cand, target, mask = data_utils.contrastive_batch_csr(conn, rows, "in_batch", clicks)
    news = np.concatenate([r[1] for r in rows])
    uniq = np.unique(np.concatenate(h + [news[news >= 0]]))
    assert last.shape == (len(uniq), 1024) and hoff.tolist() == [0, 2, 4, 5, 8]
    assert np.array_equal(uniq[hidx], np.concatenate(h))
    assert cand.dtype == np.int32 and target.dtype == np.int32 and mask.dtype == np.uint8
    assert np.array_equal(np.where(cand >= 0, uniq[np.maximum(cand, 0)], -1), news)
    assert target.tolist() == [0, 3, 6, 9]
    # columns:   10 14 15 | 11 15 10 | 12 11 -1 | 13 10 12
    want = np.array([[0, 0, 0, 1, 0, 1, 0, 1, 1, 0, 1, 0],
                     [1, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1],
                     [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]], dtype=np.uint8)
    assert np.array_equal(mask, want)
    # the sampled form: the row's own block, minus the pads
    _, _, _, cand_s, target_s, mask_s = data_utils.contrastive_batch_csr(conn, rows, "sampled")
    assert np.array_equal(cand_s, cand) and np.array_equal(target_s, target)
    want_s = np.ones((4, 12), dtype=np.uint8)
    for b in range(4):
        want_s[b, 3 * b:3 * b + 3] = 0
    want_s[:, 8] = 1
    assert np.array_equal(mask_s, want_s)
    conn.close()


def test_infonce_dataset_positives_of():
    g = golden("infonce_dataset")
    ds = _dataset(g)
    cands = data_utils.group_items(g["cand"], g["cand_len"])
    for i in range(len(ds)):
        imp = int(ds.pos_neg_indices[i, -1])
        clicks = ds.positives_of(i)
        assert int(ds.pos_neg_indices[i, 0]) in clicks
        assert sorted(clicks.tolist()) == sorted(int(n) for n, y in zip(cands[imp], _labels(g)[imp]) if y)
