"""Generate tests/golden/infonce_dataset.npz by running the REAL reference
(build container only; same import shims as make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_infonce.py

The reference's FinalAttentionTrainInfoNCEDataset (data_utils.py:512-578, over
split_impressions_pos_neg_infonce, :275-334) and
final_attention_train_infonce_collate_fn (:794-817) on a seeded synthetic set:
25 impressions, news ids < 50, K = 5 negatives per positive, batch size 8, with
impressions that have fewer than K negatives (-1 pads), several positives, and
a single candidate.  Stored: the inputs, ``pos_neg_indices`` after construction
and after one ``reset()``, and the four collate outputs of the first batch.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

K, BATCH, N_NEWS, N_IMP = 5, 8, 50, 25


def infonce_inputs(seed: int = 415):
    rng = np.random.default_rng(seed)
    h = rng.integers(1, 7, N_IMP).astype(np.int32)
    c = rng.integers(2, 13, N_IMP).astype(np.int32)
    c[3] = 1    # a single candidate (clicked): no negative at all
    c[7] = 3    # fewer than K negatives
    c[11] = 12  # several positives over many negatives
    labels = []
    for i, ci in enumerate(c):
        lab = (rng.random(ci) < 0.3).astype(int)
        lab[0] = 1
        if ci > 1:
            lab[-1] = 0
        if i == 11:
            lab[:4] = 1
        # (every impression keeps a positive: the reference's row-index concatenate
        # cannot cast the empty list of an impression without one)
        labels.append(tuple(int(x) for x in lab))
    hist = rng.integers(0, N_NEWS, int(h.sum())).astype(np.int32)
    # two impressions share one history (the collate makes histories unique)
    hist[int(h[:2].sum()):int(h[:3].sum())] = rng.integers(0, N_NEWS, int(h[2]))
    cand = rng.integers(0, N_NEWS, int(c.sum())).astype(np.int32)
    return h, c, hist, cand, labels


def main():
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    import make_golden
    _, du, _, _, _ = make_golden.import_reference()
    h, c, hist, cand, labels = infonce_inputs()
    lab = np.empty(len(labels), dtype=object)
    lab[:] = labels
    ds = du.FinalAttentionTrainInfoNCEDataset(hist, h, cand, c, lab, batch_size=BATCH, num_neg_per_pos=K,
                                              rng=np.random.default_rng(1234))
    pni0 = ds.pos_neg_indices.copy()
    rows0 = [ds[i] for i in range(min(BATCH, len(ds)))]
    hidx, hmask, hrev, pn = du.final_attention_train_infonce_collate_fn(rows0)
    ds.reset()
    pni1 = ds.pos_neg_indices.copy()
    assert (pni0[:, 1:-1] < 0).any(), "the fixture must contain pad columns"
    np.savez_compressed(HERE / "infonce_dataset.npz", hist=hist, hist_len=h, cand=cand, cand_len=c,
                        labels_flat=np.concatenate([np.array(l) for l in labels]).astype(np.int64),
                        batch_size=np.array(BATCH), num_neg_per_pos=np.array(K), rng_seed=np.array(1234),
                        pos_neg_indices=pni0, pos_neg_indices_after_reset=pni1,
                        b0_hidx=hidx.numpy(), b0_hmask=hmask.numpy(), b0_hrev=hrev.numpy(), b0_pn=pn.numpy())
    print("pos_neg_indices", pni0.shape, pni0.dtype, "pads", int((pni0 < 0).sum()))


if __name__ == "__main__":
    main()
