#!/usr/bin/env python3
"""Time the MMR re-ranking of retrieved lists at the §3.8 probe shape --
255,990 distinct users x 72,023 news, bf16, pool 64, K = 10 -- against the route a torch
user would take, interleaved in one process.

    python tools/rerank_probe.py [--pooler final] [--rounds 3] [--iters 2] [--out FILE.json]
                                 [--users 255990] [--news 72023] [--pool 64] [-k 10] [--lam 0.7]
                                 [--torch-block 8192] [--no-torch]

The lists are PoolScoreEngine's own top-`pool` lists of synthetic users (histories with the
benchmark's lengths).  Each round times with device events, after a warm-up of every route:
  rerank             ops.rerank_mmr alone on those lists (gather + 64 x 64 cosines + K rounds)
  recommend_diverse  PoolScoreEngine.recommend_diverse whole (transform + norms + pooling +
                     retrieval of `pool` + re-ranking)
  recommend_pool     PoolScoreEngine.recommend(pool): the retrieval before it, for scale
  torch              the same lists: table[idx] in user blocks, bmm, scale by the inverse
                     norms, K rounds of masked arg-max / maximum
and prints one JSON line with the medians, the gather rate of `rerank` against the
U x pool x 2 KiB it reads (the table itself is far smaller and may be served from the
last-level cache: the figure says nothing about which bound applies), the share of users
on which the torch route picks the same lists, and, per lambda of --lams, the mean
intra-list diversity and mean relevance before and after (random weights: these numbers
only show the plumbing).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from news_recommendation_project_v2_amd import ops, weights as W  # noqa: E402
from news_recommendation_project_v2_amd.engine import PoolScoreEngine  # noqa: E402
from news_recommendation_project_v2_amd.evaluation import diversity_metrics  # noqa: E402
from news_recommendation_project_v2_amd.latent_attention import LatentAttentionModel  # noqa: E402
from news_recommendation_project_v2_amd.modeling_utils import FinalAttention  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_route(table, inv, idx, rel, k, lam, block):
    """Greedy MMR in torch ops on the same lists (every entry valid): positions int64 [U, k]."""
    U, M = idx.shape
    out = torch.empty((U, k), dtype=torch.int64, device=idx.device)
    eye = torch.eye(M, dtype=torch.bool, device=idx.device)
    for u0 in range(0, U, block):
        ix = idx[u0:u0 + block].long()
        r = rel[u0:u0 + block]
        E = table[ix]                                    # [B, M, D] materialised
        S = torch.bmm(E, E.transpose(1, 2)).float()
        ci = inv[ix]
        S = (S * ci[:, :, None]) * ci[:, None, :]
        S.masked_fill_(eye, 0.0)
        left = torch.ones_like(r, dtype=torch.bool)
        ms = torch.full_like(r, float("-inf"))
        rows = torch.arange(ix.shape[0], device=idx.device)
        for t in range(k):
            obj = r if t == 0 else lam * r - (1.0 - lam) * ms
            p = torch.argmax(torch.where(left, obj, torch.full_like(obj, float("-inf"))), dim=1)
            out[u0:u0 + block, t] = p
            left[rows, p] = False
            ms = torch.maximum(ms, S[rows, p])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--users", type=int, default=255_990)
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--lams", default="0.3,0.5,0.7,1.0")
    ap.add_argument("--torch-block", type=int, default=8192)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--pooler", choices=["final", "latent"], default="final")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1234)
    U, N, M, k, lam = args.users, args.news, args.pool, args.k, args.lam
    hl = np.clip(rng.geometric(1 / 33.0, U), 1, 600).astype(np.int32)
    hi = rng.integers(0, N, int(hl.sum())).astype(np.int32)
    table = W.news_table(1234, N, 1024, name="topk-probe")
    if args.pooler == "final":
        m = FinalAttention(1024, 4096)
        m.load_state_dict(W.final_attention_state_dict(1234))
    else:
        m = LatentAttentionModel()
        m.load_state_dict(W.latent_attention_state_dict(1234, ln_random=True))
    eng = PoolScoreEngine(m.to(dev).eval(), dtype=torch.bfloat16, device=dev)
    eng.load_news(table)
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(U, np.int32), dedupe=False)
    pidx, prel = eng.recommend(M)
    tab, inv = eng.cand_table, eng.cand_inv
    o = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev),
         torch.empty((U, k), dtype=torch.int32, device=dev), None, None)
    fns = {"rerank": lambda: ops.rerank_mmr(tab, inv, pidx, prel, k, lam, want_pos=True, out=o),
           "recommend_diverse": lambda: eng.recommend_diverse(k, lam, pool=M),
           "recommend_pool": lambda: eng.recommend(M)}
    if not args.no_torch:
        fns["torch"] = lambda: torch_route(tab, inv, pidx, prel, k, lam, args.torch_block)
    for fn in fns.values():
        timed(fn, 1)
    res = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            res[n].append(timed(fn, args.iters))
    gathered = float(U) * M * 1024 * tab.element_size()
    out = {"U": U, "N": N, "dtype": "bf16", "pooler": args.pooler, "pool": M, "K": k, "lambda": lam,
           "rounds": args.rounds, "iters": args.iters, "gathered_gb": round(gathered / 1e9, 2),
           "table_mb": round(N * 1024 * tab.element_size() / 1e6, 1)}
    for n, v in res.items():
        out[n + "_ms"] = round(statistics.median(v), 3)
        out[n + "_ms_all"] = [round(x, 3) for x in v]
    out["rerank_gather_gbps"] = round(gathered / out["rerank_ms"] / 1e6, 1)
    out["rerank_share_of_recommend_pool"] = round(out["rerank_ms"] / out["recommend_pool_ms"], 4)
    if not args.no_torch:
        same = (torch_route(tab, inv, pidx, prel, k, lam, args.torch_block) == o[2].long()).all(dim=1)
        out["torch_same_lists_share"] = round(float(same.float().mean()), 6)
        out["torch_over_rerank"] = round(out["torch_ms"] / out["rerank_ms"], 2)
    out["quality"] = []
    for l in (float(x) for x in args.lams.split(",")):
        _, r_after, ild = ops.rerank_mmr(tab, inv, pidx, prel, k, l, want_ild=True)
        q = diversity_metrics(ild.cpu().numpy(), rel_before=prel[:, :k].cpu().numpy(), rel_after=r_after.cpu().numpy())
        out["quality"].append({"lambda": l, **{n: round(v, 6) for n, v in q.items() if n != "lists"}})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
