#!/usr/bin/env python3
"""Time top-K retrieval over the whole news table at the MIND-large dev
shape -- 255,990 distinct users x 72,023 news, bf16, K = 10 and 64 -- against the route a
torch user would take, interleaved in one process.

    python tools/topk_probe.py [--pooler final] [--rounds 3] [--iters 2] [--out FILE.json]
                               [--users 255990] [--news 72023] [--band-users 10000] [--no-torch]

Per pooler's user rows (synthetic histories with the benchmark's lengths, pooled by the
engine) and per K, each round times with device events, after a warm-up of every shape:
  recommend   PoolScoreEngine.recommend (transform + norms + pooling + retrieval)
  topk        ops.topk_users alone (bf16 pre-pass, stage 1, stage 2), history excluded
  torch       users.bfloat16() @ table.T in user blocks that fit memory, scaled by
              cand_inv, then torch.topk -- no exclusion, so it does less
and prints one JSON line with the medians: ms per pass, executed TFLOP/s of the
2 U N 1024 product (against the 2.5 PF bf16 peak), workspace bytes.  The stage split
(stage 1 / merge / re-score / sort) comes from a kernel trace of a run of its own.

The bf16 swap band: over `--band-users` sampled users, every news is scored on the
evaluation path (ops.score_users); reported are the share of returned rows that are not
in the top K by that score and the largest deficit of such a row below the K-th best.
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


def torch_route(users, table, inv, k, block):
    out_i = torch.empty((users.shape[0], k), dtype=torch.int64, device=users.device)
    for u0 in range(0, users.shape[0], block):
        s = users[u0:u0 + block].bfloat16() @ table.T
        s *= inv.to(s.dtype)[None, :]
        out_i[u0:u0 + block] = torch.topk(s, k, dim=1).indices
    return out_i


def swap_band(users, table, inv, k, n_sample, rng):
    """(share of returned rows outside the evaluation-path top K, largest deficit) over sampled users."""
    U, N = users.shape[0], table.shape[0]
    pick = torch.as_tensor(np.sort(rng.choice(U, min(n_sample, U), replace=False))).to(users.device)
    sub = users[pick].contiguous()
    idx, _ = ops.topk_users(sub, table, inv, k)
    bad, worst, blk = 0, 0.0, 500
    every = torch.arange(N, dtype=torch.int32, device=users.device).repeat(blk)
    for u0 in range(0, sub.shape[0], blk):
        n = min(blk, sub.shape[0] - u0)
        full = ops.score_users(sub, torch.arange(u0, u0 + n, dtype=torch.int32, device=users.device), table, inv,
                               every[:n * N], torch.arange(n + 1, dtype=torch.int64, device=users.device) * N,
                               n * N).reshape(n, N)
        kth = torch.topk(full, k, dim=1).values[:, -1:]
        got = torch.gather(full, 1, idx[u0:u0 + n].long())
        out = got < kth
        bad += int(out.sum())
        if bool(out.any()):
            worst = max(worst, float((kth - got)[out].max()))
    return bad / (sub.shape[0] * k), worst, int(sub.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--users", type=int, default=255_990)
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--band-users", type=int, default=10_000)
    ap.add_argument("--torch-block", type=int, default=16_384)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--pooler", choices=["final", "latent", "both"], default="both")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1234)
    U, N = args.users, args.news
    hl = np.clip(rng.geometric(1 / 33.0, U), 1, 600).astype(np.int32)
    hi = rng.integers(0, N, int(hl.sum())).astype(np.int32)
    table = W.news_table(1234, N, 1024, name="topk-probe")
    flop = 2.0 * U * N * 1024
    out = {"U": U, "N": N, "dtype": "bf16", "rounds": args.rounds, "iters": args.iters, "gemm_tflop": flop / 1e12,
           "hist_rows": int(hl.sum()), "chunk_rows": int(ops._lib.load().nr_topk_chunk_rows()), "cases": []}
    for pooler in (["final", "latent"] if args.pooler == "both" else [args.pooler]):
        if pooler == "final":
            m = FinalAttention(1024, 4096)
            m.load_state_dict(W.final_attention_state_dict(1234))
        else:
            m = LatentAttentionModel()
            m.load_state_dict(W.latent_attention_state_dict(1234, ln_random=True))
        eng = PoolScoreEngine(m.to(dev).eval(), dtype=torch.bfloat16, device=dev)
        eng.load_news(table)
        eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(U, np.int32), dedupe=False)
        eng.recommend(1)  # transform, norms and the pooled users
        users, tab, inv = eng._users, eng.cand_table, eng.cand_inv
        for k in (10, 64):
            ws = torch.empty(ops.topk_workspace_bytes(torch.bfloat16, U, N, k), dtype=torch.uint8, device=dev)
            o = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev))
            fns = {"recommend": lambda: eng.recommend(k),
                   "topk": lambda: ops.topk_users(users, tab, inv, k, eng.hist_idx, eng.hist_off, out=o, workspace=ws)}
            if not args.no_torch:
                fns["torch"] = lambda: torch_route(users, tab, inv, k, args.torch_block)
            for fn in fns.values():
                timed(fn, 1)
            res = {n: [] for n in fns}
            for _ in range(args.rounds):
                for n, fn in fns.items():
                    res[n].append(timed(fn, args.iters))
            case = {"pooler": pooler, "K": k, "workspace_bytes": int(ws.numel())}
            for n, v in res.items():
                ms = statistics.median(v)
                case[n + "_ms"] = round(ms, 3)
                case[n + "_ms_all"] = [round(x, 3) for x in v]
                case[n + "_tflops"] = round(flop / ms / 1e9, 1)
            case["topk_share_of_bf16_peak"] = round(flop / case["topk_ms"] / 1e9 / 2500.0, 4)
            if args.band_users:
                share, worst, n_s = swap_band(users, tab, inv, k, args.band_users, rng)
                case.update(band_users=n_s, band_share_outside_topk=share, band_max_deficit=worst)
            del ws, o
            print(json.dumps(case), file=sys.stderr, flush=True)
            out["cases"].append(case)
        del eng
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
