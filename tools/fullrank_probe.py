#!/usr/bin/env python3
"""Time the full-table ranks of clicked news at the MIND-large dev shape --
255,990 distinct users x 72,023 news, bf16, histories excluded, the benchmark's clicked
candidates as targets -- against top-K retrieval over the same product and against the
route a torch user would take, interleaved in one process.

    python tools/fullrank_probe.py [--pooler final] [--rounds 3] [--iters 2] [--out FILE.json]
                                   [--impressions 376471] [--users 255990] [--news 72023] [--no-torch]

The impressions are synthetic.mind_impressions(users=...) (a user's history repeats on each
of the user's impressions; clicks = label 1), loaded with the histories deduplicated, so the
targets of an impression are grouped under its distinct user.  Each round times with device
events, after a warm-up of every route:
  engine      PoolScoreEngine.rank_targets (transform + norms + pooling + grouping + ranks)
  rank        ops.rank_targets alone (bf16 pre-pass, thresholds, counting pass)
  topk1/10    ops.topk_users alone at K = 1 and K = 10: the same product with the heap epilogue
  torch       users.bfloat16() @ table.T in user blocks that fit memory, scaled by cand_inv,
              then per target a compare-and-sum over its user's row -- no exclusion, so it
              does less
and prints one JSON line with the medians: ms per pass, executed TFLOP/s of the
2 U N 1024 product, workspace bytes, and the retrieval metrics of the ranks (random
weights on a random table: chance level, they only show the plumbing).  The kernel split
(pre-pass / thresholds / count) comes from a kernel trace of a run of its own.
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

from news_recommendation_project_v2_amd import ops, synthetic, weights as W  # noqa: E402
from news_recommendation_project_v2_amd.data_utils import lengths_to_offsets  # noqa: E402
from news_recommendation_project_v2_amd.engine import PoolScoreEngine  # noqa: E402
from news_recommendation_project_v2_amd.evaluation import retrieval_metrics  # noqa: E402
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


def torch_route(users, table, inv, tgt, toff_host, block):
    """Ranks by the torch route: a bf16 score block per user block, then per target the
    number of rows of its user's scores that beat it (ties by row).  No exclusion."""
    out = torch.empty(tgt.numel(), dtype=torch.int32, device=users.device)
    cols = torch.arange(table.shape[0], device=users.device)[None, :]
    U = users.shape[0]
    for u0 in range(0, U, block):
        u1 = min(u0 + block, U)
        a, b = int(toff_host[u0]), int(toff_host[u1])
        if a == b:
            continue
        s = users[u0:u1].bfloat16() @ table.T
        s *= inv.to(s.dtype)[None, :]
        lens = torch.as_tensor(np.diff(toff_host[u0:u1 + 1]), device=users.device)
        owner = torch.repeat_interleave(torch.arange(u1 - u0, device=users.device), lens)
        t = tgt[a:b].long()
        for j0 in range(0, b - a, 8192):  # 8,192 targets' rows at a time (1.2 GB)
            rows = s[owner[j0:j0 + 8192]]
            tj = t[j0:j0 + 8192, None]
            thr = torch.gather(rows, 1, tj)
            out[a + j0:a + j0 + rows.shape[0]] = ((rows > thr) | ((rows == thr) & (cols < tj))).sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--impressions", type=int, default=synthetic.SHAPES["mind_large_dev"][1])
    ap.add_argument("--users", type=int, default=synthetic.MIND_LARGE_DEV_USERS)
    ap.add_argument("--news", type=int, default=synthetic.SHAPES["mind_large_dev"][0])
    ap.add_argument("--torch-block", type=int, default=16_384)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--pooler", choices=["final", "latent", "both"], default="final")
    ap.add_argument("--only", default=None, help="run one route once, untimed (for a kernel trace): rank, topk1 or topk10")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = args.news
    imps = synthetic.mind_impressions(N, args.impressions, seed=1234, users=args.users)
    clicked = imps.labels.astype(bool)
    tgt = imps.cand_idx[clicked]
    tlen = np.add.reduceat(clicked.astype(np.int64), imps.cand_off()[:-1])
    table = W.news_table(1234, N, 1024, name="fullrank-probe")
    out = {"impressions": imps.n_imp, "N": N, "dtype": "bf16", "rounds": args.rounds, "iters": args.iters,
           "targets": int(len(tgt)), "hist_rows_per_impression": round(imps.n_hist / imps.n_imp, 2), "cases": []}
    for pooler in (["final", "latent"] if args.pooler == "both" else [args.pooler]):
        if pooler == "final":
            m = FinalAttention(1024, 4096)
            m.load_state_dict(W.final_attention_state_dict(1234))
        else:
            m = LatentAttentionModel()
            m.load_state_dict(W.latent_attention_state_dict(1234, ln_random=True))
        eng = PoolScoreEngine(m.to(dev).eval(), dtype=torch.bfloat16, device=dev)
        eng.load_news(table)
        eng.load_impressions(imps.hist_idx, imps.hist_len, np.zeros(0, np.int32), np.zeros(imps.n_imp, np.int32),
                             dedupe=True)
        ranks_eng = eng.rank_targets(tgt, tlen)  # transform, norms and the pooled users
        users, tab, inv = eng._users, eng.cand_table, eng.cand_inv
        U = users.shape[0]
        flop = 2.0 * U * N * 1024
        # the targets under their distinct user, as the engine groups them
        owner = np.repeat(eng.user_idx.cpu().numpy().astype(np.int64), tlen)
        order = np.argsort(owner, kind="stable")
        toff_host = lengths_to_offsets(np.bincount(owner, minlength=U))
        tidx_d = torch.from_numpy(tgt[order]).to(dev)
        toff_d = torch.from_numpy(toff_host).to(dev)
        T = int(tidx_d.numel())
        ws = torch.empty(ops.rank_targets_workspace_bytes(torch.bfloat16, U, N, T), dtype=torch.uint8, device=dev)
        r_out = torch.empty(T, dtype=torch.int32, device=dev)
        fns = {"engine": lambda: eng.rank_targets(tgt, tlen),
               "rank": lambda: ops.rank_targets(users, tab, inv, tidx_d, toff_d, eng.uhist_idx, eng.uhist_off,
                                                out=r_out, workspace=ws)}
        for k in (1, 10):
            kws = torch.empty(ops.topk_workspace_bytes(torch.bfloat16, U, N, k), dtype=torch.uint8, device=dev)
            o = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev))
            fns[f"topk{k}"] = (lambda k=k, o=o, kws=kws: ops.topk_users(users, tab, inv, k, eng.uhist_idx,
                                                                          eng.uhist_off, out=o, workspace=kws))
        if args.only:
            fns[args.only]()
            fns[args.only]()
            torch.cuda.synchronize()
            print(json.dumps({"only": args.only, "U": U, "N": N, "targets": T}), flush=True)
            return
        if not args.no_torch:
            fns["torch"] = lambda: torch_route(users, tab, inv, tidx_d, toff_host, args.torch_block)
        for fn in fns.values():
            timed(fn, 1)
        res = {n: [] for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                res[n].append(timed(fn, args.iters))
        case = {"pooler": pooler, "U": U, "targets": T, "targets_per_user_max": int(np.diff(toff_host).max()),
                "gemm_tflop": round(flop / 1e12, 2), "workspace_bytes": int(ws.numel())}
        for n, v in res.items():
            ms = statistics.median(v)
            case[n + "_ms"] = round(ms, 3)
            case[n + "_ms_all"] = [round(x, 3) for x in v]
            case[n + "_tflops"] = round(flop / ms / 1e9, 1)
        # the routes agree: engine order vs grouped order, and the K = 1 / 10 sets of top-K
        r_host = r_out.cpu().numpy()
        back = np.empty_like(r_host)
        back[order] = r_host
        case["engine_equals_ops"] = bool(np.array_equal(back, ranks_eng.cpu().numpy()))
        top10 = ops.topk_users(users, tab, inv, 10, eng.uhist_idx, eng.uhist_off)[0]
        own = torch.from_numpy(owner[order]).to(dev)
        in_top = (top10[own] == tidx_d[:, None]).any(1)
        case["rank_lt_10_equals_top10_membership"] = bool(torch.equal(in_top, (r_out >= 0) & (r_out < 10)))
        if not args.no_torch:
            rt = fns["torch"]()
            ok = r_out >= 0  # the torch route excludes nothing: compare where no history row can lie before the target
            case["torch_rank_minus_rank_max"] = int((rt[ok] - r_out[ok]).max())
            case["torch_rank_minus_rank_min"] = int((rt[ok] - r_out[ok]).min())
        case["metrics"] = retrieval_metrics(back, tlen, ks=(1, 10, 64, 100, 1000))
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
        del eng, ws, fns
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
