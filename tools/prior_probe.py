#!/usr/bin/env python3
"""Time what the rank-one prior of retrieval (include/newsrec_prior.h) costs at
the MIND-large dev shape of §3.8 -- 255,990 distinct users x 72,023 news, bf16, K = 10 and
64 -- against the entries without it and against the route a torch user would take, all
interleaved in one process.

    python tools/prior_probe.py [--rounds 5] [--iters 2] [--out profiles/prior/prior_probe.json]
                                [--users 255990] [--news 72023] [--no-torch]
                                [--parent-lib OLD/libnewsrec_hip.so]

User rows are the final pooler's over synthetic histories with the benchmark's lengths.  Per
K, after a warm-up of every route, each round times with device events, in this order:
  topk            ops.topk_users, history excluded
  filtered        ops.topk_users_filtered: a per-user time window that keeps ~60 % of the
                  news and a category mask that keeps half of the categories
  prior           ops.topk_users_prior without a filter: a popularity-like prior in [0, 1],
                  per-user gains in [0, 0.5]
  prior_filtered  ops.topk_users_prior under the filter above
  topk_again      ops.topk_users once more: the spread of a repeated route
  torch           users.bfloat16() @ table.T in blocks of 16,384 users, scaled by cand_inv,
                  + gain[:, None] * prior[None, :], torch.topk -- no exclusion, no filter
and one JSON line holds the medians, every round's time, and |topk - topk_again| of the
medians beside them.  With --parent-lib the same rounds also time nr_topk_users and
nr_topk_users_filtered of that library (a build of the parent commit) on the same buffers, as
parent_topk and parent_filtered, and record whether rows and score bits are equal.  Nothing is
asserted and no ratio is expected: the numbers are reported as measured.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from news_recommendation_project_v2_amd import _lib, ops, synthetic, weights as W  # noqa: E402
from news_recommendation_project_v2_amd.engine import PoolScoreEngine  # noqa: E402
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


def torch_route(users, table, inv, gain, prior, k, block):
    out_i = torch.empty((users.shape[0], k), dtype=torch.int64, device=users.device)
    for u0 in range(0, users.shape[0], block):
        s = (users[u0:u0 + block].bfloat16() @ table.T).float()
        s *= inv[None, :]
        s += gain[u0:u0 + block, None] * prior[None, :]
        out_i[u0:u0 + block] = torch.topk(s, k, dim=1).indices
    return out_i


def parent_entries(path, users, table, inv, eidx, eoff, flt, k, dev):
    """nr_topk_users and nr_topk_users_filtered of another build of the library on the given buffers:
    (plain call, filtered call, their (idx, scores))."""
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in {**_lib.TOPK_SIGNATURES, **_lib.FILTER_SIGNATURES}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    U, N = users.shape[0], table.shape[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(lib.nr_topk_workspace_bytes(_lib.NR_BF16, U, N, k), dtype=torch.uint8, device=dev)
    o = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev))
    head = (_lib.NR_BF16, 1024, U, p(users), N, p(table), table.stride(0), p(inv), p(eidx), p(eoff))
    tail = lambda: (k, p(o[0]), p(o[1]), p(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    fptr = tuple(p(flt[n]) for n in ("news_time", "time_lo", "time_hi", "news_cat", "cat_mask"))

    def plain():
        assert lib.nr_topk_users(*head, *tail()) == 0, lib.nr_last_error()

    def filtered():
        assert lib.nr_topk_users_filtered(*head, *fptr, *tail()) == 0, lib.nr_last_error()
    return plain, filtered, o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--users", type=int, default=255_990)
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--torch-block", type=int, default=16_384)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--parent-lib", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=Path("profiles/prior/prior_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1234)
    U, N = args.users, args.news
    hl = np.clip(rng.geometric(1 / 33.0, U), 1, 600).astype(np.int32)
    hi = rng.integers(0, N, int(hl.sum())).astype(np.int32)
    table = W.news_table(1234, N, 1024, name="topk-probe")
    m = FinalAttention(1024, 4096)
    m.load_state_dict(W.final_attention_state_dict(1234))
    eng = PoolScoreEngine(m.to(dev).eval(), dtype=torch.bfloat16, device=dev)
    eng.load_news(table)
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(U, np.int32), dedupe=False)
    eng.recommend(1)  # transform, norms and the pooled users
    users, tab, inv = eng._users, eng.cand_table, eng.cand_inv
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prior = up(synthetic.catalogue_prior(N, seed=1234))
    gain = up((rng.random(U) * 0.5).astype(np.float32))
    news_time = rng.integers(0, 1000, N).astype(np.int32)
    lo = rng.integers(0, 400, U).astype(np.int32)
    flt = dict(news_time=up(news_time), time_lo=up(lo), time_hi=up(lo + 600),
               news_cat=up(rng.integers(0, 18, N).astype(np.uint8)),
               cat_mask=up(np.full(U, 0b010101010101010101, np.int64)))
    flop = 2.0 * U * N * 1024
    out = {"U": U, "N": N, "dtype": "bf16", "rounds": args.rounds, "iters": args.iters, "gemm_tflop": flop / 1e12,
           "chunk_rows": int(ops._lib.load().nr_topk_chunk_rows()), "cases": []}
    for k in (10, 64):
        ws = torch.empty(ops.topk_users_prior_workspace_bytes(torch.bfloat16, U, N, k), dtype=torch.uint8, device=dev)
        o = tuple(torch.empty((U, k), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32))
        ex = dict(excl_idx=eng.hist_idx, excl_off=eng.hist_off, workspace=ws)
        plain = lambda: ops.topk_users(users, tab, inv, k, out=o[:2], **ex)
        fns = {"topk": plain,
               "filtered": lambda: ops.topk_users_filtered(users, tab, inv, k, out=o[:2], **flt, **ex),
               "prior": lambda: ops.topk_users_prior(users, tab, inv, k, news_prior=prior, user_gain=gain, out=o, **ex),
               "prior_filtered": lambda: ops.topk_users_prior(users, tab, inv, k, news_prior=prior, user_gain=gain,
                                                              out=o, **flt, **ex),
               "topk_again": plain}
        equal = {}
        if args.parent_lib is not None:
            fns["parent_topk"], fns["parent_filtered"], po = parent_entries(args.parent_lib, users, tab, inv, eng.hist_idx,
                                                                             eng.hist_off, flt, k, dev)
            for a in ("topk", "filtered"):
                fns[a]()
                fns["parent_" + a]()
                torch.cuda.synchronize()
                equal[a] = all(torch.equal(x, y) for x, y in zip(o[:2], po))
        if not args.no_torch:
            fns["torch"] = lambda: torch_route(users, tab, inv, gain, prior, k, args.torch_block)
        for fn in fns.values():
            timed(fn, 1)
        res = {n: [] for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                res[n].append(timed(fn, args.iters))
        case = {"K": k, "workspace_bytes": int(ws.numel()),
                "prior_workspace_extra_bytes": int(ws.numel() - ops.topk_workspace_bytes(torch.bfloat16, U, N, k))}
        for n, v in res.items():
            case[n + "_ms"] = round(statistics.median(v), 3)
            case[n + "_ms_all"] = [round(x, 3) for x in v]
        if equal:
            case["equal_to_parent"] = equal
        case["repeat_spread_ms"] = round(abs(case["topk_ms"] - case["topk_again_ms"]), 3)
        case["round_spread_ms"] = round(max(max(v) - min(v) for n, v in res.items() if n != "torch"), 3)
        del ws, o
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
    line = json.dumps(out)
    print(line, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
