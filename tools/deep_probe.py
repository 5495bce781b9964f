#!/usr/bin/env python3
"""Time deep retrieval (include/newsrec_deep.h) at the MIND-large dev shape of
tools/page_probe.py -- 255,990 distinct users x 72,023 news, histories excluded -- against the
paged route it replaces, against one 64-row walk, against the route a torch user would take, and
the 64-row entries against a build of the parent commit, all interleaved in one process.

    python tools/deep_probe.py [--dtype bf16|f32] [--rounds 5] [--iters 1] [--users 255990] [--news 72023]
                               [--no-torch] [--no-engine] [--routes deep256,topk64] [--no-entries]
                               [--parent-lib OLD/libnewsrec_hip.so]
                               [--out profiles/deep/deep_probe_bf16.json]

User rows are the final pooler's over synthetic histories with the benchmark's lengths.  After a
warm-up of every route, each round times with device events, in this order:
  deep{K}       ops.topk_users_deep(K), K = 128 and 256: one walk over the table
  paged{K}      ceil(K / 64) chained ops.topk_users_after calls of 64 rows (what the deep call
                replaces; the two sorts that order the pages as one list are NOT included)
  topk64        ops.topk_users(64): what one walk with the 64-slot heap costs
  torch{K}      users.to(dtype) @ table.T in blocks of 16,384 users, scaled by cand_inv,
                torch.topk(K) -- no exclusion, so it does less
  rec_walk256   PoolScoreEngine.recommend_deep(256, walk=256): transform + norms + pooling + one deep call
  rec_page64    PoolScoreEngine.recommend_deep(256, page=64): the same around four pages and two sorts
  deep256_again ops.topk_users_deep(256) once more: the spread of a repeated route
and, for K = 10 and 64, the entries whose kernels this feature leaves alone:
  topk / filtered / prior / after       ops.topk_users, _filtered, _prior, _after (from a start cursor)
  parent_topk / _filtered / _prior / _after   the same entries of --parent-lib on the same buffers,
                with whether rows and score bits are equal.  The parent's entries are bare C calls;
                this build's go through ops.*, whose host check of the exclusion rows (a min / max
                and a sync) is inside the timed region, except after (excl_checked).
One JSON line holds the medians, every round's time, the largest spread of a route over its
rounds, and the deep workspace.  Nothing is asserted: the numbers are reported as measured.
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


def torch_route(users, table, inv, k, block):
    out_i = torch.empty((users.shape[0], k), dtype=torch.int64, device=users.device)
    for u0 in range(0, users.shape[0], block):
        s = users[u0:u0 + block].to(table.dtype) @ table.T
        s *= inv.to(s.dtype)[None, :]
        out_i[u0:u0 + block] = torch.topk(s, k, dim=1).indices
    return out_i


def parent_entries(path, dt, users, table, inv, eidx, eoff, flt, prior, gain, k, dev):
    """The 64-row entries of another build of the library on the given buffers: {name: call} and
    the (idx, scores, keys) they write."""
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in {**_lib.TOPK_SIGNATURES, **_lib.FILTER_SIGNATURES, **_lib.PRIOR_SIGNATURES,
                              **_lib.PAGE_SIGNATURES}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    U, N = users.shape[0], table.shape[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(lib.nr_topk_users_prior_workspace_bytes(dt, U, N, k), dtype=torch.uint8, device=dev)
    o = tuple(torch.empty((U, k), dtype=d, device=dev) for d in (torch.int32, torch.float32, torch.float32))
    cur, nxt = ops.start_cursor(U, dev), ops.start_cursor(U, dev)
    head = (dt, 1024, U, p(users), N, p(table), table.stride(0), p(inv), p(eidx), p(eoff))
    tail = lambda *keys: (k, p(o[0]), p(o[1]), *keys, p(ws), ws.numel(),
                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    fptr = tuple(p(flt[n]) for n in ("news_time", "time_lo", "time_hi", "news_cat", "cat_mask"))
    ok = lambda rc: rc == 0 or sys.exit(lib.nr_last_error().decode())
    return {"topk": lambda: ok(lib.nr_topk_users(*head, *tail())),
            "filtered": lambda: ok(lib.nr_topk_users_filtered(*head, *fptr, *tail())),
            "prior": lambda: ok(lib.nr_topk_users_prior(*head, *(None,) * 5, p(prior), p(gain), *tail(p(o[2])))),
            "after": lambda: ok(lib.nr_topk_users_after(*head, *(None,) * 7, p(cur[0]), p(cur[1]), p(nxt[0]), p(nxt[1]),
                                                        *tail(p(o[2]))))}, o, (ws, cur, nxt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--users", type=int, default=255_990)
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--torch-block", type=int, default=16_384)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--routes", default=None, metavar="A,B", help="time only these routes of the first list")
    ap.add_argument("--no-entries", action="store_true", help="skip the 64-row entries")
    ap.add_argument("--parent-lib", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    dt = _lib.NR_BF16 if args.dtype == "bf16" else _lib.NR_F32
    rng = np.random.default_rng(1234)
    U, N = args.users, args.news
    hl = np.clip(rng.geometric(1 / 33.0, U), 1, 600).astype(np.int32)
    hi = rng.integers(0, N, int(hl.sum())).astype(np.int32)
    m = FinalAttention(1024, 4096)
    m.load_state_dict(W.final_attention_state_dict(1234))
    eng = PoolScoreEngine(m.to(dev).eval(), dtype=dtype, device=dev)
    eng.load_news(W.news_table(1234, N, 1024, name="topk-probe"))
    eng.load_impressions(hi, hl, np.zeros(0, np.int32), np.zeros(U, np.int32), dedupe=False)
    eng.recommend(1)  # transform, norms and the pooled users
    users, tab, inv = eng._users, eng.cand_table, eng.cand_inv
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prior = up(synthetic.catalogue_prior(N, seed=1234))
    gain = up((rng.random(U) * 0.5).astype(np.float32))
    lo = rng.integers(0, 400, U).astype(np.int32)
    flt = dict(news_time=up(rng.integers(0, 1000, N).astype(np.int32)), time_lo=up(lo), time_hi=up(lo + 600),
               news_cat=up(rng.integers(0, 18, N).astype(np.uint8)),
               cat_mask=up(np.full(U, 0b010101010101010101, np.int64)))
    ws_bytes = ops.topk_users_deep_workspace_bytes(dtype, U, N, 256)
    out = {"U": U, "N": N, "dtype": args.dtype, "rounds": args.rounds, "iters": args.iters,
           "gemm_tflop": 2.0 * U * N * 1024 / 1e12, "deep_workspace_bytes": int(ws_bytes),
           "deep_workspace_bytes_per_user": round(ws_bytes / U, 1)}

    def measure(fns):
        for fn in fns.values():
            timed(fn, 1)
        res = {n: [] for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                res[n].append(timed(fn, args.iters))
        case = {}
        for n, v in res.items():
            case[n + "_ms"] = round(statistics.median(v), 3)
            case[n + "_ms_all"] = [round(x, 3) for x in v]
        case["round_spread_ms"] = round(max(max(v) - min(v) for v in res.values()), 3)
        return case

    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    ex = dict(excl_idx=eng.hist_idx, excl_off=eng.hist_off, workspace=ws, excl_checked=True)
    outs = {k: tuple(torch.empty((U, k), dtype=d, device=dev) for d in (torch.int32, torch.float32, torch.float32))
            for k in (64, 128, 256)}
    cur = ops.start_cursor(U, dev)

    def deep(k):
        return lambda: ops.topk_users_deep(users, tab, inv, k, out=outs[k], next_out=cur, **ex)

    def paged(k):
        def run():
            c = ops.start_cursor(U, dev)
            for _ in range(k // 64):
                ops.topk_users_after(users, tab, inv, 64, after=c, next_out=c, out=outs[64], **ex)
        return run

    fns = {}
    for k in (128, 256):
        fns[f"deep{k}"], fns[f"paged{k}"] = deep(k), paged(k)
    fns["topk64"] = lambda: ops.topk_users(users, tab, inv, 64, out=outs[64][:2], excl_idx=eng.hist_idx,
                                           excl_off=eng.hist_off, workspace=ws)
    if not args.no_torch:
        for k in (128, 256):
            fns[f"torch{k}"] = (lambda k: lambda: torch_route(users, tab, inv, k, args.torch_block))(k)
    if not args.no_engine:
        fns["rec_walk256"] = lambda: eng.recommend_deep(256, walk=256)
        fns["rec_page64"] = lambda: eng.recommend_deep(256, page=64)
    fns["deep256_again"] = deep(256)
    if args.routes is not None:
        fns = {n: fns[n] for n in args.routes.split(",")}
    out["deep"] = measure(fns)
    if "deep256" in fns and "deep256_again" in fns:
        out["deep"]["repeat_spread_ms"] = round(abs(out["deep"]["deep256_ms"] - out["deep"]["deep256_again_ms"]), 3)
    print(json.dumps(out["deep"]), file=sys.stderr, flush=True)

    out["entries"] = []
    for k in () if args.no_entries else (10, 64):
        o = tuple(torch.empty((U, k), dtype=d, device=dev) for d in (torch.int32, torch.float32, torch.float32))
        e2 = dict(excl_idx=eng.hist_idx, excl_off=eng.hist_off, workspace=ws)
        pri = dict(news_prior=prior, user_gain=gain)
        start, nxt = ops.start_cursor(U, dev), ops.start_cursor(U, dev)
        fns = {"topk": lambda: ops.topk_users(users, tab, inv, k, out=o[:2], **e2),
               "filtered": lambda: ops.topk_users_filtered(users, tab, inv, k, out=o[:2], **flt, **e2),
               "prior": lambda: ops.topk_users_prior(users, tab, inv, k, out=o, **pri, **e2),
               "after": lambda: ops.topk_users_after(users, tab, inv, k, after=start, next_out=nxt, out=o,
                                                     excl_checked=True, **e2)}
        equal = {}
        if args.parent_lib is not None:
            old, po, keep = parent_entries(args.parent_lib, dt, users, tab, inv, eng.hist_idx, eng.hist_off, flt, prior,
                                           gain, k, dev)
            for a, fn in old.items():
                fns[a]()
                fn()
                torch.cuda.synchronize()
                equal[a] = all(torch.equal(x, y) for x, y in zip(o[:3 if a in ("prior", "after") else 2], po))
            fns.update({"parent_" + a: fn for a, fn in old.items()})
        case = {"K": k, **measure(fns)}
        if equal:
            case["equal_to_parent"] = equal
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["entries"].append(case)
    line = json.dumps(out)
    print(line, flush=True)
    path = args.out or Path(f"profiles/deep/deep_probe_{args.dtype}.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")


if __name__ == "__main__":
    main()
