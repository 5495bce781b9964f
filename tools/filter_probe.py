#!/usr/bin/env python3
"""Time the catalogue filters of retrieval and ranks at the MIND-large dev
shape -- 255,990 users x 72,023 news, bf16, K = 10 and 64 -- interleaved in one process.

    python tools/filter_probe.py [--users 255990] [--news 72023] [--rounds 3] [--iters 2]
                                 [--route-users 8192] [--parent-lib OLD/libnewsrec_hip.so]
                                 [--no-torch] [--out FILE.json]

Users and table are seeded normal rows (the scan's work depends on how often a score beats
the running K-th best, which random rows exercise as pooled users do).  Per K, each round
times with device events, after a warm-up of every shape:

  unfiltered       ops.topk_users / ops.rank_targets (one target per user), no exclusions
  parent           the same two entries of the library given with --parent-lib (a build of
                   an earlier commit), called through ctypes on the same buffers: the
                   unfiltered instantiation must not have changed.  Where that library has
                   the filtered entries, parent_allpass times them too, and parent_equal
                   records whether both builds return the same idx, scores and ranks, bit
                   for bit, for the unfiltered, all-pass and f10.s cases
  allpass          the filtered entries with a window and a mask that pass every row: the
                   cost of the predicate itself
  f50 / f10 / f1   a window that leaves 50 % / 10 % / 1 % of the table eligible, the eligible
                   rows contiguous in the table (.c) or scattered over it (.s)
  torch            users.bfloat16() @ table.T in user blocks, masked_fill, torch.topk
and, on the first --route-users users only (the lists of all users would not fit memory):
  route            ops.topk_users with the ineligible rows as exclusion lists, against
  filtered_sub     the filtered entry on the same users.
Prints one JSON line with the medians in ms.
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

from news_recommendation_project_v2_amd import _lib, ops  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_route(users, table, inv, elig, k, block):
    out_i = torch.empty((users.shape[0], k), dtype=torch.int64, device=users.device)
    for u0 in range(0, users.shape[0], block):
        s = users[u0:u0 + block].bfloat16() @ table.T
        s *= inv.to(s.dtype)[None, :]
        s.masked_fill_(~elig[None, :], float("-inf"))
        out_i[u0:u0 + block] = torch.topk(s, k, dim=1).indices
    return out_i


def parent_entries(path, users, table, inv, k, tgt, toff, dev):
    """The parent library's entries on the given buffers: topk(flt) and rank(flt) return closures
    over nr_topk_users / nr_rank_targets (flt None) or their _filtered forms (flt = the five
    filter tensors in the C order); ``filtered`` tells whether that library has the latter."""
    lib = ctypes.CDLL(str(path))
    filtered = hasattr(lib, "nr_topk_users_filtered")
    for name, (res, args) in {**_lib.TOPK_SIGNATURES, **_lib.FULLRANK_SIGNATURES,
                              **(_lib.FILTER_SIGNATURES if filtered else {})}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    U, N = users.shape[0], table.shape[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(max(lib.nr_topk_workspace_bytes(_lib.NR_BF16, U, N, k),
                         lib.nr_rank_targets_workspace_bytes(_lib.NR_BF16, U, N, U)), dtype=torch.uint8, device=dev)
    oi = torch.empty((U, k), dtype=torch.int32, device=dev)
    os_ = torch.empty((U, k), dtype=torch.float32, device=dev)
    rk = torch.empty(U, dtype=torch.int32, device=dev)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (_lib.NR_BF16, 1024, U, p(users), N, p(table), table.stride(0), p(inv), None, None)

    def entry(name, flt, *tail):
        fn = getattr(lib, name if flt is None else name + "_filtered")
        fptr = () if flt is None else tuple(p(t) for t in flt)

        def call():
            rc = fn(*head, *fptr, *tail, p(ws), ws.numel(), st())
            assert rc == 0, lib.nr_last_error()
        return call

    topk = lambda flt=None: entry("nr_topk_users", flt, k, p(oi), p(os_))
    rank = lambda flt=None: entry("nr_rank_targets", flt, U, p(tgt), p(toff), p(rk))
    return topk, rank, (oi, os_, rk), filtered


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=255_990)
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--route-users", type=int, default=8192)
    ap.add_argument("--torch-block", type=int, default=16_384)
    ap.add_argument("--parent-lib", type=Path, default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    U, N = args.users, args.news
    gen = torch.Generator(device=dev).manual_seed(1234)
    table = torch.randn((N, 1024), generator=gen, device=dev).to(torch.bfloat16)
    users = torch.randn((U, 1024), generator=gen, device=dev)
    inv = ops.row_inv_norm(table, 1e-8)
    tgt = torch.randint(0, N, (U,), generator=gen, device=dev, dtype=torch.int32)
    toff = torch.arange(U + 1, dtype=torch.int64, device=dev)
    i32 = torch.iinfo(torch.int32)
    cat = torch.zeros(N, dtype=torch.uint8, device=dev)
    every = torch.full((U,), -1, dtype=torch.int64, device=dev)
    order = {"c": torch.arange(N, dtype=torch.int32, device=dev),
             "s": torch.randperm(N, generator=gen, device=dev).to(torch.int32)}
    Us = min(args.route_users, U)
    out = {"U": U, "N": N, "dtype": "bf16", "rounds": args.rounds, "iters": args.iters, "route_users": Us, "cases": []}
    for k in (10, 64):
        ws = torch.empty(ops.topk_workspace_bytes(torch.bfloat16, U, N, k), dtype=torch.uint8, device=dev)
        rws = torch.empty(ops.rank_targets_workspace_bytes(torch.bfloat16, U, N, U), dtype=torch.uint8, device=dev)
        o = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev))
        ro = torch.empty(U, dtype=torch.int32, device=dev)

        def window(lo, hi, n=U):
            return (torch.full((n,), lo, dtype=torch.int32, device=dev), torch.full((n,), hi, dtype=torch.int32, device=dev))

        def filtered(news_time, lo, hi, n=U):
            a, b = window(lo, hi, n)
            return lambda: ops.topk_users_filtered(users[:n], table, inv, k, news_time=news_time, time_lo=a, time_hi=b,
                                                   news_cat=cat, cat_mask=every[:n], out=(o[0][:n], o[1][:n]),
                                                   workspace=ws)

        a_lo, a_hi = window(i32.min, i32.max)
        fns = {"unfiltered_topk": lambda: ops.topk_users(users, table, inv, k, out=o, workspace=ws),
               "unfiltered_rank": lambda: ops.rank_targets(users, table, inv, tgt, toff, out=ro, workspace=rws),
               "allpass_topk": filtered(order["c"], i32.min, i32.max),
               "allpass_rank": lambda: ops.rank_targets_filtered(users, table, inv, tgt, toff, news_time=order["c"],
                                                                 time_lo=a_lo, time_hi=a_hi, news_cat=cat, cat_mask=every,
                                                                 out=ro, workspace=rws)}
        allpass = (order["c"], a_lo, a_hi, cat, every)
        parent = None
        if args.parent_lib is not None:
            parent = parent_entries(args.parent_lib, users, table, inv, k, tgt, toff, dev)
            fns["parent_topk"], fns["parent_rank"] = parent[0](), parent[1]()
            if parent[3]:
                fns["parent_allpass_topk"], fns["parent_allpass_rank"] = parent[0](allpass), parent[1](allpass)
        once = {}
        for frac, tag in ((0.5, "f50"), (0.1, "f10"), (0.01, "f1")):
            n_ok = max(1, int(round(frac * N)))
            for how in ("c", "s"):
                fns[f"{tag}.{how}_topk"] = filtered(order[how], 0, n_ok - 1)
                elig = order[how] < n_ok
                # the exclusion-CSR route, on the first Us users: every user's list = the ineligible rows
                bad = torch.nonzero(~elig).reshape(-1).to(torch.int32)
                eidx = bad.repeat(Us)
                eoff = torch.arange(Us + 1, dtype=torch.int64, device=dev) * bad.numel()
                once[f"{tag}.{how}_route_sub"] = (lambda eidx=eidx, eoff=eoff: ops.topk_users(
                    users[:Us], table, inv, k, excl_idx=eidx, excl_off=eoff, out=(o[0][:Us], o[1][:Us]), workspace=ws))
                once[f"{tag}.{how}_filtered_sub"] = filtered(order[how], 0, n_ok - 1, Us)
                if not args.no_torch:
                    once[f"{tag}.{how}_torch"] = (lambda elig=elig: torch_route(users, table, inv, elig, k,
                                                                                 args.torch_block))
        for fn in fns.values():
            timed(fn, 1)
        res = {n: [] for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                res[n].append(timed(fn, args.iters))
        case = {"K": k}
        for n, v in res.items():
            case[n + "_ms"] = round(statistics.median(v), 3)
            case[n + "_ms_all"] = [round(x, 3) for x in v]
        for n, fn in once.items():  # the slow baselines: one warm-up, then the median of `rounds` single passes
            timed(fn, 1)
            case[n + "_ms"] = round(statistics.median(timed(fn, 1) for _ in range(args.rounds)), 3)
        if parent is not None and parent[3]:  # both builds on one filter: the same bits
            def same(flt):
                names = ("news_time", "time_lo", "time_hi", "news_cat", "cat_mask")
                kw = {} if flt is None else dict(zip(names, flt))
                (ops.topk_users if flt is None else ops.topk_users_filtered)(users, table, inv, k, out=o, workspace=ws, **kw)
                (ops.rank_targets if flt is None else ops.rank_targets_filtered)(users, table, inv, tgt, toff, out=ro,
                                                                                 workspace=rws, **kw)
                parent[0](flt)()
                parent[1](flt)()
                torch.cuda.synchronize()
                return all(torch.equal(x, y) for x, y in zip((*o, ro), parent[2]))

            f10s = (order["s"], *window(0, max(1, int(round(0.1 * N))) - 1), cat, every)
            case["parent_equal"] = {"unfiltered": same(None), "allpass": same(allpass), "f10.s": same(f10s)}
            case["over_parent"] = {n: round(case[n + "_ms"] / case[f"parent_{n.replace('unfiltered_', '')}_ms"], 4)
                                   for n in ("unfiltered_topk", "unfiltered_rank", "allpass_topk", "allpass_rank")}
        case["allpass_over_unfiltered_topk"] = round(case["allpass_topk_ms"] / case["unfiltered_topk_ms"], 4)
        case["allpass_over_unfiltered_rank"] = round(case["allpass_rank_ms"] / case["unfiltered_rank_ms"], 4)
        case["f1.c_over_1pct_of_unfiltered"] = round(case["f1.c_topk_ms"] / (0.01 * case["unfiltered_topk_ms"]), 2)
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
        del ws, rws, o, ro, parent, fns, once
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
