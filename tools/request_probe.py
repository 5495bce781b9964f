#!/usr/bin/env python3
"""Time the request path of retrieval on one MI355X: N = 72,023 news, U in
{1, 8, 32} readers with MIND-like histories (excluded), K in {10, 64}, bf16 and f32.

    python tools/request_probe.py [--news 72023] [--rounds 5] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- \\
        python tools/request_probe.py --trace-run [--trace-calls 7]
    python tools/request_probe.py --merge-trace DIR/.../trace_kernel_trace.csv --out FILE.json

Routes, interleaved in one process, medians over --rounds rounds after a warm-up of each:
  request  ops.topk_request
  bulk     ops.topk_users_after with the same arguments and buffers: the route a request had
           to take before, the baseline
  torch    users (rounded to the table's dtype) @ table.T, scaled, the excluded rows set to
           -inf, torch.topk
Every route holds its outputs, cursor and workspace across calls and skips the host-side range
check of the exclusion lists, so no call waits for the device.  Per route and round two
figures: ``stream_us``, the per-call time of a few hundred back-to-back calls between two
events on one stream (as many calls as fill about --window seconds), and ``wall_us``, the
median host time of single calls from the Python call to the end of a device synchronise.
``spread`` is (max - min) / median over the rounds.  ``engine_us`` is
PoolScoreEngine.recommend_request end to end: from Python lists in to Python lists out.

--trace-run only runs ops.topk_request --trace-calls times per configuration, in the order
(dtype, U, K) of the main run, for a kernel trace taken in a run of its own; --merge-trace
reads that trace, takes the medians of request_stage1_kernel per configuration and writes them
next to the table-read bound (N x 1024 x the dtype's bytes at 8 TB/s) into the record.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from news_recommendation_project_v2_amd import ops  # noqa: E402

DTYPES = (("bf16", torch.bfloat16), ("f32", torch.float32))
US, KS = (1, 8, 32), (10, 64)
HBM_BYTES_PER_S = 8e12


def histories(rng, n_users, n_news):
    """MIND-like history lengths: log-normal around 20 clicks, 1 .. 400."""
    lens = np.clip(np.round(rng.lognormal(3.0, 0.9, n_users)), 1, 400).astype(np.int64)
    return [rng.integers(0, n_news, n).astype(np.int32) for n in lens]


def stream_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def wall_time(fn, calls):
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def summary(v):
    med = statistics.median(v)
    return {"median": round(med, 2), "spread": round((max(v) - min(v)) / med, 4), "all": [round(x, 2) for x in v]}


def configurations(n_news, dev):
    """(dtype name, U, K, the three routes, their outputs) in the order every mode runs them."""
    for name, dtype in DTYPES:
        gen = torch.Generator(device=dev).manual_seed(1234)
        table = torch.randn((n_news, 1024), generator=gen, device=dev).to(dtype)
        inv = ops.row_inv_norm(table, 1e-8)
        scale = inv.to(dtype)
        for U in US:
            rng = np.random.default_rng(100 + U)
            users = torch.randn((U, 1024), generator=gen, device=dev)
            hist = histories(rng, U, n_news)
            eoff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int64)).to(dev)
            eidx = torch.from_numpy(np.concatenate(hist)).to(dev)
            owner = torch.repeat_interleave(torch.arange(U, device=dev), eoff[1:] - eoff[:-1])
            for K in KS:
                bufs = {}
                for route, size in (("request", ops.topk_request_workspace_bytes),
                                    ("bulk", ops.topk_users_after_workspace_bytes)):
                    bufs[route] = dict(
                        out=tuple(torch.empty((U, K), dtype=dt, device=dev)
                                  for dt in (torch.int32, torch.float32, torch.float32)),
                        next_out=(torch.empty(U, dtype=torch.float32, device=dev),
                                  torch.empty(U, dtype=torch.int32, device=dev)),
                        workspace=torch.empty(size(dtype, U, n_news, K), dtype=torch.uint8, device=dev))
                common = dict(excl_idx=eidx, excl_off=eoff, excl_checked=True)
                dense = {}

                def torch_route(users=users, K=K, dense=dense):
                    s = users.to(dtype) @ table.T
                    s *= scale[None, :]
                    s[owner, eidx.long()] = float("-inf")
                    dense["top"] = torch.topk(s.float(), K, dim=1)

                fns = {"request": lambda users=users, K=K, b=bufs["request"]: ops.topk_request(users, table, inv, K, **common, **b),
                       "bulk": lambda users=users, K=K, b=bufs["bulk"]: ops.topk_users_after(users, table, inv, K, **common, **b),
                       "torch": torch_route}
                yield name, U, K, fns, bufs, hist
        del table, inv, scale
        torch.cuda.empty_cache()


def engine_cases(n_news, rounds, dev):
    """recommend_request end to end, Python lists in to Python lists out."""
    from news_recommendation_project_v2_amd import weights as W
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    from news_recommendation_project_v2_amd.latent_attention import LatentAttentionModel
    model = LatentAttentionModel()
    model.load_state_dict(W.latent_attention_state_dict(5, ln_random=True))
    model = model.to(dev).eval()
    out = []
    for name, dtype in DTYPES:
        eng = PoolScoreEngine(model, dtype=dtype, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1234)
        eng.load_news(torch.randn((n_news, 1024), generator=gen, device=dev))
        t0 = time.perf_counter()
        eng.prepare_requests()
        torch.cuda.synchronize()
        prepare_ms = (time.perf_counter() - t0) * 1e3
        for U in US:
            hist = [h.tolist() for h in histories(np.random.default_rng(100 + U), U, n_news)]
            for K in KS:
                def call():
                    idx, scores = eng.recommend_request([np.asarray(h, dtype=np.int32) for h in hist], K)
                    return idx.tolist(), scores.tolist()
                call()
                v = [wall_time(call, 10) for _ in range(rounds)]
                out.append({"dtype": name, "U": U, "K": K, "engine_us": summary(v),
                            "prepare_requests_ms": round(prepare_ms, 2)})
                print(json.dumps(out[-1]), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    return out


def merge_trace(path, n_news, calls):
    """Medians of request_stage1_kernel per configuration from a kernel trace of --trace-run."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "request_stage1_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    order = [(name, U, K) for name, _ in DTYPES for U in US for K in KS]
    if len(us) != calls * len(order):
        raise SystemExit(f"{path}: {len(us)} stage-1 dispatches, expected {calls} x {len(order)}")
    out = []
    for i, (name, U, K) in enumerate(order):
        v = us[calls * i + 2:calls * (i + 1)]  # (the first two calls of a configuration warm up)
        bound = n_news * 1024 * (2 if name == "bf16" else 4) / HBM_BYTES_PER_S * 1e6
        out.append({"dtype": name, "U": U, "K": K, "stage1_us": summary(v), "table_read_bound_us": round(bound, 2),
                    "stage1_over_bound": round(statistics.median(v) / bound, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of back-to-back calls per route and round")
    ap.add_argument("--wall-calls", type=int, default=15)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-calls", type=int, default=7)
    ap.add_argument("--merge-trace", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.merge_trace is not None:
        rec = json.loads(args.out.read_text()) if args.out and args.out.is_file() else {"N": args.news}
        rec["stage1_trace"] = merge_trace(args.merge_trace, rec.get("N", args.news), args.trace_calls)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            args.out.write_text(line + "\n")
        return
    dev = torch.device("cuda:0")
    if args.trace_run:
        for name, U, K, fns, _, _ in configurations(args.news, dev):
            for _ in range(args.trace_calls):
                fns["request"]()
            torch.cuda.synchronize()
        return
    rec = {"N": args.news, "rounds": args.rounds, "window_s": args.window, "wall_calls": args.wall_calls,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for name, U, K, fns, bufs, hist in configurations(args.news, dev):
        iters = {}
        for n, fn in fns.items():  # warm up, then as many calls as fill the window (10 .. 400)
            fn()
            iters[n] = int(min(400, max(10, args.window * 1e6 / stream_time(fn, 3))))
        same = lambda a, b: torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                        b.view(torch.int32) if b.dtype == torch.float32 else b)
        case = {"dtype": name, "U": U, "K": K, "excluded_rows": int(sum(len(h) for h in hist)), "iters": iters,
                "request_equals_bulk": all(same(a, b) for r in ("out", "next_out")
                                           for a, b in zip(bufs["request"][r], bufs["bulk"][r]))}
        res = {n: {"stream_us": [], "wall_us": []} for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                res[n]["stream_us"].append(stream_time(fn, iters[n]))
            for n, fn in fns.items():
                res[n]["wall_us"].append(wall_time(fn, args.wall_calls))
        for n in fns:
            case[n] = {m: summary(v) for m, v in res[n].items()}
        for m in ("stream_us", "wall_us"):
            rq, bk = case["request"][m], case["bulk"][m]
            case[f"bulk_over_request_{m}"] = round(bk["median"] / rq["median"], 2)
            # the condition: faster by more than either route's spread over its rounds
            case[f"request_wins_{m}"] = bool(bk["median"] - rq["median"]
                                             > max(rq["spread"] * rq["median"], bk["spread"] * bk["median"]))
            case[f"torch_over_request_{m}"] = round(case["torch"][m]["median"] / rq["median"], 2)
        print(json.dumps(case), file=sys.stderr, flush=True)
        rec["cases"].append(case)
    if not args.no_engine:
        rec["engine"] = engine_cases(args.news, args.rounds, dev)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
