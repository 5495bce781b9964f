#!/usr/bin/env python3
"""Time cursors for top-K retrieval (include/newsrec_page.h) at the MIND-large
dev shape of §3.8 -- 255,990 distinct users x 72,023 news, bf16, histories excluded -- against
the entries without a cursor, against a build of the parent commit, and against the route a
torch user would take, all interleaved in one process.

    python tools/page_probe.py [--rounds 5] [--iters 2] [--out profiles/page/page_probe.json]
                               [--users 255990] [--news 72023] [--no-torch] [--no-deep]
                               [--parent-lib OLD/libnewsrec_hip.so [--parent-first]]

User rows are the final pooler's over synthetic histories with the benchmark's lengths.  Per
K in (10, 64), after a warm-up of every route, each round times with device events, in this
order:
  topk        ops.topk_users, history excluded
  filtered    ops.topk_users_filtered: a per-user time window that keeps ~60 % of the news and a
              category mask that keeps half of the categories
  prior       ops.topk_users_prior without a filter: a popularity-like prior in [0, 1], per-user
              gains in [0, 0.5]
  after_p1    ops.topk_users_after without a cursor, the next cursor wanted: page 1
  after_p2    ops.topk_users_after from the cursor behind page 1: page 2
  after_p2_prior   the same under the prior
  topk_again  ops.topk_users once more: the spread of a repeated route
With --parent-lib the same rounds also time nr_topk_users, nr_topk_users_filtered and
nr_topk_users_prior of that library (a build of the parent commit) on the same buffers, as
parent_topk, parent_filtered and parent_prior, and record whether rows and score bits are equal;
they run at the end of a round, or with --parent-first at its start (a route's time depends a
little on what ran before it: the two orders bound that effect).  The parent's entries are bare C
calls; this build's go through ops.*, whose host check of the exclusion rows (a min / max and a
sync) is inside the timed region, except after_* (excl_checked).
Then, once (not per K):
  deep256_pages    four chained cursor calls of 64 rows and the two stable sorts that order the
                   256 (ops level: what recommend_deep adds to the engine's fixed work)
  recommend_deep   PoolScoreEngine.recommend_deep(256, page=64): transform + norms + pooling +
                   the above
  torch256         users.bfloat16() @ table.T in blocks of 16,384 users, scaled by cand_inv,
                   torch.topk(256) -- no exclusion, so it does less
One JSON line holds the medians and every round's time.  Nothing is asserted and no ratio is
expected: the numbers are reported as measured.
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
        s = users[u0:u0 + block].bfloat16() @ table.T
        s *= inv.to(s.dtype)[None, :]
        out_i[u0:u0 + block] = torch.topk(s, k, dim=1).indices
    return out_i


def parent_entries(path, users, table, inv, eidx, eoff, flt, prior, gain, k, dev):
    """nr_topk_users, nr_topk_users_filtered and nr_topk_users_prior of another build of the library
    on the given buffers: {name: call}, and the (idx, scores, keys) they write."""
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in {**_lib.TOPK_SIGNATURES, **_lib.FILTER_SIGNATURES, **_lib.PRIOR_SIGNATURES}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    U, N = users.shape[0], table.shape[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(lib.nr_topk_users_prior_workspace_bytes(_lib.NR_BF16, U, N, k), dtype=torch.uint8, device=dev)
    o = tuple(torch.empty((U, k), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32))
    head = (_lib.NR_BF16, 1024, U, p(users), N, p(table), table.stride(0), p(inv), p(eidx), p(eoff))
    tail = lambda *keys: (k, p(o[0]), p(o[1]), *keys, p(ws), ws.numel(),
                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    fptr = tuple(p(flt[n]) for n in ("news_time", "time_lo", "time_hi", "news_cat", "cat_mask"))

    def plain():
        assert lib.nr_topk_users(*head, *tail()) == 0, lib.nr_last_error()

    def filtered():
        assert lib.nr_topk_users_filtered(*head, *fptr, *tail()) == 0, lib.nr_last_error()

    def with_prior():
        assert lib.nr_topk_users_prior(*head, *(None,) * 5, p(prior), p(gain), *tail(p(o[2]))) == 0, lib.nr_last_error()
    return {"topk": plain, "filtered": filtered, "prior": with_prior}, o, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--users", type=int, default=255_990)
    ap.add_argument("--news", type=int, default=72_023)
    ap.add_argument("--torch-block", type=int, default=16_384)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-deep", action="store_true")
    ap.add_argument("--parent-lib", type=Path, default=None)
    ap.add_argument("--parent-first", action="store_true")
    ap.add_argument("--out", type=Path, default=Path("profiles/page/page_probe.json"))
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
           "chunk_rows": int(ops._lib.load().nr_topk_chunk_rows()), "parent_first": args.parent_first, "cases": []}

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
        return case

    for k in (10, 64):
        ws = torch.empty(ops.topk_users_after_workspace_bytes(torch.bfloat16, U, N, k), dtype=torch.uint8, device=dev)
        o = tuple(torch.empty((U, k), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32))
        ex = dict(excl_idx=eng.hist_idx, excl_off=eng.hist_off, workspace=ws)
        pri = dict(news_prior=prior, user_gain=gain)
        # the cursors behind page 1, without and with the prior (made once; every timed page 2 starts there)
        c1 = ops.topk_users_after(users, tab, inv, k, out=o, **ex)[3]
        c1p = ops.topk_users_after(users, tab, inv, k, out=o, **pri, **ex)[3]
        nxt = ops.start_cursor(U, dev)
        page = lambda **kw: ops.topk_users_after(users, tab, inv, k, out=o, next_out=nxt, excl_checked=True, **kw, **ex)
        plain = lambda: ops.topk_users(users, tab, inv, k, out=o[:2], **ex)
        fns = {"topk": plain,
               "filtered": lambda: ops.topk_users_filtered(users, tab, inv, k, out=o[:2], **flt, **ex),
               "prior": lambda: ops.topk_users_prior(users, tab, inv, k, out=o, **pri, **ex),
               "after_p1": lambda: page(),
               "after_p2": lambda: page(after=c1),
               "after_p2_prior": lambda: page(after=c1p, **pri),
               "topk_again": plain}
        equal = {}
        if args.parent_lib is not None:
            old, po, pws = parent_entries(args.parent_lib, users, tab, inv, eng.hist_idx, eng.hist_off, flt, prior, gain,
                                          k, dev)
            for a, fn in old.items():
                fns[a]()
                fn()
                torch.cuda.synchronize()
                equal[a] = all(torch.equal(x, y) for x, y in zip(o[:3 if a == "prior" else 2], po))
                fns["parent_" + a] = fn
            if args.parent_first:
                fns = {**{n: f for n, f in fns.items() if n.startswith("parent_")},
                       **{n: f for n, f in fns.items() if not n.startswith("parent_")}}
        case = {"K": k, "workspace_bytes": int(ws.numel()), **measure(fns)}
        if equal:
            case["equal_to_parent"] = equal
        case["repeat_spread_ms"] = round(abs(case["topk_ms"] - case["topk_again_ms"]), 3)
        case["round_spread_ms"] = round(max(max(case[n + "_ms_all"]) - min(case[n + "_ms_all"]) for n in fns), 3)
        del ws, o
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)

    if not args.no_deep:
        ws = torch.empty(ops.topk_users_after_workspace_bytes(torch.bfloat16, U, N, 64), dtype=torch.uint8, device=dev)
        pages = [tuple(torch.empty((U, 64), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32))
                 for _ in range(4)]

        def deep_pages():
            cur = ops.start_cursor(U, dev)
            for p in range(4):
                ops.topk_users_after(users, tab, inv, 64, after=cur, next_out=cur, out=pages[p], excl_idx=eng.hist_idx,
                                     excl_off=eng.hist_off, workspace=ws, excl_checked=True)
            idx, sc, ky = (torch.cat([pg[i] for pg in pages], dim=1) for i in range(3))
            by_row = torch.sort(idx, dim=1, stable=True).indices
            order = by_row.gather(1, torch.sort(ky.gather(1, by_row), dim=1, descending=True, stable=True).indices)
            return idx.gather(1, order), sc.gather(1, order)

        fns = {"deep256_pages": deep_pages, "recommend_deep": lambda: eng.recommend_deep(256, page=64)}
        if not args.no_torch:
            fns["torch256"] = lambda: torch_route(users, tab, inv, 256, args.torch_block)
        deep = {"k": 256, "page": 64, **measure(fns)}
        print(json.dumps(deep), file=sys.stderr, flush=True)
        out["deep"] = deep
    line = json.dumps(out)
    print(line, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
