"""Pool+score stage at a synthetic MIND shape: today's kernel against the column-sliced path
at W = 64 and W = 128 (bf16), HIP events over `reps` launches, `rounds` interleaved rounds
(profiles/sliced/stage_*.jsonl).  Run from the repository root:
  python tools/sliced_stage_probe.py SHAPE OUT.jsonl [reps] [rounds] [mode] [pooler]
mode: time (default) | prof (three launches of each after a warm-up, for rocprofv3: kernel
trace, or counters in a run of their own)"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from news_recommendation_project_v2_amd import engine, ops, synthetic  # noqa: E402

shape = sys.argv[1]
out = sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
mode = sys.argv[5] if len(sys.argv) > 5 else "time"
pooler = sys.argv[6] if len(sys.argv) > 6 else "latent"

dev = torch.device("cuda:0")
n_news, n_imp = synthetic.SHAPES[shape]
t0 = time.time()
imps = synthetic.mind_impressions(n_news, n_imp, seed=1234)
table = bench.news_table(n_news, dev)
model = bench.make_model(pooler, dev)
eng = engine.PoolScoreEngine(model, dtype=torch.bfloat16, device=dev).load_news(table)
eng.load_impressions(imps.hist_idx, imps.hist_len, imps.cand_idx, imps.cand_len)
assert eng.user_idx is None
eng.hist_table = eng.transform(out=eng.hist_table)
eng.inv_norms()
scores = {w: torch.empty(imps.n_cand, dtype=torch.float32, device=dev) for w in (0, 64, 128)}
torch.cuda.synchronize()
print(f"setup {time.time() - t0:.1f}s N={n_news} I={imps.n_imp} C={imps.n_cand} H={imps.n_hist}", flush=True)


def run(w):
    engine.SLICED_W = engine.SLICED_W_FINAL = w
    engine.SLICED_MIN_TABLE_BYTES = 0
    return eng.pool_score(scores=scores[w])[0]


for w in (0, 64, 128):  # warm-up: images, workspaces, code objects
    run(w)
    torch.cuda.synchronize()
    print("warm", w, flush=True)
if mode == "prof":
    for w in (0, 64, 128):
        for _ in range(3):
            run(w)
        torch.cuda.synchronize()
    sys.exit(0)

res = {"shape": shape, "pooler": pooler, "n_news": n_news, "imp": imps.n_imp, "cand": imps.n_cand,
       "hist": imps.n_hist, "reps": reps, "rounds": []}
for w in (64, 128):
    d = (scores[w] - scores[0])
    ok = ~torch.isnan(scores[0])
    res[f"maxdiff_{w}"] = float(d[ok].abs().max())
    res[f"nan_equal_{w}"] = bool(torch.equal(torch.isnan(scores[w]), ~ok))
    again = scores[w].clone()
    run(w)
    torch.cuda.synchronize()
    res[f"bit_equal_rerun_{w}"] = bool(torch.equal(again.view(torch.int32), scores[w].view(torch.int32)))
print(json.dumps({k: v for k, v in res.items() if k != "rounds"}), flush=True)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


parts = 2 if pooler == "final" else 1
for r in range(rounds):
    row = {}
    for w in (0, 64, 128):
        row[f"pool_score_ms_{w}"] = round(timed(lambda: run(w), reps), 4)
    for w in (64, 128):  # the per-step re-layout of the transformed table alone
        row[f"slice_hist_ms_{w}"] = round(timed(lambda: ops.slice_table(eng.hist_table, w, parts, out=eng._hist_image
                                                                       if eng._hist_image.shape[2] == parts * w else None), reps), 4)
    res["rounds"].append(row)
    print(json.dumps(row), flush=True)
with open(out, "w") as f:
    f.write(json.dumps(res) + "\n")
print("done", flush=True)
