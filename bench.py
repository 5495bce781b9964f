#!/usr/bin/env python3
"""Headline benchmark: scored candidates/sec on MIND-large-shaped impressions.

    python bench.py [--gpus N --steps K --warmup W --pooler latent|final --dtype bf16|fp32
                     --scaling strong|weak --backend nccl|gloo --dump-outputs DIR --full]

A plain run sets up, warms up, times the K steps, writes its outputs if
``--dump-outputs DIR`` is given (the scores of the last timed step as
``DIR/scores.npy``, float32; per rank ``scores_rank<r>.npy`` at N > 1) and
prints the result line with the headline figure (``value``, ``ms_per_step``).
Everything else described below (roofline, CPU baseline, AUC gates, the other
poolers / precisions / shapes, the multi-rank parity checks and extras) runs
only with ``--full``, which prints the same line with those fields added.

Workload (BASELINE.json configs[2] at N = 1, configs[3] at N > 1): synthetic
MIND-large-dev-shaped impressions (N = 72,023 news, I = 376,471 impressions,
h ~ geometric(1/33), c ~ geometric(1/37)), a seeded N(0,1) news table resident
in HBM, deterministic random-init pooler weights (no checkpoint exists).  One
step = the per-news pooler transform (MFMA GEMM chain) + candidate inverse
norms + the fused pool+score kernel, i.e. everything `scripts/eval.py`
computes between loading the table and ranking.

Multi-GPU (one process per GPU, RCCL over xGMI).  ``--gpus N`` with no
WORLD_SIZE in the environment re-launches this script under
``torch.distributed.run`` with N ranks (as a child process, before any GPU
call).  Every rank transforms 1/N of the news table and one RCCL all-gather
gives every GPU the whole table (the path's one exchange step); impressions
are the shard unit.  Default ``--scaling strong`` = BASELINE configs[3] as ONE
eval job: the MIND-large-dev set split into N contiguous cost-balanced ranges
(``partition_by_cost``); ``value`` = the set's candidates / the step time,
timed from a barrier to the last rank's completion (max over ranks); the
per-rank pool_score times and their max / mean are in ``extra``.  At N > 1
the extras add the same strong-scaling step on the MIND-large *test* shape
(2.37 M impressions, so per-GPU work stays large at N = 8) and the weak-scaling
reading (``--scaling weak``: every rank its own full MIND-large-dev-sized set,
per-GPU work fixed as N grows, rank 0's set = the N = 1 set).

With ``--full``, also reported in the same JSON line:
  roofline      the pool+score kernel (dominant; a random-row gather served by
                HBM + Infinity Cache): algorithmic bytes per launch / its
                HIP-event average duration, vs the 8 TB/s HBM spec and vs the
                measured random-row gather ceiling of the microarch guide
  cpu_baseline  the oracle (the reference algorithm restated on PyTorch CPU:
                padded batches of 128, pooler per padded slot, per-impression
                cosine loop) on this host's CPU share (all affinity cores, or
                OMP_NUM_THREADS where the pool declares a per-GPU share), on the
                first 1,000 impressions of a MIND-small-shaped set (configs[0]),
                for both poolers, and on the first 10,000
                (capped at --cpu-10k-seconds of CPU time per
                pooler, the impressions done reported; --no-cpu-10k drops it)
  extra         the FinalAttention pooler, f32, per-stage times, AUC of the GPU
                path vs the CPU reference on the config-1 sample, MIND-large
                test shape, Zipf ids, device metrics, PCIe costs, config 5
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import socket
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

from news_recommendation_project_v2_amd import _lib, synthetic  # noqa: E402
from news_recommendation_project_v2_amd import weights as W  # noqa: E402
from news_recommendation_project_v2_amd.distributed import ShardedTable, partition_by_cost, sharded_step  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
# measured random-row gather rate of a ~151 MB table, every CU gathering
# (MI355X_MICROARCH.md "Indexed rows": 7.4-7.9 TB/s); the upper end is used
GATHER_CEILING_GBS = 7900.0
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


PHASE_ENV = "NR_BENCH_PHASE_DIR"


def phase(name: str) -> None:
    """Record this rank's current phase (a file per rank under $NR_BENCH_PHASE_DIR,
    written by rename so the parent never reads half a line): when the launch
    has to be killed, spawn_ranks reports where every rank was.  A test hook
    (NR_BENCH_TEST_STALL="rank:phase") parks that rank at that phase forever,
    as a rank stuck in a collective would be."""
    d = os.environ.get(PHASE_ENV)
    rank = os.environ.get("RANK", "0")
    if d:
        tmp = Path(d) / f".rank{rank}.tmp"
        tmp.write_text(json.dumps({"phase": name, "t": time.time()}))
        tmp.replace(Path(d) / f"rank{rank}")
    if os.environ.get("NR_BENCH_TEST_STALL") == f"{rank}:{name}":
        while True:
            time.sleep(3600)


def _phases(d: Path, n: int) -> dict:
    out = {}
    for r in range(n):
        try:
            rec = json.loads((d / f"rank{r}").read_text())
            out[str(r)] = {"phase": rec["phase"], "seconds_in_phase": round(time.time() - rec["t"], 1)}
        except (OSError, ValueError, KeyError):
            out[str(r)] = {"phase": "not started", "seconds_in_phase": None}
    return out


def spawn_ranks(n: int, argv: list, stall_s: float = 300.0, wall_s: float = 1800.0) -> int:
    """Run this script under torch.distributed.run with n ranks (child process
    group; nothing here has touched the GPU) and return its exit code.  A launch
    that stops making progress -- no rank changes phase for `stall_s`, or the
    whole run passes `wall_s` -- is killed (the whole process group) and one
    JSON line with value null names every rank's phase, so a stuck RCCL init
    or collective ends with a record instead of at the driver's kill with no
    line at all.  If rank 0 already printed its result line
    and only the teardown hangs, the stragglers are killed and 0 returned."""
    import shutil
    import signal
    import tempfile
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(Path(__file__).resolve()), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    pdir = Path(tempfile.mkdtemp(prefix="nr_bench_phase_"))
    env[PHASE_ENV] = str(pdir)
    log("[bench] launching", " ".join(cmd))
    t0 = time.time()
    proc = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        while True:
            try:
                return proc.wait(timeout=1.0)
            except subprocess.TimeoutExpired:
                pass
            ph = _phases(pdir, n)
            started = [v["seconds_in_phase"] for v in ph.values() if v["seconds_in_phase"] is not None]
            newest = min(started) if started else time.time() - t0
            elapsed = time.time() - t0
            if newest < stall_s and elapsed < wall_s:
                continue
            why = "stalled" if newest >= stall_s else "wall"
            done = ph.get("0", {}).get("phase") == "printed"
            try:
                os.killpg(proc.pid, signal.SIGTERM)
                proc.wait(timeout=15)
            except (subprocess.TimeoutExpired, ProcessLookupError):
                try:
                    os.killpg(proc.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                proc.wait()
            if done:
                log(f"[bench] rank 0 printed its line; teardown {why} ({json.dumps(ph)}): stragglers killed")
                return 0
            print(json.dumps({"metric": "scored candidates/sec on MIND-large impressions; AUC parity vs CPU ref",
                              "value": None, "unit": "scored candidates/s", "n_gpus": n, "higher_is_better": True,
                              "error": (f"no rank changed phase for {stall_s:.0f} s" if why == "stalled" else
                                        f"the launch passed its {wall_s:.0f} s wall limit") + "; killed",
                              "elapsed_s": round(elapsed, 1), "rank_phases": ph}), flush=True)
            return 124
    finally:
        shutil.rmtree(pdir, ignore_errors=True)


def make_model(pooler: str, dev):
    from news_recommendation_project_v2_amd.latent_attention import LatentAttentionModel
    from news_recommendation_project_v2_amd.modeling_utils import FinalAttention
    if pooler == "final":
        m = FinalAttention(1024, 4096)
        m.load_state_dict(W.final_attention_state_dict(1234))
    else:
        m = LatentAttentionModel()
        m.load_state_dict(W.latent_attention_state_dict(1234))
    return m.to(dev).eval()


def state_dict(pooler: str) -> dict:
    return W.final_attention_state_dict(1234) if pooler == "final" else W.latent_attention_state_dict(1234)


def news_table(n: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    return torch.randn((n, 1024), generator=g, device=dev, dtype=torch.float32)


def ps_bytes(imps, pooler: str, es: int) -> int:
    """Algorithmic bytes of one pool+score launch (streaming model:
    every gathered row counted once per use)."""
    k = 2 if pooler == "final" else 1
    return (imps.n_cand * (1024 * es + 4 + 4 + 4) + imps.n_hist * (k * 1024 * es + 4) + imps.n_imp * 16)


def tx_flops(n: int, pooler: str) -> float:
    if pooler == "final":
        return n * 2.0 * (1024 * 4096 * 2 + 4096 * 4096 + 4096 * 1024 * 2)
    # folded latent: 1024->512, 512->1024, 1024->8192, 4096->1024
    return n * 2.0 * (1024 * 512 + 512 * 1024 + 1024 * 8192 + 4096 * 1024)


class Run:
    """One pooler/dtype on one rank: engine + its impression range + sharded table."""

    def __init__(self, pooler, dtype, imps, table, dev, rank, world, chunks=1):
        from news_recommendation_project_v2_amd.engine import PoolScoreEngine
        self.pooler, self.dtype = pooler, dtype
        self.model = make_model(pooler, dev)
        self.eng = PoolScoreEngine(self.model, dtype=DTYPES[dtype], device=dev).load_news(table)
        self.eng.load_impressions(imps.hist_idx, imps.hist_len, imps.cand_idx, imps.cand_len)
        self.tab = ShardedTable(self.eng, rank, world, chunks=chunks)
        self.scores = torch.empty(imps.n_cand, dtype=torch.float32, device=dev)
        self.imps = imps

    def step(self):
        return sharded_step(self.tab, scores=self.scores)

    def stage_times(self, reps: int = 3):
        """HIP-event times (ms) of each stage, events on the launch stream."""
        s = torch.cuda.current_stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        acc = np.zeros(3)
        split = np.zeros(2)
        self.tab.timing = True
        for _ in range(reps):
            ev[0].record(s)
            self.tab.build()
            ev[1].record(s)
            self.eng.inv_norms()
            ev[2].record(s)
            self.eng.pool_score(scores=self.scores)
            ev[3].record(s)
            torch.cuda.synchronize()
            acc += [ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])]
            t, g = self.tab.last_ms()
            split += [t, g if g is not None else float("nan")]
        self.tab.timing = False
        self.split_ms = split / reps  # (transform, all-gather) of the table build
        return acc / reps


DUMP_MAX_BYTES = 60_000_000  # per array; the headline's 13.9 M float32 scores fit whole


def dump_outputs(out_dir: str, arrays: dict) -> dict:
    """--dump-outputs: write what the timed path returned in its last step as
    <name>.npy (float32).  An array above DUMP_MAX_BYTES is cut to a fixed
    sample (sorted positions drawn once from seed 1234) so that two builds dump
    the same elements.  Returns {name: elements written}."""
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    written = {}
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy().reshape(-1)
        cap = DUMP_MAX_BYTES // 4
        if a.size > cap:
            a = a[np.sort(np.random.default_rng(1234).choice(a.size, cap, replace=False))]
        np.save(d / f"{name}.npy", np.ascontiguousarray(a, dtype=np.float32))
        written[name] = int(a.size)
    return written


def timed(step, steps: int, warmup: int, world: int, dev, host_reduce: bool, keep: list = None):
    """Warmup, then `steps` steps bracketed by barrier + device sync; max over ranks.
    `keep` (a list) receives what the last timed step returned."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(steps):
        last = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if keep is not None:
        keep.append(last)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if host_reduce else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def rank_parity(run: Run, n_check: int = 200, seed: int = 0) -> float:
    """Max |score - float64 re-pool| over `n_check` sampled impressions of this
    rank's range, re-pooled from the rank's own (all-gathered) table and
    candidate rows in float64 (tests/test_gpu_parity.py
    test_full_size_mind_large_properties): FinalAttention sum x p / (sum p +
    1e-10), latent normalize(mean); cosine with the per-vector 1e-8 clamps."""
    s, _ = run.step()
    torch.cuda.synchronize()
    imps, eng = run.imps, run.eng
    if imps.n_imp == 0:
        return 0.0
    rng = np.random.default_rng(seed)
    ho, co = imps.hist_off(), imps.cand_off()
    dev = s.device
    tab, cand = eng.hist_table, eng.cand_table
    err = 0.0
    for i in rng.choice(imps.n_imp, min(n_check, imps.n_imp), replace=False):
        rows = tab[torch.as_tensor(imps.hist_idx[ho[i]:ho[i + 1]], dtype=torch.long, device=dev)].double()
        if run.pooler == "final":
            x, p = rows[:, :1024], rows[:, 1024:]
            u = (x * p).sum(0) / (p.sum(0) + 1e-10)
        else:
            u = rows.mean(0)
            u = u / u.norm().clamp_min(1e-12)
        e = cand[torch.as_tensor(imps.cand_idx[co[i]:co[i + 1]], dtype=torch.long, device=dev)].double()
        ref = (e @ u) / u.norm().clamp_min(1e-8) / e.norm(dim=1).clamp_min(1e-8)
        err = max(err, float((s[co[i]:co[i + 1]].double() - ref).abs().max()))
    return err


def rank_balance(pool_ms: float, imps, dev, host_reduce: bool, world: int) -> dict:
    """Every rank's pool_score time and candidate count (all-gathered), with the
    max / mean of the times: how evenly partition_by_cost split the work."""
    red = "cpu" if host_reduce else dev
    mine = torch.tensor([pool_ms, float(imps.n_cand), float(imps.n_imp)], dtype=torch.float64, device=red)
    allr = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allr, mine)
    t = [float(x[0]) for x in allr]
    return {"pool_score_ms_per_rank": [round(x, 4) for x in t],
            "candidates_per_rank": [int(x[1]) for x in allr], "impressions_per_rank": [int(x[2]) for x in allr],
            "pool_score_max_over_mean": round(max(t) / (sum(t) / len(t)), 4) if sum(t) > 0 else None}


def table_digest(t: torch.Tensor) -> int:
    """Order-sensitive integer digest of a table's bytes (equal on every rank
    iff the all-gathered tables agree, up to a 2^-63 collision chance)."""
    v = t.contiguous().view(torch.int16).to(torch.int64).flatten()
    w = torch.arange(1, v.numel() + 1, device=v.device, dtype=torch.int64) % 1_000_003
    return int(((v * w).sum() % (2 ** 61 - 1)).item())


def auc_of(run: Run) -> float:
    """Mean AUC over all impressions: dense ranks + per-impression metrics on the
    device (nr_dense_rank, nr_impression_metrics; == evaluation.score, tested)."""
    from news_recommendation_project_v2_amd import evaluation
    s, _ = run.step()
    r = run.eng.rank(s)
    return float(evaluation.score_device(r, run.imps.labels, run.imps.cand_off())["auc"])


def metrics_ms(run: Run, reps: int = 3) -> float:
    """Device time of dense ranks + MIND metrics over the whole workload."""
    from news_recommendation_project_v2_amd import ops
    s, _ = run.step()
    y = torch.as_tensor(np.asarray(run.imps.labels, dtype=np.float32)).to(s.device)
    off = torch.as_tensor(run.imps.cand_off()).to(s.device)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        r = run.eng.rank(s)
        ops.impression_metrics(r, y, off)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def train_step_ms(dev, batch_rows: int = 256, steps: int = 30, pooler: str = "final", warmup: int = 10) -> dict:
    """Config 5 (BASELINE configs[4]): one train step (fwd + bwd + clip + AdamW) on a
    synthetic MIND-shaped batch: FinalAttentionTrainStep in bf16 MFMA, or with
    pooler="latent" LatentAttentionTrainStep (one nr_latent_train_step call: bf16
    operands and activations, f32 accumulation / statistics / gradients)."""
    from news_recommendation_project_v2_amd.modeling_utils import FinalAttention, get_token_attn_model
    from news_recommendation_project_v2_amd.train_step import FinalAttentionTrainStep, TrainBatch
    rng = np.random.default_rng(1234)
    h = np.clip(rng.geometric(1 / 33.0, batch_rows), 1, 600)
    ids = rng.integers(0, 40_000, int(h.sum()) + 2 * batch_rows)
    uniq, rev = np.unique(ids, return_inverse=True)
    Hs = int(h.sum())
    tok = torch.randn((len(uniq), 1024), generator=torch.Generator().manual_seed(1)).half().to(dev)
    b = TrainBatch(tok, torch.as_tensor(rev[:Hs].astype(np.int32)).to(dev),
                   torch.as_tensor(np.concatenate([[0], np.cumsum(h)]).astype(np.int64)).to(dev),
                   torch.as_tensor(rev[Hs:Hs + batch_rows].astype(np.int32)).to(dev),
                   torch.as_tensor(rev[Hs + batch_rows:].astype(np.int32)).to(dev))
    tm = get_token_attn_model()
    tm.load_state_dict(W.token_attn_state_dict(1234))
    if pooler == "latent":  # configs[4]'s pairing: token encoder + LatentAttentionModel
        from news_recommendation_project_v2_amd.latent_attention import LatentAttentionModel
        from news_recommendation_project_v2_amd.train_step import LatentAttentionTrainStep
        lm = LatentAttentionModel()
        lm.load_state_dict(W.latent_attention_state_dict(1234))
        eng = LatentAttentionTrainStep(tm, lm.to(dev), dtype=torch.bfloat16, device=dev)
    else:
        fa = FinalAttention(1024, 4096)
        fa.load_state_dict(W.final_attention_state_dict(1234))
        eng = FinalAttentionTrainStep(tm, fa.to(dev), dtype=torch.bfloat16, device=dev)
    for _ in range(warmup):  # (after the eval legs: let the clocks settle on this load)
        eng.step(b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.step(b)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    hb = eng.hbm_bytes_per_step(Hs, len(uniq))
    bound_s = eng.flops_per_step(Hs) / (MFMA_PEAK_TFLOPS["bf16"] * 1e12) + sum(hb.values()) / (HBM_PEAK_GBS * 1e9)
    out = {"pooler": pooler, "dtype": "bf16", "batch_rows": batch_rows,
           "history_slots": Hs, "ms_per_step": round(ms, 3), "rows_per_s": round(batch_rows / ms * 1e3, 1),
           "gemm_tflops": round(eng.flops_per_step(Hs) / ms / 1e9, 1),
           # (executed GEMM FLOPs / 2.5 PF + AdamW and row-kernel bytes / 8 TB/s) / measured step
           "step_roofline_frac": round(bound_s / (ms * 1e-3), 4), "step_bound_ms": round(bound_s * 1e3, 4),
           "hbm_bytes_model": {k: int(v) for k, v in hb.items()}}
    if hasattr(eng, "model_flops_per_step"):
        # the latent step runs the last linear layer over B rows (the history mean commutes
        # with it): gemm_tflops counts the FLOPs executed; model_tflops_equiv the reference
        # formulation's per-slot GEMM FLOPs over the same time (what rounds 1-3 reported)
        out["model_tflops_equiv"] = round(eng.model_flops_per_step(Hs) / ms / 1e9, 1)
        out["flops_basis"] = ("gemm_tflops: FLOPs executed; model_tflops_equiv: the per-slot formula of "
                              "rounds 1-3 (VERDICT r3's 298 -> 450 TF/s target is in this basis)")
    return out


def config2_leg(dev, n_news: int = 8192) -> dict:
    """BASELINE configs[1] rates (f32): the 24-layer XLM-R-large-shaped title
    encoder over n_news synthetic titles, query (~46 tokens) + passage (~20)
    passes as save_emb.py runs them, and one f32 FinalAttention eval step over
    the whole MIND-small-dev-shaped impression set.  The full-size chain is
    tests/test_config2.py."""
    sys.path.insert(0, str(REPO / "scripts"))
    from save_emb import synthetic_titles
    from news_recommendation_project_v2_amd.encoder import XLMREncoder
    out = {}
    enc = XLMREncoder(W.xlmr_state_dict(1234, 24, 50_000), dtype=torch.float32, device=dev)
    p_ids, p_lens = synthetic_titles(n_news, 1234, 50_000, 20)
    q_ids, q_lens = synthetic_titles(n_news, 1234, 50_000, 20, prefix_len=26)
    enc.encode_packed(p_ids[:int(p_lens[:256].sum())], p_lens[:256], normalize=True)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc.encode_packed(q_ids, q_lens, normalize=True)
    enc.encode_packed(p_ids, p_lens, normalize=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tok = int(p_lens.sum() + q_lens.sum())
    out["encoder_f32"] = {"news": n_news, "tokens": tok, "seconds": round(dt, 3), "tokens_per_s": round(tok / dt, 1),
                          "news_per_s": round(n_news / dt, 1),
                          "tflops": round(tok * 603_979_776 / dt / 1e12, 1)}
    del enc
    _lib.empty_cache()
    n_news_s, n_imp_s = synthetic.SHAPES["mind_small_dev"]
    im = synthetic.mind_impressions(n_news_s, n_imp_s, seed=1234)
    r = Run("final", "fp32", im, news_table(n_news_s, dev), dev, 0, 1)
    d = timed(r.step, 3, 1, 1, dev, False) / 3
    out["eval_f32_final"] = {"impressions": im.n_imp, "candidates": im.n_cand, "ms_per_step": round(d * 1e3, 3),
                             "value": round(im.n_cand / d, 1)}
    del r
    _lib.empty_cache()
    return out


def host_parse_leg(n_news: int, rows: int = 100_000) -> dict:
    """SURVEY §8(d) 'report separately: host parsing (A1)': the native behaviours
    parser (split_impressions_and_history, libnewsrec_host.so) on the first
    `rows` MIND-large-dev-shaped behaviours lines (synthetic text of the
    headline's impressions), host time."""
    from news_recommendation_project_v2_amd import native
    imps = synthetic.mind_impressions(n_news, rows, seed=1234)
    hist, impr = synthetic.to_behaviors(imps)
    nbytes = sum(map(len, impr)) + sum(len(h) for h in hist if h)
    native.split_behaviors(impr[:1000], hist[:1000])  # load the library
    t0 = time.perf_counter()
    out = native.split_behaviors(impr, hist)
    dt = time.perf_counter() - t0
    assert out is not None
    return {"rows": rows, "text_MB": round(nbytes / 1e6, 1), "seconds": round(dt, 3),
            "rows_per_s": round(rows / dt, 1), "MB_per_s": round(nbytes / dt / 1e6, 1)}


def hipblaslt_yardstick(pooler: str, n: int, ours_ms: float, dev, reps: int = 10, rounds: int = 5) -> dict:
    """The same per-news transform GEMM shapes (M = n) as bare torch.matmul
    (hipBLASLt: bf16, no bias, no LayerNorm, no epilogue, so less work than
    the fused transform) beside our own bf16 GEMM on each shape with the
    transform's epilogue (bias + ReLU / exp / softmax64 / GEGLU / residual; the
    LayerNorm fold of S and ff1 aside), interleaved in rounds (medians), and
    the fused transform's own time: a vendor-library yardstick per shape and
    for transform_peak_frac.  Yardstick only; the product path never calls it."""
    from news_recommendation_project_v2_amd import ops
    shapes = ([(4096, 1024, "relu"), (4096, 4096, "relu"), (1024, 4096, "none"), (4096, 1024, "relu"),
               (1024, 4096, "exp")] if pooler == "final" else
              [(512, 1024, "softmax64"), (1024, 512, "resadd"), (8192, 1024, "geglu"), (1024, 4096, "resadd")])
    g = torch.Generator(device=dev).manual_seed(7)
    per, ours = [], []
    for nn, kk, epi in shapes:
        a = torch.randn((n, kk), device=dev, generator=g).bfloat16()
        w = (torch.randn((nn, kk), device=dev, generator=g) * kk ** -0.5).bfloat16()
        b = torch.randn(nn, device=dev, generator=g) * 0.1
        nc = nn // 2 if epi == "geglu" else nn
        r = torch.randn((n, nc), device=dev, generator=g).bfloat16() if epi == "resadd" else None
        out = torch.empty((n, nc), device=dev, dtype=torch.bfloat16)
        fns = {"hipblaslt": lambda: torch.matmul(a, w.T),
               "ours": lambda: ops.gemm(a, w, b, epilogue=epi, residual=r, out=out)}
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps)
        per.append(round(float(np.median(times["hipblaslt"])), 4))
        ours.append(round(float(np.median(times["ours"])), 4))
        del a, w, b, r, out
    _lib.empty_cache()
    tot = sum(per)
    fl = tx_flops(n, pooler)
    ratio = [round(o / h, 3) for o, h in zip(ours, per)]
    return {"shapes_NK_epi": shapes, "hipblaslt_ms_each": per, "ours_ms_each": ours, "ours_over_hipblaslt_each": ratio,
            "every_shape_at_most_hipblaslt": all(x <= 1.0 for x in ratio), "hipblaslt_sum_ms": round(tot, 4),
            "hipblaslt_peak_frac": round(fl / (tot * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS["bf16"], 3),
            "fused_transform_ms": round(float(ours_ms), 4), "fused_over_hipblaslt_time": round(ours_ms / tot, 3)}


def encoder_bf16_leg(dev, n_news: int = 16384) -> dict:
    """BASELINE configs[2]'s embedding step in bf16: the 24-layer XLM-R-large-
    shaped title encoder (packed varlen, nr_encoder_forward) over n_news
    synthetic titles, query (~46 tokens) + passage (~20) passes as save_emb.py
    runs them; tokens/s, news/s and the GEMM+attention FLOP rate against the
    2.5 PF dense bf16 peak (0.604 GFLOP per token + 4 L^2 1024 per sequence and
    layer)."""
    sys.path.insert(0, str(REPO / "scripts"))
    from save_emb import synthetic_titles
    from news_recommendation_project_v2_amd.encoder import XLMREncoder
    enc = XLMREncoder(W.xlmr_state_dict(1234, 24, 50_000), dtype=torch.bfloat16, device=dev)
    p_ids, p_lens = synthetic_titles(n_news, 1234, 50_000, 20)
    q_ids, q_lens = synthetic_titles(n_news, 1234, 50_000, 20, prefix_len=26)
    enc.encode_packed(q_ids, q_lens, normalize=True)  # warm-up at the full size
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc.encode_packed(q_ids, q_lens, normalize=True)
    enc.encode_packed(p_ids, p_lens, normalize=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tok = int(p_lens.sum() + q_lens.sum())
    sq = float((np.asarray(p_lens, dtype=np.float64) ** 2).sum() + (np.asarray(q_lens, dtype=np.float64) ** 2).sum())
    flops = tok * 603_979_776 + 24 * 4 * 1024 * sq
    del enc
    _lib.empty_cache()
    return {"news": n_news, "tokens": tok, "seconds": round(dt, 3), "tokens_per_s": round(tok / dt, 1),
            "news_per_s": round(n_news / dt, 1), "tflops": round(flops / dt / 1e12, 1),
            "peak_frac": round(flops / dt / 2.5e15, 3)}


def api_end_to_end(pooler: str, dtype: str, imps, table_cpu: torch.Tensor, dev, reps: int = 3) -> dict:
    """The drop-in API call the reference's scripts/eval.py makes,
    data_model_helper.get_final_second_attention_score (data_model_helper.py:416-443),
    on the whole headline set from host inputs to host outputs: numpy CSR
    indices + the CPU news table in, scores + per-impression dense ranks (object
    array) out.  Phases (data_model_helper.PROFILE, a device sync between them):
    setup_upload (engine, pooler weights, table and index arrays host -> HBM),
    device (transform + pool + score + dense ranks), download (scores + ranks),
    host (grouping the ranks into per-impression arrays, the reference's return
    format).  Medians over `reps` calls after one warm-up call."""
    from news_recommendation_project_v2_amd import data_model_helper as dmh
    model = make_model(pooler, dev)
    hb = np.ones(imps.n_imp, dtype=bool)
    args = (np.asarray(imps.hist_idx), np.asarray(imps.hist_len), np.asarray(imps.cand_idx),
            np.asarray(imps.cand_len), table_cpu, hb, model)
    runs = []
    dmh.PROFILE = True
    try:
        for i in range(reps + 1):
            out = dmh.get_final_second_attention_score(*args, dtype=DTYPES[dtype])
            if i:
                runs.append(dict(dmh.LAST_TIMINGS))
            del out
    finally:
        dmh.PROFILE = False
    med = {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]}
    idx_b = int(4 * (imps.n_hist + imps.n_cand) + 8 * 2 * (imps.n_imp + 1))
    med.update({"pooler": pooler, "dtype": dtype, "impressions": imps.n_imp, "candidates": imps.n_cand,
                "table_bytes": int(table_cpu.numel() * 4), "index_bytes": idx_b,
                "download_bytes": int(8 * imps.n_cand),
                "download_GBs": round(8 * imps.n_cand / (med["download"] * 1e-3) / 1e9, 1),
                "candidates_per_s_end_to_end": round(imps.n_cand / (med["total"] * 1e-3), 1)})
    _lib.empty_cache()
    return med


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def cpu_reference(pooler: str, imps, table_cpu: torch.Tensor, budget_s: float):
    """The reference algorithm (oracle, PyTorch CPU f32: padded batches of 128,
    pooler per padded slot, per-impression cosine) over the given impressions,
    128 at a time, stopping early only if `budget_s` of CPU time is spent.
    Returns (impressions done, candidates done, seconds, scores)."""
    from oracle import pool_ref
    sd = state_dict(pooler)
    ho, co = imps.hist_off(), imps.cand_off()
    done_imp, t_used, parts = 0, 0.0, []
    while done_imp < imps.n_imp and t_used < budget_s:
        a, b = done_imp, min(done_imp + 128, imps.n_imp)
        t0 = time.perf_counter()
        parts.append(pool_ref.cos_sim_scores(pooler, sd, imps.hist_idx[ho[a]:ho[b]], imps.hist_len[a:b],
                                             imps.cand_idx[co[a]:co[b]], imps.cand_len[a:b], table_cpu))
        t_used += time.perf_counter() - t0
        done_imp = b
    return done_imp, int(co[done_imp]), t_used, torch.cat(parts).numpy()


def cpu_leg(args, dev) -> tuple:
    """the CPU reference restatement timed on this host's cores
    (all of its affinity set) on the first 1,000 impressions of a MIND-small-
    shaped set (configs[0]) for both poolers; the GPU path scores the same
    impressions (f32 and bf16) for the AUC / score parity check."""
    from news_recommendation_project_v2_amd import evaluation
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    from oracle import data_ref, pool_ref
    # The GPU pool gives each GPU a CPU share and says so in OMP_NUM_THREADS (16 per GPU)
    # while the affinity mask lists every CPU of the host (256): at 256 threads on that
    # share the restatement ran 74 cand/s against ~3k at 16 (profiles/round2/cpu_threads.txt).
    # Use the share when the pool declares one, else the whole affinity set.
    affinity = len(os.sched_getaffinity(0))
    cores = min(affinity, int(os.environ.get("OMP_NUM_THREADS") or affinity))
    torch.set_num_threads(cores)
    n_news, n_imp_full = synthetic.SHAPES[args.cpu_shape]
    full = synthetic.mind_impressions(n_news, n_imp_full, seed=1234)
    table_d = news_table(n_news, dev)
    table_c = table_d.cpu()
    samples = [args.cpu_impressions] + ([] if args.no_cpu_10k else [10_000])
    out, parity = {}, {}
    for pooler in ("latent", "final"):
        for n_imp in samples:
            imps = full.slice(0, n_imp)
            cap = args.cpu_seconds if n_imp == args.cpu_impressions else min(args.cpu_seconds, args.cpu_10k_seconds)
            done, ncand, secs, cpu_scores = cpu_reference(pooler, imps, table_c, cap)
            out.setdefault(pooler, {})[f"first_{n_imp}"] = {
                "impressions": done, "candidates": ncand, "seconds": round(secs, 2),
                "value": round(ncand / secs, 1), "cpu_seconds_cap": cap,
                "capped": done < n_imp}
            log(f"[bench] CPU reference {pooler} first {n_imp}: {done} imps {ncand} cands in {secs:.1f}s "
                f"= {ncand / secs:.0f} cand/s on {cores} threads")
            if n_imp != args.cpu_impressions:
                continue
            sub = imps.slice(0, done)
            grouped_y = sub.grouped_labels()
            cpu_m = data_ref.score(pool_ref.dense_ranks(cpu_scores, sub.cand_len), grouped_y)
            parity[pooler] = {"impressions": done, "candidates": ncand,
                              "cpu_ref": {k: cpu_m[k] for k in ("auc", "mrr", "ndcg5", "ndcg10")}}
            # the floor a bf16 table sets: the same CPU reference (f32 math) on the news
            # table rounded to bf16 -- what storing the inputs in bf16 alone moves the AUC
            _, _, _, s16 = cpu_reference(pooler, sub, table_c.bfloat16().float(), float("inf"))
            m16 = data_ref.score(pool_ref.dense_ranks(s16, sub.cand_len), grouped_y)
            parity[pooler]["cpu_ref_bf16_table"] = {
                "auc": m16["auc"], "auc_abs_diff": abs(m16["auc"] - cpu_m["auc"]),
                "max_abs_score_diff": float(np.abs(s16 - cpu_scores).max()),
                "note": "CPU reference, f32 math, news table rounded to bf16: the AUC shift of bf16 inputs alone"}
            for dt in ("fp32", "bf16"):
                eng = PoolScoreEngine(make_model(pooler, dev), dtype=DTYPES[dt], device=dev).load_news(table_d)
                eng.load_impressions(sub.hist_idx, sub.hist_len, sub.cand_idx, sub.cand_len)
                s, _ = eng.step()
                g = evaluation.score_device(eng.rank(s), sub.labels, sub.cand_off())
                d = {k: g[k] for k in ("auc", "mrr", "ndcg5", "ndcg10")}
                d["max_abs_score_diff"] = float(np.abs(s.cpu().numpy() - cpu_scores).max())
                d["auc_abs_diff"] = abs(g["auc"] - cpu_m["auc"])
                d["auc_equal_4dp"] = round(g["auc"], 4) == round(cpu_m["auc"], 4)
                if dt == "bf16":  # against the CPU reference fed the same bf16-rounded table
                    d["auc_abs_diff_vs_bf16_table_ref"] = abs(g["auc"] - m16["auc"])
                    d["max_abs_score_diff_vs_bf16_table_ref"] = float(np.abs(s.cpu().numpy() - s16).max())
                parity[pooler][f"gpu_{dt}"] = d
                del eng
    head = out[args.pooler][f"first_{args.cpu_impressions}"]
    base = {"value": head["value"], "unit": "scored candidates/s", "cores": cores, "kind": "port",
            "sample": f"first {head['impressions']} impressions ({head['candidates']} candidates) of the seeded "
                      f"{args.cpu_shape}-shaped set (configs[0]), {args.pooler} pooler (headline), f32, "
                      f"{head['seconds']}s on {cores} threads of {cpu_model()}; both poolers in by_pooler",
            "by_pooler": out, "affinity_cpus": affinity}
    return base, parity


AUC_4DP = 5e-5  # "AUC equal to the CPU reference to 4 decimal places": |diff| < half a unit in the 4th


def auc_gate_full(dev, poolers=("latent", "final"), dtype: str = "bf16") -> dict:
    """The north star's AUC gate at BASELINE configs[2] size: all 376,471
    MIND-large-dev-shaped impressions of the headline workload (same seed,
    labels and N(0,1) table), GPU `dtype` path (device scores -> device dense
    ranks -> device metrics) against the CPU reference in f32 (the oracle's
    per-news restatement of get_cos_sim_scores, pinned to the reference golden;
    per-impression AUC as score_row computes it).  CPU time is on this host's
    cores (torch.set_num_threads as the cpu_baseline leg)."""
    from news_recommendation_project_v2_amd import evaluation
    from news_recommendation_project_v2_amd.engine import PoolScoreEngine
    from oracle import data_ref, pool_ref
    n_news, n_imp = synthetic.SHAPES["mind_large_dev"]
    imps = synthetic.mind_impressions(n_news, n_imp, seed=1234)
    table_d = news_table(n_news, dev)
    table_c = table_d.cpu()
    out = {}
    for pooler in poolers:
        t0 = time.perf_counter()
        ref = pool_ref.cos_sim_scores_large(pooler, state_dict(pooler), imps.hist_idx, imps.hist_len, imps.cand_idx,
                                            imps.cand_len, table_c)
        auc_ref = float(np.nanmean(data_ref.impression_aucs(ref, imps.labels, imps.cand_len)))
        t_cpu = time.perf_counter() - t0
        eng = PoolScoreEngine(make_model(pooler, dev), dtype=DTYPES[dtype], device=dev).load_news(table_d)
        eng.load_impressions(imps.hist_idx, imps.hist_len, imps.cand_idx, imps.cand_len)
        s, _ = eng.step()
        r = eng.rank(s)
        g = evaluation.score_device(r, imps.labels, imps.cand_off())
        diff = abs(g["auc"] - auc_ref)
        out[pooler] = {"cpu_ref_f32_auc": auc_ref, f"gpu_{dtype}_auc": g["auc"], "auc_abs_diff": diff,
                       "auc_equal_4dp": bool(diff < AUC_4DP),
                       "auc_rounded_4dp_equal": round(g["auc"], 4) == round(auc_ref, 4),
                       "max_abs_score_diff": float(np.abs(s.cpu().numpy() - ref).max()),
                       "cpu_ref_seconds": round(t_cpu, 1)}
        # the same gate with clicks that follow the reference score (AUC ~ 0.8: ranking quality)
        lab = synthetic.logistic_labels(ref, imps.cand_len)
        a_ref = float(np.nanmean(data_ref.impression_aucs(ref, lab, imps.cand_len)))
        a_gpu = evaluation.score_device(r, lab, imps.cand_off())["auc"]
        out[pooler]["logistic_labels"] = {
            "cpu_ref_f32_auc": a_ref, f"gpu_{dtype}_auc": a_gpu, "auc_abs_diff": abs(a_gpu - a_ref),
            "auc_equal_4dp": bool(abs(a_gpu - a_ref) < AUC_4DP),
            "auc_rounded_4dp_equal": round(a_gpu, 4) == round(a_ref, 4),
            "labels": "y ~ Bernoulli(sigmoid(4 (s_ref - q90) / std)), synthetic.logistic_labels"}
        log(f"[bench] AUC gate {pooler}: cpu f32 {auc_ref:.7f} gpu {dtype} {g['auc']:.7f} |d| {diff:.2e}; "
            f"logistic labels cpu {a_ref:.7f} gpu {a_gpu:.7f} |d| {abs(a_gpu - a_ref):.2e} "
            f"(CPU reference {t_cpu:.1f}s)")
        del eng, s, r, ref
        _lib.empty_cache()
    return {"impressions": imps.n_imp, "candidates": imps.n_cand, "by_pooler": out,
            "auc_equal_4dp": all(v["auc_equal_4dp"] and v["logistic_labels"]["auc_equal_4dp"] for v in out.values()),
            "criterion": f"|AUC_gpu - AUC_cpu_ref| < {AUC_4DP} for both label sets (random i.i.d. clicks and "
                         f"logistic-of-reference-score clicks)"}


def load_traffic(pooler: str, dtype: str):
    p = REPO / "profiles" / "pmc_pool_score.json"
    if p.is_file():
        d = json.loads(p.read_text())
        return d.get(f"{pooler}_{dtype}")
    return None


class _DryRunEngine:
    """CPU stand-in for PoolScoreEngine in --dry-run (no GPU): the per-news
    "transform" is a fixed elementwise map (tanh(x) + 0.25 x) and pool + score
    is the latent pooler in float64 (mean of the history rows, F.normalize,
    cosine with the per-vector 1e-8 clamps).  Exercises ShardedTable's real
    partition -> all-gather -> gather_scores path over gloo; the kernels
    themselves are covered by the GPU tests."""

    pooler = "latent"

    def __init__(self, table: torch.Tensor, imps):
        self.hist_src, self.cand_table, self.imps = table, table, imps
        self.dtype, self.device, self.hist_table = table.dtype, table.device, None

    def transform(self, rows=None, out=None, src=None):
        src = self.hist_src if src is None else src
        x = src if rows is None else src[rows]
        res = torch.tanh(x) + 0.25 * x
        if out is None:
            return res
        out.copy_(res)
        return out

    def inv_norms(self):
        pass

    def pool_score(self, want_users=False, scores=None):
        im = self.imps
        tab = self.hist_table.double()
        ho = torch.as_tensor(im.hist_off())
        seg = torch.repeat_interleave(torch.arange(im.n_imp), torch.as_tensor(im.hist_len, dtype=torch.int64))
        u = torch.zeros((im.n_imp, tab.shape[1]), dtype=torch.float64)
        u.index_add_(0, seg, tab[torch.as_tensor(im.hist_idx, dtype=torch.int64)])
        u = u / (ho[1:] - ho[:-1]).clamp_min(1).double()[:, None]
        u = u / u.norm(dim=1, keepdim=True).clamp_min(1e-12)
        e = self.cand_table.double()[torch.as_tensor(im.cand_idx, dtype=torch.int64)]
        cseg = torch.repeat_interleave(torch.arange(im.n_imp), torch.as_tensor(im.cand_len, dtype=torch.int64))
        uc = u[cseg]
        s = (e * uc).sum(1) / uc.norm(dim=1).clamp_min(1e-8) / e.norm(dim=1).clamp_min(1e-8)
        return s, None


def dry_run(args, rank: int, world: int) -> None:
    """--dry-run (CPU, gloo): the multi-rank path without the GPU (what the CPU
    test suite can check): the impression split (strong: one set partitioned by
    cost; weak: a set per rank), the real ShardedTable (each rank transforms its
    1/world shard of the news table, one all-gather), pool + score on the rank's
    range (_DryRunEngine), gather_scores back to impression order, and parity of
    the gathered scores against one process scoring the whole set from the
    whole, unsharded transform; timing max over ranks."""
    from news_recommendation_project_v2_amd.distributed import gather_scores
    n_news, n_imp = synthetic.SHAPES[args.shape]
    n_news = args.dry_run_news or n_news
    n_imp = args.impressions or n_imp
    if args.scaling == "strong":
        full = synthetic.mind_impressions(n_news, n_imp, seed=1234)
        b = partition_by_cost(full.hist_len, full.cand_len, world, 1024 * 2, 1024 * 2)
        mine = full.slice(int(b[rank]), int(b[rank + 1]))
        expected = full.n_cand
    else:  # every rank its own set; rank r's candidates summed over the ranks
        b, full = None, None
        mine = synthetic.mind_impressions(n_news, n_imp, seed=1234 + rank)
        expected = sum(synthetic.mind_impressions(n_news, n_imp, seed=1234 + r).n_cand for r in range(world))
    g = torch.Generator().manual_seed(1234)
    table = torch.randn((n_news, 1024), generator=g, dtype=torch.float32)
    eng = _DryRunEngine(table, mine)
    tab = ShardedTable(eng, rank, world)
    phase("dry_run_step")
    dist.barrier()
    t0 = time.perf_counter()
    local, _ = sharded_step(tab)
    dist.barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    # the all-gathered table equals the unsharded transform on every rank
    whole = _DryRunEngine(table, mine).transform()
    ok_tab = torch.tensor([int(torch.equal(tab.full[:n_news], whole))])
    dist.all_reduce(ok_tab, op=dist.ReduceOp.MIN)
    if args.scaling == "strong":  # scores back in impression order == one process over the whole set
        got = gather_scores(local, world)
        ref_eng = _DryRunEngine(table, full)
        ref_eng.hist_table = whole
        want, _ = ref_eng.pool_score()
        ok_sc = int(got.shape == want.shape and torch.equal(got, want))
    else:
        ref_eng = _DryRunEngine(table, mine)
        ref_eng.hist_table = whole
        want, _ = ref_eng.pool_score()
        ok_sc = int(torch.equal(local, want))
    ok_s = torch.tensor([ok_sc])
    dist.all_reduce(ok_s, op=dist.ReduceOp.MIN)
    c = torch.tensor([mine.n_cand, mine.n_imp], dtype=torch.int64)
    dist.all_reduce(c)
    if rank == 0:
        print(json.dumps({"metric": "scored candidates/sec on MIND-large impressions; AUC parity vs CPU ref",
                          "dry_run": True, "value": None, "n_gpus": world, "scaling": args.scaling,
                          "n_news": n_news, "partition": [int(x) for x in b] if b is not None else None,
                          "candidates_total": int(c[0]),
                          "impressions_total": int(c[1]), "candidates_expected": int(expected),
                          "allgather_ok": bool(ok_tab.item()), "scores_match_single_process": bool(ok_s.item()),
                          "step_s": float(t.item())}), flush=True)
    phase("printed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: stage times and roofline, the other poolers / "
                         "precisions / shapes, training and encoder legs, the CPU baseline and the AUC gates, the "
                         "multi-rank parity checks (the --no-extra / --cpu-* / --no-auc-gate options trim these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's scores as DIR/scores.npy (float32; "
                         "scores_rank<r>.npy per rank at N > 1)")
    ap.add_argument("--pooler", choices=["latent", "final"], default="latent")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--shape", default="mind_large_dev", choices=list(synthetic.SHAPES))
    ap.add_argument("--impressions", type=int, default=0, help="override the shape's impression count")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="strong (default): one MIND-large-dev set partitioned over the ranks (configs[3] as one "
                         "eval job); weak: a full set per rank, the per-GPU work fixed as N grows (an extra at N > 1)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="gloo: test mode, ranks may share one GPU (tables staged through the host)")
    ap.add_argument("--cpu-shape", default="mind_small_dev", choices=list(synthetic.SHAPES))
    ap.add_argument("--cpu-impressions", type=int, default=1000)
    ap.add_argument("--no-cpu-10k", action="store_true", help="skip the 10,000-impression CPU reference sample")
    ap.add_argument("--cpu-10k-seconds", type=float, default=30.0,
                    help="CPU-time cap per pooler for the 10,000-impression sample (impressions done are reported)")
    ap.add_argument("--cpu-seconds", type=float, default=60.0, help="CPU-time cap per pooler and sample")
    ap.add_argument("--no-extra", action="store_true", help="headline config only")
    ap.add_argument("--no-auc-gate", action="store_true",
                    help="skip the full-size (376,471-impression) AUC parity gate vs the CPU reference")
    ap.add_argument("--dry-run", action="store_true", help="CPU-only check of the multi-rank plumbing")
    ap.add_argument("--dry-run-news", type=int, default=8192, help="--dry-run news-table rows (0: the shape's)")
    ap.add_argument("--dist-timeout", type=float, default=600.0,
                    help="seconds: torch.distributed's collective timeout and the RCCL communicator init deadline")
    ap.add_argument("--stall-timeout", type=float, default=300.0,
                    help="N > 1 launcher: kill the ranks when none changes phase for this many seconds")
    ap.add_argument("--wall-timeout", type=float, default=1800.0, help="N > 1 launcher: kill the ranks after this")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:], args.stall_timeout, args.wall_timeout))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"note: WORLD_SIZE={world} but --gpus={args.gpus}; using WORLD_SIZE")
    from datetime import timedelta
    pg_timeout = timedelta(seconds=args.dist_timeout)
    phase("init_process_group")
    if args.dry_run:
        if world > 1:
            dist.init_process_group("gloo", timeout=pg_timeout)
        try:
            dry_run(args, rank, world) if world > 1 else print(json.dumps({"dry_run": True, "n_gpus": 1}))
        finally:
            if world > 1:
                dist.destroy_process_group()
        return

    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    host_reduce = args.backend == "gloo"
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=pg_timeout)
        else:
            dist.init_process_group("gloo", timeout=pg_timeout)
    phase("data")

    n_news, n_imp = synthetic.SHAPES[args.shape]
    n_imp = args.impressions or n_imp
    t0 = time.time()
    es = 2 if args.dtype == "bf16" else 4
    kw = 2 if args.pooler == "final" else 1
    if args.scaling == "strong":
        full = synthetic.mind_impressions(n_news, n_imp, seed=1234)
        bounds = partition_by_cost(full.hist_len, full.cand_len, world, kw * 1024 * es, 1024 * es)
        imps = full.slice(int(bounds[rank]), int(bounds[rank + 1]))
        total_cand = full.n_cand
    else:
        full, bounds = None, None
        imps = synthetic.mind_impressions(n_news, n_imp, seed=1234 + rank)
        total_cand = None
    table = news_table(n_news, dev)
    log(f"[bench] data ready in {time.time() - t0:.1f}s: N={n_news} I={imps.n_imp} C={imps.n_cand} "
        f"H={imps.n_hist} (rank 0 of {world}, {args.scaling} scaling)")

    phase("headline")
    head = Run(args.pooler, args.dtype, imps, table, dev, rank, world)
    last = []
    dt = timed(head.step, args.steps, args.warmup, world, dev, host_reduce, keep=last)
    phase("headline_done")
    ms = dt / args.steps * 1e3
    if total_cand is None:  # weak: every rank's own set
        c = torch.tensor([imps.n_cand], dtype=torch.int64, device="cpu" if host_reduce else dev)
        if world > 1:
            dist.all_reduce(c)
        total_cand = int(c.item())
    value = total_cand / (dt / args.steps)
    dumped = None
    if args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, {"scores" if world == 1 else f"scores_rank{rank}": last[0][0]})
    del last
    line = {
        "metric": "scored candidates/sec on MIND-large impressions; AUC parity vs CPU ref",
        "value": round(value, 1),
        "unit": "scored candidates/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms, 3),
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic (seeded MIND-large-dev-shaped impressions, N(0,1) news table, deterministic "
                "random-init pooler weights)",
        "config": {"workload": f"{args.shape} eval, {args.pooler} pooler: per-news transform + pool + "
                               f"cosine score", "pooler": args.pooler, "n_news": n_news,
                   "impressions": n_imp if args.scaling == "strong" else n_imp * world,
                   "parallelism": f"impressions x{world} ({args.scaling}), news-table transform sharded + "
                                  f"all-gather ({args.backend})"},
        "full": args.full,
    }
    if dumped is not None:
        line["dumped_outputs"] = {"dir": args.dump_outputs, "elements": dumped}
    if not args.full:  # the headline only
        log(f"[bench] {args.pooler}/{args.dtype} x{world}: {ms:.3f} ms/step, {value:.3e} cand/s")
        if rank == 0:
            print(json.dumps(line), flush=True)
        phase("printed")
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    stages = head.stage_times()
    bytes_ps = ps_bytes(imps, args.pooler, es)
    achieved = bytes_ps / (stages[2] * 1e-3) / 1e9
    log(f"[bench] {args.pooler}/{args.dtype} x{world}: {ms:.3f} ms/step, {value:.3e} cand/s; stages ms "
        f"transform+gather={stages[0]:.3f} invnorm={stages[1]:.3f} pool_score={stages[2]:.3f}")

    tx_rank = tx_flops(head.tab.rows, args.pooler)  # this rank's shard of the transform
    extra = {"stage_ms": {"transform_allgather": round(stages[0], 3), "inv_norm": round(stages[1], 4),
                          "pool_score": round(stages[2], 3)},
             # the transform's own interval (without the all-gather at N > 1)
             "transform_tflops": round(tx_rank / (head.split_ms[0] * 1e-3) / 1e12, 1),
             "transform_peak_frac": round(tx_rank / (head.split_ms[0] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[args.dtype],
                                          3),
             "step_roofline_frac": round((bytes_ps / (HBM_PEAK_GBS * 1e9)
                                          + tx_rank / (MFMA_PEAK_TFLOPS[args.dtype] * 1e12)) / (ms * 1e-3), 4),
             "n_news": n_news, "impressions_rank0": imps.n_imp, "candidates_rank0": imps.n_cand,
             "history_slots_rank0": imps.n_hist, "candidates_total": total_cand}
    if bounds is not None and world > 1:
        extra["partition"] = [int(x) for x in bounds]
    if world > 1:
        # load balance of the impression split: every rank's pool_score time (HIP events)
        extra.update(rank_balance(stages[2], imps, dev, host_reduce, world))
    if world > 1:
        # phase A / phase B separately: the shard's transform, then the RCCL all-gather
        # (events on the current stream, which waits for RCCL's stream at the end of the call)
        t_ms, g_ms = head.split_ms
        gb_in = head.tab.gather_bytes_in
        extra["transform_ms"] = round(float(t_ms), 3)
        extra["allgather_ms"] = round(float(g_ms), 3)
        extra["allgather_bytes_in_per_gpu"] = int(gb_in)
        extra["allgather_GBs_in_per_gpu"] = round(gb_in / (g_ms * 1e-3) / 1e9, 1) if g_ms > 0 else None
        extra["transform_chunks"] = head.tab.chunks

    dist_info = None
    if world > 1:
        # what actually ran: world size / backend as initialised, RCCL version, the ranks
        # that joined, per-rank float64 parity of 200 sampled impressions, table identity
        red = "cpu" if host_reduce else dev
        err = rank_parity(head)
        ok_t = torch.tensor([1 if err <= 2e-5 else 0, 1], dtype=torch.int64, device=red)
        dist.all_reduce(ok_t)  # [ranks with parity ok, ranks]
        err_t = torch.tensor([err], dtype=torch.float64, device=red)
        dist.all_reduce(err_t, op=dist.ReduceOp.MAX)
        dg = table_digest(head.tab.full)
        dmin = torch.tensor([dg], dtype=torch.int64, device=red)
        dmax = dmin.clone()
        dist.all_reduce(dmin, op=dist.ReduceOp.MIN)
        dist.all_reduce(dmax, op=dist.ReduceOp.MAX)
        try:
            rv = ".".join(map(str, torch.cuda.nccl.version())) if dist.get_backend() == "nccl" else None
        except Exception:  # noqa: BLE001
            rv = None
        dist_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "rccl_version": rv,
                     "rccl_ranks": int(ok_t[1].item()) if dist.get_backend() == "nccl" else 0,
                     "parity_ok": bool(int(ok_t[0].item()) == world), "parity_ranks_ok": int(ok_t[0].item()),
                     "parity_max_abs_err": float(err_t.item()),
                     "parity_check": "200 sampled impressions per rank vs a float64 re-pool of the rank's own "
                                     "all-gathered table, |err| <= 2e-5",
                     "table_identical_on_all_ranks": bool(int(dmin.item()) == int(dmax.item()))}
        log(f"[bench] ranks: {json.dumps(dist_info)}")

    if world > 1 and not args.no_extra and args.backend == "nccl":
        # the same all-gather through the library's own RCCL communicator (nr_comm_init /
        # nr_allgather): its step time and its table against torch's bit for bit
        from news_recommendation_project_v2_amd.distributed import NrComm
        comm = None
        phase("nr_comm_init")
        try:
            ref_table = head.tab.full.clone()
            comm = NrComm(rank, world, timeout_s=args.dist_timeout)
            phase("nr_allgather")
            r = Run(args.pooler, args.dtype, imps, table, dev, rank, world)
            r.tab = ShardedTable(r.eng, rank, world, comm=comm)
            r.tab.timing = True
            d = timed(r.step, max(3, args.steps // 2), 2, world, dev, host_reduce) / max(3, args.steps // 2)
            r.tab.build()
            torch.cuda.synchronize()
            t_ms, g_ms = r.tab.last_ms()
            same = torch.tensor([int(torch.equal(r.tab.full, ref_table))], device=dev)
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
            extra["nr_allgather"] = {"ms_per_step": round(d * 1e3, 3), "value": round(total_cand / d, 1),
                                     "allgather_ms": round(float(g_ms), 3),
                                     "table_bit_identical_to_torch": bool(same.item())}
            r.tab.timing = False
            del r, ref_table
        except Exception as e:  # noqa: BLE001  (an extra: report, never fail the headline)
            extra["nr_allgather"] = {"error": repr(e)[:300]}
        finally:
            if comm is not None:
                comm.close()
            _lib.empty_cache()

    if world > 1 and not args.no_extra:
        phase("overlapped_build")
        # the opt-in overlapped build (2 chunks, each chunk's all-gather beside the next
        # chunk's transform): its step time, and its table against the default's bit for bit
        ref_table = head.tab.full.clone()
        r = Run(args.pooler, args.dtype, imps, table, dev, rank, world, chunks="auto")
        if r.tab.chunks > 1:
            d = timed(r.step, max(3, args.steps // 2), 2, world, dev, host_reduce) / max(3, args.steps // 2)
            same = torch.tensor([int(torch.equal(r.tab.full, ref_table))], device="cpu" if host_reduce else dev)
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
            extra["overlapped_build"] = {"chunks": r.tab.chunks, "ms_per_step": round(d * 1e3, 3),
                                         "value": round(total_cand / d, 1),
                                         "table_bit_identical": bool(same.item())}
        del r, ref_table
        _lib.empty_cache()
        # the other scaling mode as an extra
        phase("other_scaling")
        if args.scaling == "strong":  # every rank its own full MIND-large-dev-sized set
            other = synthetic.mind_impressions(n_news, n_imp, seed=1234 + rank)
        else:  # configs[3] as ONE eval job: the rank-0 set partitioned over the ranks
            one = synthetic.mind_impressions(n_news, n_imp, seed=1234)
            ob = partition_by_cost(one.hist_len, one.cand_len, world, kw * 1024 * es, 1024 * es)
            other = one.slice(int(ob[rank]), int(ob[rank + 1]))
            del one
        r = Run(args.pooler, args.dtype, other, table, dev, rank, world)
        d = timed(r.step, max(3, args.steps // 2), 2, world, dev, host_reduce) / max(3, args.steps // 2)
        c = torch.tensor([other.n_cand], dtype=torch.int64, device="cpu" if host_reduce else dev)
        dist.all_reduce(c)
        key = "weak_scaling" if args.scaling == "strong" else "strong_scaling"
        extra[key] = {"value": round(int(c.item()) / d, 1), "ms_per_step": round(d * 1e3, 3),
                      "impressions_per_gpu_rank0": other.n_imp}
        other_parity = rank_parity(r)
        pt = torch.tensor([other_parity], dtype=torch.float64, device="cpu" if host_reduce else dev)
        dist.all_reduce(pt, op=dist.ReduceOp.MAX)
        extra[key]["parity_max_abs_err"] = float(pt.item())
        extra[key]["parity_ok"] = bool(float(pt.item()) <= 2e-5)
        del r, other
        _lib.empty_cache()
        # configs[3]'s strong scaling on the MIND-large *test* shape: 2.37 M impressions
        # over 121 k news keep ~300 k impressions per GPU at N = 8
        phase("mind_large_test")
        tn, ti = synthetic.SHAPES["mind_large_test"]
        one = synthetic.mind_impressions(tn, ti, seed=1234)
        ob = partition_by_cost(one.hist_len, one.cand_len, world, kw * 1024 * es, 1024 * es)
        part = one.slice(int(ob[rank]), int(ob[rank + 1]))
        n_total = one.n_cand
        del one
        tb = news_table(tn, dev)
        r = Run(args.pooler, args.dtype, part, tb, dev, rank, world)
        d = timed(r.step, max(3, args.steps // 2), 2, world, dev, host_reduce) / max(3, args.steps // 2)
        st = r.stage_times(2)
        extra["strong_scaling_mind_large_test"] = {
            "n_news": tn, "impressions": ti, "candidates": int(n_total), "value": round(n_total / d, 1),
            "ms_per_step": round(d * 1e3, 3), "partition": [int(x) for x in ob],
            **rank_balance(st[2], part, dev, host_reduce, world)}
        del r, tb, part
        _lib.empty_cache()

    if world == 1 and not args.no_extra:
        for pooler, dtype in [(args.pooler, "fp32" if args.dtype == "bf16" else "bf16"),
                              ("final" if args.pooler == "latent" else "latent", args.dtype)]:
            r = Run(pooler, dtype, imps, table, dev, rank, world)
            k = max(3, args.steps // 2)
            d = timed(r.step, k, 2, world, dev, host_reduce) / k
            st = r.stage_times(2)
            e2 = 2 if dtype == "bf16" else 4
            extra[f"{pooler}_{dtype}"] = {
                "value": round(total_cand / d, 1), "ms_per_step": round(d * 1e3, 3),
                "pool_score_ms": round(st[2], 3), "transform_ms": round(st[0], 3),
                "pool_score_GBs": round(ps_bytes(imps, pooler, e2) / (st[2] * 1e-3) / 1e9, 1)}
            if pooler == args.pooler:
                extra["auc"] = {args.dtype: auc_of(head), dtype: auc_of(r)}
                extra["auc"]["abs_diff"] = abs(extra["auc"][args.dtype] - extra["auc"][dtype])
            del r
            _lib.empty_cache()
        # throughput on the MIND-large *test* shape and cache sensitivity under Zipf(1.1) id popularity
        for tag, shape, zipf in [("mind_large_test", "mind_large_test", None), ("zipf1.1", args.shape, 1.1)]:
            nn_, ni_ = synthetic.SHAPES[shape]
            im = synthetic.mind_impressions(nn_, ni_, seed=1234, zipf=zipf)
            tb = table if nn_ == n_news else news_table(nn_, dev)
            r = Run(args.pooler, args.dtype, im, tb, dev, rank, world)
            d = timed(r.step, 3, 1, world, dev, host_reduce) / 3
            st = r.stage_times(2)
            extra[tag] = {"n_news": nn_, "impressions": im.n_imp, "candidates": im.n_cand,
                          "value": round(im.n_cand / d, 1), "ms_per_step": round(d * 1e3, 3),
                          "pool_score_ms": round(st[2], 3),
                          "pool_score_GBs": round(ps_bytes(im, args.pooler, es) / (st[2] * 1e-3) / 1e9, 1)}
            del r, tb, im
            _lib.empty_cache()
        # MIND's user structure: ~256 k users' histories repeated over 376 k impressions
        # (synthetic.MIND_LARGE_DEV_USERS, an assumption); the engine then pools each
        # distinct history once (automatic at >= 15 % repeats), the fused pass beside it
        im = synthetic.mind_impressions(n_news, n_imp, seed=1234, users=synthetic.MIND_LARGE_DEV_USERS)
        sh = {"users": synthetic.MIND_LARGE_DEV_USERS, "impressions": im.n_imp, "candidates": im.n_cand}
        for tag, mode in (("distinct_histories_pooled_once", None), ("fused_per_impression", False)):
            r = Run(args.pooler, args.dtype, im, table, dev, rank, world)
            r.eng.load_impressions(im.hist_idx, im.hist_len, im.cand_idx, im.cand_len, dedupe=mode)
            d = timed(r.step, 3, 1, world, dev, host_reduce) / 3
            sh[tag] = {"value": round(im.n_cand / d, 1), "ms_per_step": round(d * 1e3, 3)}
            sh["repeated_history_share"] = round(r.eng.shared_history_share, 4) if mode is None else \
                sh.get("repeated_history_share")
            del r
            _lib.empty_cache()
        extra["shared_histories"] = sh
        del im
        extra["metrics_ms"] = round(metrics_ms(head), 3)
        extra["host_parse_A1"] = host_parse_leg(n_news)
        if args.dtype == "bf16":
            extra["transform_vs_hipblaslt"] = hipblaslt_yardstick(args.pooler, n_news, head.split_ms[0], dev)
        # PCIe-side costs (never part of `value`): load_impressions (its host-side range
        # checks and offsets + the copies), the bare copies of the same arrays, and the
        # score download pinned (the API path, data_model_helper._host) and pageable
        from news_recommendation_project_v2_amd import data_model_helper as dmh
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        head.eng.load_impressions(imps.hist_idx, imps.hist_len, imps.cand_idx, imps.cand_len, dedupe=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host_arrays = [np.ascontiguousarray(imps.hist_idx, dtype=np.int32), np.ascontiguousarray(imps.cand_idx,
                                                                                                 dtype=np.int32),
                       imps.hist_off(), imps.cand_off()]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for a_ in host_arrays:
            torch.as_tensor(a_).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        dmh._host(head.scores)
        t4 = time.perf_counter()
        head.scores.cpu()
        t5 = time.perf_counter()
        ib = int(sum(a_.nbytes for a_ in host_arrays))
        sb = int(4 * imps.n_cand)
        extra["pcie_ms"] = {"load_impressions": round((t1 - t0) * 1e3, 3), "h2d_index_arrays": round((t3 - t2) * 1e3, 3),
                            "h2d_index_GBs": round(ib / (t3 - t2) / 1e9, 1),
                            "d2h_scores_pinned": round((t4 - t3) * 1e3, 3),
                            "d2h_scores_pinned_GBs": round(sb / (t4 - t3) / 1e9, 1),
                            "d2h_scores_pageable": round((t5 - t4) * 1e3, 3),
                            "d2h_scores_pageable_GBs": round(sb / (t5 - t4) / 1e9, 1),
                            "index_bytes": ib, "score_bytes": sb}
        log("[bench] drop-in API end to end ...")
        extra["api_end_to_end_ms"] = api_end_to_end(args.pooler, args.dtype, imps, table.cpu(), dev)
        log(f"[bench] API end to end: {json.dumps(extra['api_end_to_end_ms'])}")
        extra["train_bf16_config5"] = train_step_ms(dev)
        extra["train_bf16_config5_latent"] = train_step_ms(dev, pooler="latent")
        extra["config2_mind_small_f32"] = config2_leg(dev)
        extra["encoder_bf16_config3"] = encoder_bf16_leg(dev)

    cpu = None
    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        log("[bench] timing the CPU reference restatement ...")
        cpu, extra["auc_vs_cpu_ref"] = cpu_leg(args, dev)
        log(f"[bench] AUC vs CPU reference: {json.dumps(extra['auc_vs_cpu_ref'])}")
    gate = None
    if rank == 0 and world == 1 and not args.no_auc_gate and args.cpu_seconds > 0:
        log("[bench] full-size AUC gate (all MIND-large-dev impressions, both poolers) ...")
        gate = auc_gate_full(dev, dtype=args.dtype)

    if rank == 0:
        out = {
            **line,
            "roofline": {"bound": "hbm", "kernel": "pool_score_kernel",
                         "bound_detail": "random-row gather of ~150-300 MB tables (L2 miss, served by HBM + "
                                         "Infinity Cache); 8 TB/s is the HBM spec, the gather ceiling is the "
                                         "guide's measured 7.4-7.9 TB/s",
                         "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "gather_ceiling": GATHER_CEILING_GBS,
                         "frac_vs_gather_ceiling": round(achieved / GATHER_CEILING_GBS, 4),
                         "traffic": load_traffic(args.pooler, args.dtype) if world == 1 else None,
                         "algorithmic_bytes_per_launch": bytes_ps, "avg_launch_ms": round(stages[2], 4)},
            # both scaling readings at the top level: configs[3] is ONE MIND-large eval
            # partitioned over the ranks (strong); weak = a full set per rank
            "configs3_value": (round(value, 1) if world == 1 or args.scaling == "strong" else
                               extra.get("strong_scaling", {}).get("value")),
            "weak_scaling_value": (round(value, 1) if world == 1 or args.scaling == "weak" else
                                   extra.get("weak_scaling", {}).get("value")),
            "distributed": dist_info,
            "cpu_baseline": cpu,
            # the north star's AUC clause on the headline workload itself (configs[2] size)
            "auc_parity": gate,
            "extra": extra,
        }
        print(json.dumps(out), flush=True)
    phase("printed")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
