"""A plain bench.py run (no --full) times the requested steps and prints the
headline line only; --dump-outputs writes the last timed step's scores."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_scores(gpu_device, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--impressions", "2000", "--dump-outputs", str(tmp_path / "out")],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["full"] is False
    assert res["unit"] == "scored candidates/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["ms_per_step"] > 0 and res["value"] > 0
    # only the headline: nothing that takes runs of its own
    assert not {"roofline", "extra", "cpu_baseline", "auc_parity", "distributed"} & set(res)
    assert [f.name for f in (tmp_path / "out").iterdir()] == ["scores.npy"]
    s = np.load(tmp_path / "out" / "scores.npy")
    assert s.dtype == np.float32 and s.ndim == 1 and s.size == res["dumped_outputs"]["elements"]["scores"]
    # value = candidates / step time, and every candidate of the set has a cosine score
    assert abs(res["value"] - s.size / (res["ms_per_step"] * 1e-3)) <= 2e-3 * res["value"]
    assert np.isfinite(s).all() and np.abs(s).max() <= 1.0 + 1e-3 and s.std() > 0
