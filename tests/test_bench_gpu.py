"""bench.py's plain run (-m gpu): the headline line only, `--steps` timed steps, and `--dump-outputs` writing what the last
timed step returned (bench.dump_outputs)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
                        "--size", "128", "--dump-outputs", str(tmp_path)], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    for key in ("kernel_ms", "roofline", "h1_step", "allreduce_model", "stage1_step", "configs", "cpu_baseline"):
        assert key not in out, key                               # measured by --full only
    files = sorted(tmp_path.glob("*.npy"))
    assert {f.stem for f in files} == {"probs", "mean", "std", "speeds", "loss", "grad_sample", "grad_norms"}
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    a = {f.stem: np.load(f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a["probs"].shape == (8, 4) and a["mean"].shape == a["std"].shape == (8, 4, 2) and a["speeds"].shape == (8, 4, 1)
    np.testing.assert_allclose(a["probs"].sum(1), 1.0, atol=1e-3)
    assert abs(float(a["loss"]) - out["loss"]) <= 1e-5                # the line's loss is the last timed step's, to 5 places
    assert a["grad_sample"].shape == (1 << 22,) and a["grad_norms"].shape == (356,) and (a["grad_norms"] > 0).any()
