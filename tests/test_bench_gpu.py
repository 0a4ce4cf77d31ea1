"""A plain bench.py run end to end on a small configuration: exactly --steps timed steps, the headline fields of the line and
nothing of what --full measures, and --dump-outputs writing the same arrays on two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in argv], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_repeatable_dump(tmp_path):
    runs = []
    for d in ("a", "b"):
        line = _bench("--gpus", 1, "--steps", 3, "--warmup", 1, "--batch", 8, "--size", 64, "--dump-outputs", tmp_path / d)
        runs.append(line)
    for line in runs:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
        assert line["unit"] == "volumes/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["metric"].startswith("training volumes/sec") and line["config"]["losses_finite"]
        assert abs(line["value"] - 8 * 1000.0 / line["ms_per_step"]) / line["value"] < 1e-2
        assert not {"roofline", "cpu_baseline", "extra_configs"} & set(line)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b")))
    assert "vat_loss.npy" in names and "mix_losses.0.npy" in names and any(n.startswith("model.") for n in names)
    for n in names:
        a, b = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n              # the same inputs on every run, and the iteration is bit-reproducible
