"""bench.py's output side without a GPU: the options of a plain and a --full run, and what --dump-outputs writes
(names, dtypes, the 64 MB limit)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _outputs():
    g = torch.Generator().manual_seed(0)
    out = {"mix_losses": [torch.rand(3, generator=g) for _ in range(4)], "vat_loss": torch.rand(1, generator=g).double(),
           "consistency_weight": 0.5}
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.BatchNorm1d(32))
    return out, model


def test_dump_outputs_writes_losses_and_model_state(tmp_path):
    out, model = _outputs()
    bench.dump_outputs(str(tmp_path), out, model)
    names = sorted(os.listdir(str(tmp_path)))
    assert names == sorted(["mix_losses.%d.npy" % i for i in range(4)] + ["vat_loss.npy"] +
                           ["model.%s.npy" % k for k in model.state_dict()])
    for i, t in enumerate(out["mix_losses"]):
        a = np.load(str(tmp_path / ("mix_losses.%d.npy" % i)))
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())
    assert np.load(str(tmp_path / "vat_loss.npy")).dtype == np.float32
    w = np.load(str(tmp_path / "model.0.weight.npy"))
    assert w.dtype == np.float32 and np.array_equal(w, model[0].weight.detach().numpy())
    nbt = np.load(str(tmp_path / "model.1.num_batches_tracked.npy"))
    assert nbt.dtype == np.float64 and nbt.shape == ()


def test_dump_outputs_refuses_more_than_the_budget(tmp_path, monkeypatch):
    out, model = _outputs()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)            # the Linear weight alone is 8 KB
    with pytest.raises(SystemExit, match="64 MB"):
        bench.dump_outputs(str(tmp_path / "d"), out, model)
    assert not os.path.exists(str(tmp_path / "d"))
