"""What the training monitor costs per step.  bench.py's default 2D and 3D bf16 workloads and its timing method (captured iteration, W untimed
replays, then K replays between two synchronizes) on two steps of one process -- one without, one with a StepMonitor -- measured in
ALTERNATION for R rounds, so that drift of the device hits both alike; and the three kernels alone, at the shapes the step gives them (HIP
events around a captured graph of back-to-back launches).  The monitored step's ring is read once per round, as train() reads it once per
validation interval.  --out writes the result as one JSON document: {"2d": {...}, "3d": {...}}.

    python tools/monitor_cost.py [--configs 2d 3d] [--steps 200] [--warmup 10] [--rounds 3] [--out profiles/monitor_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chap_amd import ops                                         # noqa: E402
from chap_amd.monitor import StepMonitor                         # noqa: E402
from chap_amd.networks import DualDecoder, DualDecoder3d        # noqa: E402
from chap_amd.synthetic import synthetic_batch, synthetic_batch_3d      # noqa: E402
from chap_amd.train import ChapStep                              # noqa: E402

DEV = torch.device("cuda", 0)


def build(cfg, dtype, B, monitor):
    torch.manual_seed(1337)
    np.random.seed(1337)
    if cfg == "3d":
        model, C = DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True).to(DEV), 2
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2)
    else:
        model, C = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV), 4
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1)
    model = model.train().set_compute_dtype(dtype)
    return ChapStep(model, args, monitor=StepMonitor(C, ring=256, device=DEV)) if monitor else ChapStep(model, args)


def timed(step, vol, lab, steps, warmup):
    for _ in range(warmup):
        step.replay(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.replay(vol, lab)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def graph_us(launch, reps=20):
    """One launch, from a captured graph of `reps` of them."""
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            launch()
    g.replay()
    took = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        took.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(took)


def kernels_us(C, U, sp):
    """The three launches at the step's shapes: U unlabelled samples, n_first = 0."""
    g = torch.Generator().manual_seed(3)
    l1, l2 = (torch.randn((U, C) + tuple(sp), generator=g).to(DEV) for _ in range(2))
    lab = torch.randint(0, C, (U,) + tuple(sp), generator=g).to(DEV)
    m1, m2 = l1.argmax(1), l2.argmax(1)
    mon = StepMonitor(C, ring=8, device=DEV)
    slot_iter = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    scal = torch.zeros(13, dtype=torch.float32, device=DEV)
    px = U * int(np.prod(sp))
    return {"chap_monitor_accumulate": round(graph_us(lambda: ops.monitor_accumulate(l1, l2, lab, mon.ws, 0)), 2),
            "chap_monitor_accumulate_labels": round(graph_us(lambda: ops.monitor_accumulate_labels(m1, m2, lab, mon.ws, 0, C)), 2),
            "chap_monitor_finalize": round(graph_us(lambda: ops.monitor_finalize(mon.ws, mon.ring, slot_iter, C, [scal[i:i + 1] for i in range(13)])), 2),
            "bytes": {"chap_monitor_accumulate": px * (2 * C * 4 + 8), "chap_monitor_accumulate_labels": px * 24}}


def one(cfg, a):
    d3 = cfg == "3d"
    B, sp = (4, (112, 112, 80)) if d3 else (24, (256, 256))
    vol, lab = (synthetic_batch_3d if d3 else synthetic_batch)(1337, B // 2, B - B // 2, *sp)
    vol, lab = vol.to(DEV), lab.to(DEV)
    steps = {}
    for name, monitor in (("off", False), ("on", True)):
        steps[name] = build(cfg, torch.bfloat16, B, monitor)
        steps[name].capture(vol, lab, warmup=2)
    ms, rows = {"off": [], "on": []}, 0
    for _ in range(a.rounds):
        for name in ("off", "on"):
            ms[name].append(round(timed(steps[name], vol, lab, a.steps, a.warmup), 4))
        r = steps["on"].monitor.read()
        rows += len(r["iteration"]) + r["dropped"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"tool": "monitor_cost", "config": cfg, "dtype": "bf16", "batch": B, "size": list(sp), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
            "ms_per_step_off": ms["off"], "ms_per_step_on": ms["on"], "median_off": round(med["off"], 4), "median_on": round(med["on"], 4),
            "spread_off": round(max(ms["off"]) - min(ms["off"]), 4), "spread_on": round(max(ms["on"]) - min(ms["on"]), 4),
            "step_delta_ms": round(med["on"] - med["off"], 4), "rows_accounted_for": rows,
            "kernel_us": kernels_us(2 if d3 else 4, B - B // 2, sp)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["2d", "3d"], choices=["2d", "3d"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {}
    for cfg in a.configs:
        doc[cfg] = one(cfg, a)
        print(json.dumps(doc[cfg]), flush=True)
        if a.out:       # (after every configuration: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
