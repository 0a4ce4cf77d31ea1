"""What the mean teacher costs per step.  bench.py's workload and timing method (captured iteration, W untimed replays, then K replays between
two synchronizes) on two steps of one process -- one without, one with a teacher -- measured in ALTERNATION for R rounds, so that drift of the
device hits both alike; and the optimizer launch alone (chap_sgd_step against chap_sgd_ema_step on the same buffers, HIP events around a
captured graph of back-to-back launches).  One JSON line; --out writes it to a file as well.

    python tools/mean_teacher_cost.py [--config 2d|3d] [--dtype bf16|fp32] [--steps 30] [--warmup 5] [--rounds 5] [--out FILE]
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

from chap_amd.networks import DualDecoder, DualDecoder3d        # noqa: E402
from chap_amd.synthetic import synthetic_batch, synthetic_batch_3d      # noqa: E402
from chap_amd.train import ChapStep, build_teacher              # noqa: E402

DEV = torch.device("cuda", 0)


def build(cfg, dtype, B, sp, teacher):
    torch.manual_seed(1337)
    np.random.seed(1337)
    if cfg == "3d":
        make = lambda: DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True).to(DEV)       # noqa: E731
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2)
    else:
        make = lambda: DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)                                              # noqa: E731
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1)
    model = make().train().set_compute_dtype(dtype)
    t = build_teacher(make).eval() if teacher else None
    return ChapStep(model, args, teacher=t)


def timed(step, vol, lab, steps, warmup):
    for _ in range(warmup):
        step.replay(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.replay(vol, lab)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def kernel_us(step, reps=20):
    """One optimizer launch, from a captured graph of `reps` of them (gradients are zero after the first: the traffic is the same)."""
    for _ in range(3):
        step.opt.step(grad2=step.grad2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            step.opt.step(grad2=step.grad2)
    g.replay()
    best = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="2d", choices=["2d", "3d"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d3 = a.config == "3d"
    B, sp = (4, (112, 112, 80)) if d3 else (24, (256, 256))
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    vol, lab = (synthetic_batch_3d if d3 else synthetic_batch)(1337, B // 2, B - B // 2, *sp)
    vol, lab = vol.to(DEV), lab.to(DEV)
    steps = {}
    for name, teacher in (("off", False), ("on", True)):
        steps[name] = build(a.config, dtype, B, sp, teacher)
        steps[name].capture(vol, lab, warmup=2)
    ms = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name in ("off", "on"):
            ms[name].append(round(timed(steps[name], vol, lab, a.steps, a.warmup), 4))
    n = steps["off"].opt.mom.numel()
    k_off, k_on = kernel_us(steps["off"]), kernel_us(steps["on"])
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "mean_teacher_cost", "config": a.config, "dtype": a.dtype, "batch": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
            "ms_per_step_off": ms["off"], "ms_per_step_on": ms["on"], "median_off": round(med["off"], 4), "median_on": round(med["on"], 4),
            "spread_off": round(max(ms["off"]) - min(ms["off"]), 4), "spread_on": round(max(ms["on"]) - min(ms["on"]), 4),
            "step_delta_ms": round(med["on"] - med["off"], 4), "flat_parameter_floats": n,
            "optimizer_kernel_us": {"chap_sgd_step": round(k_off, 2), "chap_sgd_ema_step": round(k_on, 2)},
            "optimizer_bytes": {"chap_sgd_step": 8 * 4 * n, "chap_sgd_ema_step": 10 * 4 * n}}       # p, m, g, g2 read + written; + ema read + written
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
