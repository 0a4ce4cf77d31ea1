"""What the fused Adam / AdamW costs against the fused SGD, in the manner of tools/guard_cost.py.

Whole step: bench.py's default 2D and 3D bf16 workloads and its timing method (captured iteration, W untimed replays, then K replays between
two synchronizes), one step with optimizer='sgd' and one with optimizer='adamw' in the same process, measured in ALTERNATION for R rounds so
that drift of the device hits both alike; medians with their spread [min, max].  A difference inside the spread is no difference.

Stand-alone: chap_sgd_step, chap_adam_step without and with the mean teacher's average, and chap_adam_tick at the configuration's parameter
count, alternating for KERNEL_ROUNDS rounds (HIP events around a captured graph of back-to-back launches; zero_grad off and lr 0, so every
launch reads what the first one read), with the achieved bytes/s from the bytes these launches move.  With zero_grad off both buckets are
read (4 B each) and nothing is zeroed: chap_sgd_step moves parameter and momentum read and written (16) + 8 = 24 B per parameter, as
tools/guard_cost.py counts it; chap_adam_step parameter and two moments (24) + 8 = 32; with the average 40.  (The nominal 24 / 32 / 40 of the
training step count one bucket read and zeroed instead; its second bucket adds 8.)  --out writes one JSON document: {"2d": {...}, "3d": {...}}.

    python tools/time_optimizer.py [--configs 2d 3d] [--steps 200] [--warmup 10] [--rounds 4] [--out profiles/adam_cost.json]
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
from chap_amd.networks import DualDecoder, DualDecoder3d         # noqa: E402
from chap_amd.synthetic import synthetic_batch, synthetic_batch_3d      # noqa: E402
from chap_amd.train import ChapStep                              # noqa: E402

DEV = torch.device("cuda", 0)
KERNEL_ROUNDS = 5                   # rounds of the stand-alone timings, whatever --rounds says for the whole step
ADAMW = dict(optimizer="adamw", base_lr=1e-3, weight_decay=1e-2)


def build(cfg, B, extra):
    torch.manual_seed(1337)
    np.random.seed(1337)
    if cfg == "3d":
        model = DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True).to(DEV)
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2)
    else:
        model = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1)
    return ChapStep(model.train().set_compute_dtype(torch.bfloat16), dict(args, **extra))


def timed(step, vol, lab, steps, warmup):
    for _ in range(warmup):
        step.replay(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.replay(vol, lab)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def graph_of(launch, reps):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            launch()
    g.replay()
    torch.cuda.synchronize()
    return g


def graph_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernels(n, reps=20):
    gen = torch.Generator().manual_seed(3)
    p, g1, g2, m, v, e = (torch.randn(n, generator=gen).to(DEV) * s for s in (1.0, 1e-3, 1e-3, 1e-3, 0.0, 1.0))
    v.add_(1e-6)
    lr = torch.zeros(1, device=DEV)             # nothing moves: every launch sees the first one's values
    coef = torch.tensor([1.0, 0.0], device=DEV)
    state = torch.zeros(ops.ADAM_STATE_WORDS, dtype=torch.int32, device=DEV)
    launches = {
        "chap_sgd_step": (lambda: ops.sgd_step(p, g1, m, lr, 0.9, 1e-4, 1.0, False, g2), 16 + 8),
        "chap_adam_step": (lambda: ops.adam_step(p, g1, m, v, state, 0.9, 0.999, 1e-8, 1e-2, True, None, None, None, 1.0, False, g2), 24 + 8),
        "chap_adam_step_ema": (lambda: ops.adam_step(p, g1, m, v, state, 0.9, 0.999, 1e-8, 1e-2, True, e, coef, None, 1.0, False, g2), 32 + 8),
        "chap_adam_tick": (lambda: ops.adam_tick(state, lr, 0.9, 0.999, 1e-2, True), 0),
    }
    ops.adam_tick(state, lr, 0.9, 0.999, 1e-2, True)
    graphs = {k: graph_of(fn, reps) for k, (fn, _) in launches.items()}
    us = {k: [] for k in launches}
    for _ in range(KERNEL_ROUNDS):
        for k in launches:
            us[k].append(graph_us(graphs[k], reps))
    out = {"n": n, "launches_per_graph": reps, "rounds": KERNEL_ROUNDS}
    for k, (_, bpp) in launches.items():
        med = statistics.median(us[k])
        out[k] = {"us": round(med, 2), "us_min": round(min(us[k]), 2), "us_max": round(max(us[k]), 2), "bytes_per_parameter": bpp}
        if bpp:
            out[k]["GB_per_s"] = round(bpp * n / med * 1e-3, 1)
    return out


def one(cfg, a):
    d3 = cfg == "3d"
    B, sp = (4, (112, 112, 80)) if d3 else (24, (256, 256))
    vol, lab = (synthetic_batch_3d if d3 else synthetic_batch)(1337, B // 2, B - B // 2, *sp)
    vol, lab = vol.to(DEV), lab.to(DEV)
    variants = [("sgd", dict(optimizer="sgd")), ("adamw", ADAMW)]
    steps = {}
    for name, extra in variants:
        steps[name] = build(cfg, B, extra)
        steps[name].capture(vol, lab, warmup=2)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, _ in variants:
            ms[name].append(round(timed(steps[name], vol, lab, a.steps, a.warmup), 4))
    n = steps["sgd"].grad_both.numel() // 2
    out = {"tool": "time_optimizer", "config": cfg, "dtype": "bf16", "batch": B, "size": list(sp), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "parameters": n}
    for name in ms:
        out["ms_per_step_" + name] = ms[name]
        out["median_" + name] = round(statistics.median(ms[name]), 4)
        out["min_" + name], out["max_" + name] = min(ms[name]), max(ms[name])
    out["step_delta_ms"] = round(out["median_adamw"] - out["median_sgd"], 4)
    out["delta_inside_spread"] = bool(out["min_sgd"] <= out["median_adamw"] <= out["max_sgd"] or out["min_adamw"] <= out["median_sgd"] <= out["max_adamw"])
    del steps
    out["kernel"] = kernels(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["2d", "3d"], choices=["2d", "3d"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_optimizer.py measures on the GPU: no device found")
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
