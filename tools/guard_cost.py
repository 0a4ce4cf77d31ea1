"""What the gradient guard costs per step, in the manner of tools/monitor_cost.py.  bench.py's default 2D and 3D bf16 workloads and its timing
method (captured iteration, W untimed replays, then K replays between two synchronizes) on up to three steps of one process, measured in
ALTERNATION for R rounds so that drift of the device hits all alike:

    parent   the step of ANOTHER checkout of this project (--parent DIR: its chap_amd package, with its own built library, is imported
             under another name beside this tree's) -- the commit this feature was added to;
    off      this tree's step without a guard: its median has to lie inside the parent's measured spread [min, max] of the same visit;
    on       this tree's step with StepGuard(max_norm=1.0): clipping and the non-finite check both armed.

The guarded step's ring is read once per round, as train() reads it once per validation interval.  Then chap_grad_norm and the two optimizer
entries alone at the configuration's parameter count (HIP events around a captured graph of back-to-back launches).  --out writes one JSON
document: {"2d": {...}, "3d": {...}}.

    python tools/guard_cost.py [--parent DIR] [--configs 2d 3d] [--steps 200] [--warmup 10] [--rounds 4] [--order parent off on] [--out profiles/guard_cost.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import chap_amd                                                  # noqa: E402
from chap_amd import ops                                         # noqa: E402
from chap_amd.guard import StepGuard                             # noqa: E402
from chap_amd.synthetic import synthetic_batch, synthetic_batch_3d      # noqa: E402

DEV = torch.device("cuda", 0)


def load_package(root, name):
    """The chap_amd package of another checkout under `name` (its modules import each other relatively; its library is its own file)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "chap_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(root, "chap_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def build(pkg, cfg, dtype, B, guard):
    nets = importlib.import_module(pkg.__name__ + ".networks")
    train = importlib.import_module(pkg.__name__ + ".train")
    torch.manual_seed(1337)
    np.random.seed(1337)
    if cfg == "3d":
        model = nets.DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True).to(DEV)
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2)
    else:
        model = nets.DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1)
    model = model.train().set_compute_dtype(dtype)
    return train.ChapStep(model, args, guard=guard) if guard is not None else train.ChapStep(model, args)


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


def kernels_us(n):
    """chap_grad_norm (both launches) and the optimizer entries alone on n parameters and two buckets; zero_grad off, so every launch reads what
    the first one read."""
    g = torch.Generator().manual_seed(3)
    p, g1, g2, m = (torch.randn(n, generator=g).to(DEV) * s for s in (1.0, 1e-3, 1e-3, 0.0))
    lr = torch.tensor([1e-6], device=DEV)
    guard = StepGuard(max_norm=1.0, ring=8, device=DEV)
    return {"n": n,
            "chap_grad_norm": round(graph_us(lambda: ops.grad_norm(g1, g2, guard.ws, guard.state, guard.R, 1.0, 1.0, True)), 2),
            "chap_sgd_step": round(graph_us(lambda: ops.sgd_step(p, g1, m, lr, 0.9, 1e-4, 1.0, False, g2)), 2),
            "chap_sgd_guard_step": round(graph_us(lambda: ops.sgd_guard_step(p, g1, m, lr, 0.9, 1e-4, guard.state, None, None, 1.0, False, g2)), 2),
            "bytes": {"chap_grad_norm": 8 * n, "chap_sgd_step": 24 * n, "chap_sgd_guard_step": 24 * n}}      # g, g2 read; + p, m read and written


def one(cfg, a, parent):
    d3 = cfg == "3d"
    B, sp = (4, (112, 112, 80)) if d3 else (24, (256, 256))
    vol, lab = (synthetic_batch_3d if d3 else synthetic_batch)(1337, B // 2, B - B // 2, *sp)
    vol, lab = vol.to(DEV), lab.to(DEV)
    variants = ([("parent", parent, None)] if parent is not None else []) + [("off", chap_amd, None), ("on", chap_amd, StepGuard(max_norm=1.0, ring=256, device=DEV))]
    variants.sort(key=lambda v: a.order.index(v[0]))            # the order in which the steps are built, captured and timed within a round
    steps = {}
    for name, pkg, guard in variants:
        steps[name] = build(pkg, cfg, torch.bfloat16, B, guard)
        steps[name].capture(vol, lab, warmup=2)
    ms, rows = {name: [] for name, _, _ in variants}, 0
    for _ in range(a.rounds):
        for name, _, _ in variants:
            ms[name].append(round(timed(steps[name], vol, lab, a.steps, a.warmup), 4))
        r = steps["on"].guard.read()
        rows += len(r["step"]) + r["dropped"]
    n = steps["on"].grad_both.numel() // 2
    last = steps["on"].guard.read()
    out = {"tool": "guard_cost", "config": cfg, "order": [name for name, _, _ in variants], "dtype": "bf16", "batch": B, "size": list(sp), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "parameters": n, "rows_accounted_for": rows, "clipped_total": last["clipped_total"], "skipped_total": last["skipped_total"]}
    for name in ms:
        out["ms_per_step_" + name] = ms[name]
        out["median_" + name] = round(statistics.median(ms[name]), 4)
        out["spread_" + name] = round(max(ms[name]) - min(ms[name]), 4)
    base = "parent" if parent is not None else "off"
    out["baseline"] = base
    out["step_delta_ms"] = round(out["median_on"] - out["median_" + base], 4)
    if parent is not None:
        out["off_within_parent_spread"] = bool(min(ms["parent"]) <= out["median_off"] <= max(ms["parent"]))
    out["kernel_us"] = kernels_us(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="root of a checkout of the parent commit with its library built")
    ap.add_argument("--configs", nargs="+", default=["2d", "3d"], choices=["2d", "3d"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--order", nargs=3, default=["parent", "off", "on"], choices=["parent", "off", "on"],
                    help="order of the three steps within a round (a step's place in the process can move its time more than the guard does)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = load_package(os.path.abspath(a.parent), "chap_amd_parent") if a.parent else None
    doc = {}
    for cfg in a.configs:
        doc[cfg] = one(cfg, a, parent)
        print(json.dumps(doc[cfg]), flush=True)
        if a.out:       # (after every configuration: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
