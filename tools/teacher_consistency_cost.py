"""What the mean teacher's consistency term costs per step.  tools/mean_teacher_cost.py's method (bench.py's workload, captured iteration, W untimed
replays, then K replays between two synchronizes) on two steps of one process -- both with a mean teacher, one with teacher_consistency = 0
(launch for launch the step without the argument, tests/test_teacher_consistency_step_gpu.py), one with the term on -- measured in ALTERNATION
for R rounds; and the new launch alone beside chap_kl_fwd_bwd on tensors of pass B's size (HIP events around a captured graph of back-to-back
launches), with the bytes each moves.  One JSON line; --out appends it to a file as well.

    python tools/teacher_consistency_cost.py [--config 2d|3d] [--dtype bf16|fp32] [--weight 0.5] [--steps 30] [--warmup 5] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from chap_amd import ops                                        # noqa: E402
from chap_amd.networks import DualDecoder, DualDecoder3d        # noqa: E402
from chap_amd.synthetic import synthetic_batch, synthetic_batch_3d      # noqa: E402
from chap_amd.train import ChapStep, build_teacher              # noqa: E402
from mean_teacher_cost import timed                             # noqa: E402

DEV = torch.device("cuda", 0)


def build(cfg, dtype, B, weight):
    torch.manual_seed(1337)
    np.random.seed(1337)
    if cfg == "3d":
        make = lambda: DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True).to(DEV)       # noqa: E731
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2)
    else:
        make = lambda: DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)                                              # noqa: E731
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1)
    model = make().train().set_compute_dtype(dtype)
    return ChapStep(model, dict(args, teacher_consistency=weight), teacher=build_teacher(make).eval())


def launch_us(fn, reps=20):
    """One launch of fn(), from a captured graph of `reps` of them."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out)


def kernels(N, C, P):
    """chap_teacher_consistency (accumulating into both dlogits, as the step calls it) and chap_kl_fwd_bwd (loss and both gradients, as the VAT
    branch's final pass calls it) on [N][C][P] tensors -> microseconds, bytes (what the algorithm needs), GB/s."""
    g = torch.Generator(device=DEV).manual_seed(1)
    t = [torch.randn(N, C, P, device=DEV, generator=g) * 3 for _ in range(4)]
    soft = [torch.softmax(x, 1) for x in t[2:]]
    d = [torch.zeros(N, C, P, device=DEV) for _ in range(2)]
    loss, cw = torch.zeros(1, device=DEV), torch.full((1,), 0.5, device=DEV)
    ws = torch.empty(ops.teacher_consistency_ws_words(), device=DEV)
    elems = N * C * P * 4
    us_tc = launch_us(lambda: ops.teacher_consistency(t[:2], t[2:], loss, d, gscale=0.5, gscale_dev=cw, accumulate=True, ws=ws))
    us_kl = launch_us(lambda: ops.kl_fwd_bwd(t[:2], soft, loss, d, gscale=1.0, gscale_dev=cw))
    b_tc, b_kl = 8 * elems, 6 * elems          # 4 read + 2 read + 2 written; 4 read + 2 written
    return {"shape": [N, C, P], "chap_teacher_consistency": {"us": round(us_tc, 2), "bytes": b_tc, "GBps": round(b_tc / us_tc * 1e-3, 1)},
            "chap_kl_fwd_bwd": {"us": round(us_kl, 2), "bytes": b_kl, "GBps": round(b_kl / us_kl * 1e-3, 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="2d", choices=["2d", "3d"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--weight", type=float, default=0.5)
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
    for name, w in (("off", 0.0), ("on", a.weight)):
        steps[name] = build(a.config, dtype, B, w)
        steps[name].capture(vol, lab, warmup=2)
    ms = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name in ("off", "on"):
            ms[name].append(round(timed(steps[name], vol, lab, a.steps, a.warmup), 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "teacher_consistency_cost", "config": a.config, "dtype": a.dtype, "batch": B, "weight": a.weight, "steps": a.steps, "warmup": a.warmup,
            "rounds": a.rounds, "ms_per_step_off": ms["off"], "ms_per_step_on": ms["on"], "median_off": round(med["off"], 4), "median_on": round(med["on"], 4),
            "spread_off": round(max(ms["off"]) - min(ms["off"]), 4), "spread_on": round(max(ms["on"]) - min(ms["on"]), 4),
            "step_delta_ms": round(med["on"] - med["off"], 4),
            "kernels": kernels(B // 2, 2 if d3 else 4, int(np.prod(sp)))}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
