"""What the uncertainty mask of the mean teacher's consistency term costs per step.  tools/teacher_consistency_cost.py's method (bench.py's
workload, captured iteration, W untimed replays, then K replays between two synchronizes) on three steps of one process -- all with a mean
teacher and the term on: teacher_uncertainty = 0 (the plain term), 1 and 4 -- measured in ALTERNATION for R rounds; and each new launch alone
beside chap_teacher_consistency on tensors of pass B's size (HIP events around a captured graph of back-to-back launches), with the bytes
each needs.  One JSON line; --out appends it to a file as well.

    python tools/teacher_uncertainty_cost.py [--config 2d|3d] [--dtype bf16|fp32] [--weight 0.5] [--passes 1 4] [--steps 30] [--warmup 5] [--rounds 5] [--out FILE]
"""
import argparse
import json
import math
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
from teacher_consistency_cost import launch_us                  # noqa: E402

DEV = torch.device("cuda", 0)


def build(cfg, dtype, B, weight, T):
    torch.manual_seed(1337)
    np.random.seed(1337)
    if cfg == "3d":
        make = lambda: DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True).to(DEV)       # noqa: E731
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2)
    else:
        make = lambda: DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)                                              # noqa: E731
        args = dict(batch_size=B, labeled_bs=B // 2, vat_iters=1)
    model = make().train().set_compute_dtype(dtype)
    return ChapStep(model, dict(args, teacher_consistency=weight, teacher_uncertainty=T), teacher=build_teacher(make).eval())


def kernels(N, C, P, passes):
    """chap_teacher_uncertainty at every T of `passes`, chap_teacher_consistency_masked on its mask (threshold 0.9 ln C on 1.5 randn logits: both
    mask values occur) and chap_teacher_consistency, all accumulating as the step calls them, on [N][C][P] tensors -> microseconds, the bytes the
    algorithm needs, GB/s.  The masked kernel's bytes count what it touches for this mask: the mask, and per certain pixel 4 C floats read and
    2 C read and written (the plain kernel's 8 C floats per pixel)."""
    g = torch.Generator(device=DEV).manual_seed(1)
    mk = lambda: torch.randn(N, C, P, device=DEV, generator=g) * 1.5       # noqa: E731
    s = [mk(), mk()]
    t = [[mk(), mk()] for _ in range(max(passes))]
    d = [torch.zeros(N, C, P, device=DEV) for _ in range(2)]
    loss, cw = torch.zeros(1, device=DEV), torch.full((1,), 0.5, device=DEV)
    thr = torch.full((1,), 0.9 * math.log(C), device=DEV)
    ws = torch.empty(ops.teacher_consistency_ws_words(), device=DEV)
    wsi = torch.empty(ops.teacher_uncertainty_ws_words(), dtype=torch.int64, device=DEV)
    elems = N * C * P * 4
    out = {"shape": [N, C, P]}
    us = launch_us(lambda: ops.teacher_consistency(s, t[0], loss, d, gscale=0.5, gscale_dev=cw, accumulate=True, ws=ws))
    out["chap_teacher_consistency"] = {"us": round(us, 2), "bytes": 8 * elems, "GBps": round(8 * elems / us * 1e-3, 1)}
    for T in passes:
        us = launch_us(lambda: ops.teacher_uncertainty(t[:T], threshold_dev=thr, ws=wsi))
        b = 2 * T * elems + N * P
        out["chap_teacher_uncertainty_T%d" % T] = {"us": round(us, 2), "bytes": b, "GBps": round(b / us * 1e-3, 1)}
    mask, count = ops.teacher_uncertainty(t[:max(passes)], threshold_dev=thr, ws=wsi)
    torch.cuda.synchronize()
    share = int(count) / (N * P)
    us = launch_us(lambda: ops.teacher_consistency_masked(s, t[0], mask, count, loss, d, gscale=0.5, gscale_dev=cw, accumulate=True, ws=ws))
    b_all, b_touched = 8 * elems + N * P, int(8 * elems * share) + N * P
    out["chap_teacher_consistency_masked"] = {"us": round(us, 2), "certain_share": round(share, 4), "bytes_all_certain": b_all, "bytes": b_touched,
                                              "GBps": round(b_touched / us * 1e-3, 1)}
    ones, full = torch.ones_like(mask), torch.full((1,), N * P, dtype=torch.int64, device=DEV)
    us = launch_us(lambda: ops.teacher_consistency_masked(s, t[0], ones, full, loss, d, gscale=0.5, gscale_dev=cw, accumulate=True, ws=ws))
    out["chap_teacher_consistency_masked_all_certain"] = {"us": round(us, 2), "bytes": b_all, "GBps": round(b_all / us * 1e-3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="2d", choices=["2d", "3d"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 4])
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
    for T in [0] + a.passes:
        steps[T] = build(a.config, dtype, B, a.weight, T)
        steps[T].capture(vol, lab, warmup=2)
    ms = {T: [] for T in steps}
    for _ in range(a.rounds):
        for T in steps:
            ms[T].append(round(timed(steps[T], vol, lab, a.steps, a.warmup), 4))
    med = {T: statistics.median(v) for T, v in ms.items()}
    line = {"tool": "teacher_uncertainty_cost", "config": a.config, "dtype": a.dtype, "batch": B, "weight": a.weight, "steps": a.steps, "warmup": a.warmup,
            "rounds": a.rounds, "ms_per_step": {"T%d" % T: v for T, v in ms.items()}, "median": {"T%d" % T: round(v, 4) for T, v in med.items()},
            "spread": {"T%d" % T: round(max(v) - min(v), 4) for T, v in ms.items()},
            "delta_ms_over_plain_term": {"T%d" % T: round(med[T] - med[0], 4) for T in a.passes},
            "kernels": kernels(B // 2, 2 if d3 else 4, int(np.prod(sp)), a.passes)}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
