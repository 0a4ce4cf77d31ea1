"""Is the mean teacher's Dice less noisy from seed to seed than the student's?  tools/dice_pairs.py's protocol (BASELINE config 1 on the
synthetic fixed-seed data, graph replay, `--iters` iterations with the poly LR running to zero, the same seeds, 24 held-out slices, logit
ensemble + arg-max) with a teacher attached (ema_decay 0.99): ONE run per (seed, dtype) gives both figures -- the student of such a run is bit
for bit the student of dice_pairs.py's run (tests/test_mean_teacher_step_gpu.py) -- the teacher evaluated after sync_teacher_stats().
Reported per mode: Dice of student and teacher per seed, mean, seed-to-seed s.d., and the paired difference teacher - student.

    python tools/mean_teacher_dice.py [--seeds 6] [--iters 1500] [--size 256] [--batch 24] [--decay 0.99] [--out FILE]
                                      [--teacher-consistency W] [--teacher-noise A] [--teacher-uncertainty T] [--modes fp32,bf16]

`--teacher-consistency W` (default 0: the teacher is only averaged) switches the teacher's consistency term on with weight W
(ChapStep args teacher_consistency / teacher_noise): the same protocol, initial weights, data order and noise seed, so the figures of a run
with W > 0 are compared with those of a run with W = 0 made beside it.  `--teacher-uncertainty T` (default 0; needs W > 0) masks the term with
the entropy of T noisy teacher passes (ChapStep args teacher_uncertainty, default threshold ramp): compared with the W > 0, T = 0 run made beside it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dice_pairs import DEV, dice_per_class, stats               # noqa: E402
from chap_amd.networks import DualDecoder                       # noqa: E402
from chap_amd.synthetic import synthetic_batch                  # noqa: E402
from chap_amd.train import ChapStep, build_teacher              # noqa: E402


def predict(m, val):
    m.eval()
    with torch.no_grad():
        o1, o2 = m(val.to(DEV))
    return torch.argmax(torch.softmax((o1 + o2) / 2.0, dim=1), dim=1).cpu().numpy()


def train_and_dice(dtype, seed, B, H, W, iters, decay, lr=0.05, consistency=0.0, noise=0.1, uncertainty=0):
    """dice_pairs.train_and_dice, line for line, with a teacher: -> (student Dice per class, teacher Dice per class, seconds)."""
    lbs = B // 2
    pool = [synthetic_batch(2000 + 100 * seed + i, lbs, B - lbs, H, W) for i in range(16)]
    pool = [(v.to(DEV), l.to(DEV)) for v, l in pool]
    val, gt = synthetic_batch(4242, 24, 0, H, W)
    torch.manual_seed(1337 + seed)
    np.random.seed(1337 + seed)
    make = lambda: DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)      # noqa: E731
    m = make().train().set_compute_dtype(dtype)
    teacher = build_teacher(make).eval()
    torch.manual_seed(7000 + seed)
    step = ChapStep(m, dict(labeled_bs=lbs, batch_size=B, base_lr=lr, max_iterations=iters, ema_decay=decay, teacher_consistency=consistency, teacher_noise=noise,
                            teacher_uncertainty=uncertainty),
                    teacher=teacher)
    step.capture(*pool[0], warmup=1)
    t0 = time.time()
    for it in range(iters):
        step.replay(*pool[it % len(pool)])
    torch.cuda.synchronize()
    secs = time.time() - t0
    step.sync_teacher_stats()
    return dice_per_class(predict(m, val), gt.numpy()), dice_per_class(predict(teacher, val), gt.numpy()), secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--decay", type=float, default=0.99)
    ap.add_argument("--out", default=None, help="also write the whole record (per-seed runs included) to this file")
    ap.add_argument("--teacher-consistency", type=float, default=0.0, help="weight of the teacher's consistency term (0: off)")
    ap.add_argument("--teacher-noise", type=float, default=0.1)
    ap.add_argument("--teacher-uncertainty", type=int, default=0, help="T noisy teacher passes behind the term's entropy mask (0: the plain term)")
    ap.add_argument("--modes", default="fp32,bf16")
    a = ap.parse_args()
    modes = [(n, {"fp32": torch.float32, "bf16": torch.bfloat16}[n]) for n in a.modes.split(",")]
    runs = []
    for s in range(a.seeds):
        r = {"seed": s}
        for name, dtype in modes:
            ds, dt, secs = train_and_dice(dtype, s, a.batch, a.size, a.size, a.iters, a.decay, consistency=a.teacher_consistency, noise=a.teacher_noise,
                                          uncertainty=a.teacher_uncertainty)
            r.update({"student_" + name: float(ds.mean()), "teacher_" + name: float(dt.mean()), "student_classes_" + name: ds.round(5).tolist(),
                      "teacher_classes_" + name: dt.round(5).tolist(), "seconds_" + name: round(secs, 1)})
        print(json.dumps(r), flush=True)
        runs.append(r)
    out = {"config": {"size": a.size, "batch": a.batch, "iterations": a.iters, "seeds": a.seeds, "lr": 0.05, "ema_decay": a.decay, "teacher_consistency": a.teacher_consistency,
                      "teacher_noise": a.teacher_noise, "teacher_uncertainty": a.teacher_uncertainty, "data": "synthetic fixed-seed",
                      "teacher_bn_statistics": "the student's (ChapStep.sync_teacher_stats)"}, "runs": runs}
    for name, _ in modes:
        out[name] = {"student": stats([r["student_" + name] for r in runs]), "teacher": stats([r["teacher_" + name] for r in runs]),
                     "paired_diff_teacher_minus_student": stats([r["teacher_" + name] - r["student_" + name] for r in runs])}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
