"""Timing of the segmentation metrics (chap_amd.metrics, chap_metrics) against the scipy restatement (tests/metrics_restatement.py) on
two synthetic inputs: an ACDC-like [10, 216, 256] label map with 3 classes, and an LA-like 88 x 576 x 576 ellipsoid pair with noisy
surfaces (1 class).  GPU: warm, device-synchronised wall time of one call (inputs already on the device; the one result copy to the
host is part of the call), median of --reps.  CPU: all seven metrics from one EDT per class and direction (the cheapest host form; a
medpy caller recomputes them per metric), median of --cpu-reps.  Prints one JSON line per case; --out appends them to a file.
Run under `rocprofv3 --kernel-trace --stats` (in a run of its own) for the kernel statistics."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                   # noqa: E402
import torch                                         # noqa: E402
from scipy import ndimage                            # noqa: E402

from chap_amd import metrics                         # noqa: E402
from tests import metrics_restatement as R           # noqa: E402


def acdc_like(seed=0):
    rng = np.random.default_rng(seed)
    S, X, Y = 10, 216, 256
    z, y, x = np.ogrid[:S, :X, :Y]
    r = ((y - 108) / 60.0) ** 2 + ((x - 128) / 70.0) ** 2 + ((z - 5) / 9.0) ** 2
    lab = np.zeros((S, X, Y), np.int64)
    for c, t in ((1, 1.0), (2, 0.6), (3, 0.3)):
        lab[r < t] = c
    noise = ndimage.gaussian_filter(rng.standard_normal((S, X, Y)), 2.0) * 0.5
    pred = np.zeros((S, X, Y), np.uint8)
    for c, t in ((1, 1.0), (2, 0.6), (3, 0.3)):
        pred[r + noise < t] = c
    return pred, lab


def la_like(seed=3):
    D, H, W = 88, 576, 576
    z, y, x = np.ogrid[:D, :H, :W]
    rng = np.random.default_rng(seed)
    noise = ndimage.zoom(rng.standard_normal((12, 36, 36)), (D / 12, H / 36, W / 36), order=1)
    ra = ((z - 44) / 30.0) ** 2 + ((y - 290) / 150.0) ** 2 + ((x - 280) / 170.0) ** 2
    rb = ((z - 46) / 28.0) ** 2 + ((y - 284) / 156.0) ** 2 + ((x - 290) / 160.0) ** 2
    return ra + 0.08 * noise < 1.0, rb - 0.08 * noise < 1.0


def cpu_all(a, b):
    """The seven metrics of two binary masks from the restatement's definitions, one EDT per direction."""
    ba, bb = R.border(a), R.border(b)
    s_ab = ndimage.distance_transform_edt(~bb)[ba]
    s_ba = ndimage.distance_transform_edt(~ba)[bb]
    return dict(dc=R.dc(a, b), jc=R.jc(a, b), ravd=R.ravd(a, b), hd=max(s_ab.max(), s_ba.max()),
                hd95=np.percentile(np.hstack((s_ab, s_ba)), 95), asd=s_ab.mean(), assd=np.mean((s_ab.mean(), s_ba.mean())))


def timed(fn, reps, sync):
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="acdc,la")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for case in a.cases.split(","):
        if case == "acdc":
            pred, lab = acdc_like()
            classes = [1, 2, 3]
            pd, ld = torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev)
            gpu = lambda: metrics.per_class(pd, ld, classes)                                            # noqa: E731
            cpu = lambda: [cpu_all(pred == c, lab == c) for c in classes]                              # noqa: E731
            host = lambda: metrics.per_class(pred, lab, classes)                                       # noqa: E731
        else:
            A, B = la_like()
            pred, lab, classes = A, B, [1]
            pd, ld = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
            gpu = lambda: metrics.per_class(pd, ld, classes)                                            # noqa: E731
            cpu = lambda: [cpu_all(A, B)]                                                              # noqa: E731
            host = lambda: metrics.per_class(A.view(np.uint8), B.view(np.uint8), classes)              # noqa: E731
        for _ in range(a.warmup):
            gpu()
        t_gpu, r = timed(gpu, a.reps, True)
        t_host, _ = timed(host, max(3, a.reps // 4), True)
        t_cpu, ref = timed(cpu, a.cpu_reps, False)
        err = 0.0
        for k, c in enumerate(classes):
            for name in ("dc", "jc", "ravd", "hd", "hd95", "asd", "assd"):
                want = float(ref[k][name])
                err = max(err, abs(float(r[name][k]) - want) / max(abs(want), 1e-300))
        line = dict(case=case, shape=list(pred.shape), classes=classes, gpu_ms=round(t_gpu, 3), gpu_ms_host_input=round(t_host, 3),
                    cpu_ms=round(t_cpu, 1), speedup=round(t_cpu / t_gpu, 1), max_rel_err=err, reps=a.reps, cpu_reps=a.cpu_reps,
                    hd95=[float(v) for v in r["hd95"]], device=torch.cuda.get_device_name(0))
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
