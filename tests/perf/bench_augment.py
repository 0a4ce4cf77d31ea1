"""Host loader against the device-resident data layer (chap_amd.data): the three measurements of profiles/augment_host_vs_device.json.

  host    the scipy form of RandomGenerator (tests/augment_restatement.augment_scipy, one process) per slice, 256 x 216 -> 256 x 256,
          per branch and for the 0.5 / 0.25 / 0.25 mix of branches; the slices/s four such workers would give
  device  DeviceLoader.next_into for a batch of 24 at 256 x 256 (record upload + chap_augment2d), device events around N launches
  e2e     ms per iteration of N graph replays fed by ChapStep.stage_from, against the same replays fed by ChapStep.stage() from
          pre-built pinned host batches: old, new, old, new in one process (the two old runs give the run-to-run noise)

    python tests/perf/bench_augment.py --out profiles/augment_host_vs_device.json [--bench-line FILE]

--bench-line: a file holding the JSON line `python bench.py` printed in the same visit; its ms_per_step is what the step consumes."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from chap_amd.data import DeviceLoader, SliceStore      # noqa: E402
from tests import augment_restatement as R              # noqa: E402


def host_baseline(n):
    rng = np.random.default_rng(0)
    img, lab = rng.random((256, 216), dtype=np.float32), rng.integers(0, 4, (256, 216)).astype(np.uint8)
    branches = {"rotflip": [dict(mode=R.MODE_ROTFLIP, k=i % 4, axis=i % 2, angle=0) for i in range(n)],
                "rotate": [dict(mode=R.MODE_ROTATE, k=0, axis=0, angle=i % 40 - 20) for i in range(n)],
                "none": [dict(mode=R.MODE_NONE, k=0, axis=0, angle=0) for i in range(n)]}
    ms = {}
    for name, draws in branches.items():
        R.augment_scipy(img, lab, draws[0], (256, 256))
        t0 = time.perf_counter()
        for d in draws:
            R.augment_scipy(img, lab, d, (256, 256))
        ms[name] = (time.perf_counter() - t0) / n * 1e3
    mix = 0.5 * ms["rotflip"] + 0.25 * ms["rotate"] + 0.25 * ms["none"]
    return {"ms_per_slice": {k: round(v, 4) for k, v in ms.items()}, "ms_per_slice_mix": round(mix, 4), "slices_per_branch": n,
            "slices_per_s_one_process": round(1e3 / mix, 1), "slices_per_s_four_workers": round(4e3 / mix, 1),
            "note": "transform only: no h5 read, no collation, no pinning, no PCIe copy"}


def make_store(n, dev):
    rng = np.random.default_rng(1)
    shapes = [(256, 216), (216, 256), (224, 154), (256, 256)]
    images = [rng.random(shapes[i % 4], dtype=np.float32) for i in range(n)]
    labels = [rng.integers(0, 4, shapes[i % 4]).astype(np.uint8) for i in range(n)]
    return SliceStore(images, labels, dev)


def device_launches(store, n, dev):
    loader = DeviceLoader(store, range(len(store) // 4), range(len(store) // 4, len(store)), 24, 12, (256, 256), seed=3)
    img = torch.empty(24, 1, 256, 256, device=dev)
    lab = torch.empty(24, 256, 256, dtype=torch.int64, device=dev)
    for _ in range(10):
        loader.next_into(img, lab)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        loader.next_into(img, lab)
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the kernel alone: the same record table n times, nothing between the launches
    from chap_amd import ops
    rec = loader._dev[(loader._slot - 1) % loader.RING]
    e2, e3 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e2.record()
    for _ in range(n):
        ops.augment2d(store.images, store.labels, rec, img, lab)
    e3.record()
    torch.cuda.synchronize()
    written = img.numel() * 4 + lab.numel() * 8
    return {"launches": n, "batch": 24, "size": [256, 256], "us_per_next_into_device_events": round(e0.elapsed_time(e1) / n * 1e3, 2),
            "us_per_next_into_host_wall": round(wall / n * 1e6, 2), "us_per_kernel_back_to_back": round(e2.elapsed_time(e3) / n * 1e3, 2),
            "bytes_written": written, "note": "next_into = host draws + record upload (pinned, asynchronous) + one kernel; the host wall "
            "time per call is what the training loop's thread spends, the device-event time includes waiting for that thread"}


def end_to_end(store, n, dev):
    from chap_amd.networks import DualDecoder
    from chap_amd.synthetic import synthetic_batch
    from chap_amd.train import ChapStep
    B = 24
    torch.manual_seed(1337)
    model = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev).train().set_compute_dtype(torch.bfloat16)
    step = ChapStep(model, dict(batch_size=B, labeled_bs=B // 2, vat_iters=1))
    vol, lab = synthetic_batch(1337, B // 2, B - B // 2, 256, 256)
    step.capture(vol.to(dev), lab.to(dev), warmup=2)
    pinned = [tuple(t.pin_memory() for t in synthetic_batch(1337 + i, B // 2, B - B // 2, 256, 256)) for i in range(4)]
    loader = DeviceLoader(store, range(len(store) // 4), range(len(store) // 4, len(store)), B, B // 2, (256, 256), seed=3)

    def run(kind, steps):
        feed = (lambda i: step.stage_from(loader)) if kind == "stage_from" else (lambda i: step.stage(*pinned[i % 4]))
        feed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            out = step.replay()
            feed(i + 1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        step.replay()                               # consume the batch left staged
        assert bool(torch.isfinite(out["vat_loss"]).all())
        return dt / steps * 1e3

    run("stage", 20), run("stage_from", 20)         # warm-up of both paths
    order = ["stage", "stage_from", "stage", "stage_from"]
    ms = [(k, round(run(k, n), 4)) for k in order]
    old = [v for k, v in ms if k == "stage"]
    new = [v for k, v in ms if k == "stage_from"]
    return {"replays_per_run": n, "runs_in_order": ms, "ms_per_step_stage_host_pinned": old, "ms_per_step_stage_from_device": new,
            "noise_of_the_old_path_ms": round(abs(old[0] - old[1]), 4), "new_minus_old_ms": round(sum(new) / 2 - sum(old) / 2, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--host-slices", type=int, default=60)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--replays", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    res = {"host": host_baseline(args.host_slices)}
    store = make_store(128, dev)
    res["device"] = device_launches(store, args.launches, dev)
    res["end_to_end"] = end_to_end(store, args.replays, dev)
    if args.bench_line:
        line = json.loads([ln for ln in open(args.bench_line).read().splitlines() if ln.strip().startswith("{")][-1])
        ms = float(line["ms_per_step"])
        res["step"] = {"bench_ms_per_step": ms, "batch": 24, "slices_per_s_consumed": round(24 / ms * 1e3, 1), "source": "python bench.py, same visit"}
        res["host"]["four_workers_over_consumed"] = round(res["host"]["slices_per_s_four_workers"] / res["step"]["slices_per_s_consumed"], 3)
        res["device"]["next_into_fraction_of_step"] = round(res["device"]["us_per_next_into_device_events"] / (ms * 1e3), 5)
        res["device"]["kernel_fraction_of_step"] = round(res["device"]["us_per_kernel_back_to_back"] / (ms * 1e3), 5)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
