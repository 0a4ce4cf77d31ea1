"""Helper process of tests/test_train_dp_gpu.py (NOT a test module): one rank of train(), or the plain single process.

    python tests/train_dp_worker.py JOB.json

The rank comes from the environment (RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT), as under torch.distributed.run.  JOB.json:
{"entry": "2d" | "3d", "args": {train() args}, "snapshot": DIR, "out": FILE.pt, "data": "store" | "fixed" | "synthetic",
 "loader_rank": r, "loader_world": w}.  `data`: "store" feeds a DeviceLoader(rank=loader_rank, world=loader_world) over the small store built
here (loader_rank / loader_world default to the process's rank and world); "fixed" feeds the same four host batches on every rank;
"synthetic" leaves the loader to train().  The validation volumes are val_volumes_2d() / val_volumes_3d().

Writes to `out`: the flat parameters, the momentum, the EMA buffer (or None), per launch of the loader the global batch's store indices and
the rank's own, every per-volume validation value this rank computed, in call order, and what the gradients were exchanged through (None: no
group; "module": torch.distributed itself, i.e. RCCL; "HostStagedDist": gloo through host memory)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZE_2D, PATCH_3D = (64, 64), (16, 32, 16)
N_LAB_2D, N_LAB_3D = 17, 5


def slices_2d():
    """38 ragged slices (17 labelled at the head) cut from fixed-seed synthetic 80 x 80 ones."""
    from chap_amd.synthetic import synthetic_batch
    v, l = synthetic_batch(501, 38, 0, 80, 80, 4)
    shapes = [(80, 80), (64, 72), (71, 57), (60, 60), (77, 66), (58, 80), (80, 49)]
    images = [v[i, 0, :shapes[i % 7][0], :shapes[i % 7][1]].numpy().copy() for i in range(38)]
    labels = [l[i, :shapes[i % 7][0], :shapes[i % 7][1]].numpy().astype(np.uint8) for i in range(38)]
    return images, labels


def volumes_3d():
    """12 volumes (5 labelled at the head), some smaller than the patch on an axis (pad=True)."""
    from chap_amd.synthetic import synthetic_batch_3d
    v, l = synthetic_batch_3d(502, 12, 0, 24, 40, 24)
    crops = [(24, 40, 24), (20, 36, 20), (14, 40, 24), (24, 30, 18), (22, 40, 12), (24, 34, 24)]
    images = [v[i, 0, :crops[i % 6][0], :crops[i % 6][1], :crops[i % 6][2]].numpy().copy() for i in range(12)]
    labels = [l[i, :crops[i % 6][0], :crops[i % 6][1], :crops[i % 6][2]].numpy().astype(np.uint8) for i in range(12)]
    return images, labels


def val_volumes_2d():
    """Three volumes of 3, 5 and 4 slices: world 2 scores shards of 2 and 1."""
    from chap_amd.synthetic import synthetic_batch
    out = []
    for k, s in enumerate((3, 5, 4)):
        vi, vl = synthetic_batch(900 + k, s, 0, *SIZE_2D, 4)
        out.append((vi[:, 0].unsqueeze(0), vl.unsqueeze(0)))
    return out


def val_volumes_3d():
    from chap_amd.synthetic import synthetic_batch_3d
    v, l = synthetic_batch_3d(901, 3, 0, 24, 40, 20)
    cuts = [(24, 40, 20), (18, 34, 16), (22, 40, 14)]
    return [(v[i, 0, :c[0], :c[1], :c[2]].numpy().copy(), l[i, :c[0], :c[1], :c[2]].numpy().copy()) for i, c in enumerate(cuts)]


def fixed_batches(entry, a):
    lbs, ubs = a["labeled_bs"], a["batch_size"] - a["labeled_bs"]
    if entry == "2d":
        from chap_amd.synthetic import synthetic_batch
        pool = [synthetic_batch(700 + i, lbs, ubs, *a["image_size"], a["num_classes"]) for i in range(4)]
    else:
        from chap_amd.synthetic import synthetic_batch_3d
        pool = [synthetic_batch_3d(700 + i, lbs, ubs, *a["patch_size"], n_classes=a["num_classes"]) for i in range(4)]
    return [{"image": v, "label": l} for v, l in pool]


def main():
    job = json.load(open(sys.argv[1]))
    entry, a = job["entry"], dict(job["args"])
    if entry == "2d":
        from chap_amd import train_ours_2D as T
    else:
        from chap_amd import train_ours_3D as T
    from chap_amd.data import DeviceLoader, SliceStore, VolumeStore
    from chap_amd.distributed import rank_environment
    from chap_amd.train import ChapStep
    rank, world, _ = rank_environment() if a.get("data_parallel") else (0, 1, 0)
    steps, launches, scored = [], [], []

    class Kept(ChapStep):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            steps.append(self)

    class Recorded(DeviceLoader):
        def _launch(self, idxs, image_out, label_out):
            super()._launch(idxs, image_out, label_out)
            launches.append({"global": list(self.last_global_indices), "own": [d["index"] for d in self.last_draws]})

    T.ChapStep = Kept
    if entry == "2d":
        inner = T.test_single_volume

        def scoring(*args, **kw):
            r = inner(*args, **kw)
            scored.append(np.array(r))
            return r
        T.test_single_volume = scoring
    else:
        inner = T.var_each_case

        def scoring(*args, **kw):
            r = inner(*args, **kw)
            scored.extend(r)
            return r
        T.var_each_case = scoring
    dev = torch.device("cuda", a.get("gpu", 0))
    if job["data"] == "store":
        lr, lw = job.get("loader_rank", rank), job.get("loader_world", world)
        if entry == "2d":
            store = SliceStore(*slices_2d(), dev)
            a["trainloader"] = Recorded(store, range(N_LAB_2D), range(N_LAB_2D, len(store)), a["batch_size"], a["labeled_bs"], a["image_size"], a["seed"],
                                        rank=lr, world=lw)
        else:
            store = VolumeStore(*volumes_3d(), dev)
            a["trainloader"] = Recorded(store, range(N_LAB_3D), range(N_LAB_3D, len(store)), a["batch_size"], a["labeled_bs"], a["patch_size"], a["seed"],
                                        pad=True, rank=lr, world=lw)
    elif job["data"] == "fixed":
        a["trainloader"] = fixed_batches(entry, a)
    a["val_volumes"] = val_volumes_2d() if entry == "2d" else val_volumes_3d()
    T.train(a, job["snapshot"])
    step = steps[0]
    torch.cuda.synchronize()
    torch.save({"flat": step.model.flat_buffers()[0].cpu(), "mom": step.opt.mom.cpu(), "ema": None if step.opt.ema is None else step.opt.ema.cpu(),
                "launches": launches, "scored": scored, "exchange": None if step.grad_sync is None else type(step.grad_sync.dist).__name__, "iter_num": step.iter_num, "rank": rank, "world": world}, job["out"])


if __name__ == "__main__":
    main()
