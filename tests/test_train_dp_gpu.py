"""Data-parallel train() on the GPU: the rank-sharded DeviceLoader against the world-1 loader of the global batch, bit for bit, and whole runs of
train_ours_2D.train / train_ours_3D.train as ranks (tests/train_dp_worker.py, each rank a fresh process under a timeout of its own, on a free
port): two ranks on ONE GPU over gloo (dp_backend="gloo": the rank logic on real kernels), a 1-rank RCCL group, and -- where the box has two
GPUs -- two ranks over RCCL.  After any non-zero exit of a child the test fails at once and starts nothing further."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_dp_worker as W  # noqa: E402

WORKER = os.path.join(ROOT, "tests", "train_dp_worker.py")
DEV = "cuda"
TIMEOUT = 300

ARGS_2D = dict(model="dualdecoder", decoder_type="mcnet", num_classes=4, batch_size=8, labeled_bs=4, image_size=[64, 64], max_iterations=6,
               val_interval=3, base_lr=0.001, gpu=0, seed=1337, monitor=True, mean_teacher=True)     # (a small step: the Dice of the first validations is not yet 0, so val.csv is written)
ARGS_3D = dict(patch_size=[16, 32, 16], num_classes=2, batch_size=4, labeled_bs=2, max_iterations=4, val_interval=2, stride_xy=8, stride_z=8,
               base_lr=0.01, gpu=0, seed=3, monitor=True, mean_teacher=True)


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, tag, jobs):
    """Start one fresh worker per job (rank r of len(jobs), or the plain process when the job's args have no data_parallel), wait for all under
    TIMEOUT; the first non-zero exit stops the others and fails the test.  Returns what the workers saved."""
    port = _free_port()
    procs, outs = [], []
    for r, job in enumerate(jobs):
        out = str(tmp_path / ("%s_rank%d.pt" % (tag, r)))
        path = str(tmp_path / ("%s_rank%d.json" % (tag, r)))
        with open(path, "w") as f:
            json.dump(dict(job, out=out), f)
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        if job["args"].get("data_parallel"):
            env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(len(jobs)), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        log = open(str(tmp_path / ("%s_rank%d.log" % (tag, r))), "wb")            # a file, not a pipe: nobody has to drain it while we poll
        procs.append((subprocess.Popen([sys.executable, WORKER, path], env=env, stdout=log, stderr=subprocess.STDOUT), log))
        outs.append(out)
    deadline = time.monotonic() + TIMEOUT
    try:
        while True:
            codes = [p.poll() for p, _ in procs]
            bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
            if bad or all(c == 0 for c in codes):
                break
            assert time.monotonic() < deadline, "the workers did not finish within %d s" % TIMEOUT
            time.sleep(0.1)
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    if bad:
        r, c = bad[0]
        pytest.fail("worker %d of %s exited with %s:\n%s" % (r, tag, c, open(str(tmp_path / ("%s_rank%d.log" % (tag, r))), errors="replace").read()[-4000:]))
    return [torch.load(o, weights_only=False) for o in outs]


def _job(entry, args, snapshot, data, **kw):
    return dict(entry=entry, args=args, snapshot=str(snapshot), data=data, **kw)


# ---------------------------------------------------------------------------------------------------- the sharded loader on the device
def _loader_case(dims):
    from chap_amd.data import SliceStore, VolumeStore
    rng = np.random.default_rng(5)
    if dims == 2:
        shapes = [(17, 19), (23, 16), (16, 16), (31, 18), (20, 20), (16, 29), (25, 25), (18, 17), (33, 16), (16, 21), (22, 22),
                  (19, 30), (17, 17), (26, 16), (16, 24), (21, 18), (30, 30), (18, 27), (24, 19), (16, 18), (27, 23), (20, 16), (29, 17), (23, 23)]
        store = SliceStore([rng.random(s, dtype=np.float32) for s in shapes], [rng.integers(0, 4, s).astype(np.uint8) for s in shapes], DEV)
        return store, 11, dict(batch_size=4, labeled_bs=2, output_size=(16, 16)), {}
    shapes = [(8, 8, 4), (6, 9, 3), (12, 10, 6), (5, 5, 2), (10, 12, 8), (9, 7, 5), (16, 8, 4), (8, 13, 7), (7, 7, 7), (11, 9, 4), (8, 8, 9), (13, 13, 5)]
    store = VolumeStore([rng.random(s, dtype=np.float32) for s in shapes], [rng.integers(0, 2, s).astype(np.uint8) for s in shapes], DEV)
    return store, 5, dict(batch_size=2, labeled_bs=1, output_size=(8, 8, 4)), dict(pad=True)


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("via", ["iter", "next_into"])
def test_rank_batches_concatenate_to_the_global_loaders(dims, via):
    from chap_amd.data import DeviceLoader
    store, n_lab, kw, extra = _loader_case(dims)
    B, lbs, out = kw["batch_size"], kw["labeled_bs"], kw["output_size"]
    world = 2
    mk = lambda b, l, **rw: DeviceLoader(store, range(n_lab), range(n_lab, len(store)), b, l, out, seed=11, **extra, **rw)
    glob, ranks = mk(world * B, world * lbs), [mk(B, lbs, rank=r, world=world) for r in range(world)]
    assert [len(x) for x in ranks] == [len(glob)] * world

    def batches(ld):
        if via == "iter":
            it, res = iter(ld), []
            for _ in range(3):
                try:
                    b = next(it)
                except StopIteration:               # an epoch of the global batch size may be shorter than 3
                    it = iter(ld)
                    b = next(it)
                res.append((b["image"].clone(), b["label"].clone()))
            return res
        res = []
        for _ in range(3):
            im = torch.empty((ld.batch_size, 1) + out, dtype=torch.float32, device=DEV)
            lb = torch.empty((ld.batch_size,) + out, dtype=torch.int64, device=DEV)
            ld.next_into(im, lb)
            res.append((im, lb))
        return res
    want, got = batches(glob), [batches(x) for x in ranks]
    torch.cuda.synchronize()
    for k in range(3):
        for j in range(2):
            cat = torch.cat([got[r][k][j][:lbs] for r in range(world)] + [got[r][k][j][lbs:] for r in range(world)])
            assert torch.equal(cat, want[k][j]), (k, j)


# ---------------------------------------------------------------------------------------------------- two ranks of train()
def _expected_global_sequence(n_lab, n_all, world, B, lbs, seed, n_iter, graph):
    """The global sampler driven as train() drives a loader: captured, the first batch comes from iter(loader) and the rest from next_into's
    endless sequence; eager, epoch after epoch of iter(loader)."""
    from chap_amd.data import TwoStreamBatchSampler
    s = TwoStreamBatchSampler(range(n_lab), range(n_lab, n_all), world * B, world * (B - lbs), seed)
    seq = []
    if graph:
        first = iter(s)
        seq.append(next(first))
        while len(seq) < n_iter:
            for idxs in s:
                seq.append(idxs)
                if len(seq) == n_iter:
                    break
        return seq
    while len(seq) < n_iter:
        for idxs in s:
            seq.append(idxs)
            if len(seq) == n_iter:
                break
    return seq


def _check_common(res, snap, n_iter):
    """(a), (c), (d) of the two-rank runs."""
    r0, r1 = res
    assert r0["iter_num"] == r1["iter_num"] == n_iter
    for k in ("flat", "mom", "ema"):                                                                    # (a)
        assert torch.equal(r0[k], r1[k]), k
    files = sorted(os.listdir(snap))                                                                    # (c)
    assert files == sorted(["log.txt", "val.csv", "monitor.csv", "latest.pth", "dualdecoder_best_model.pth", "ema_latest.pth", "dualdecoder_ema_best_model.pth"]), files
    lines = open(os.path.join(snap, "monitor.csv")).read().splitlines()
    assert [int(ln.split(",")[0]) for ln in lines[1:]] == list(range(1, n_iter + 1))
    log = open(os.path.join(snap, "log.txt")).read().splitlines()
    assert len([ln for ln in log if " : l loss : " in ln]) == n_iter
    # val.csv: one row per improvement of the student's Dice, written once (two writers would double them)
    best, improved = 0.0, []
    for ln in log:
        for key in (" : model1_mean_dice : ", " : dice_score : "):
            if key in ln and "ema" not in ln:
                it, d = int(ln.split(" : ")[0].split()[1]), float(ln.split(key)[1].split()[0])
                if d > best:
                    best, improved = d, improved + [it]
    assert improved and [int(r.split(",")[1]) for r in open(os.path.join(snap, "val.csv")).read().splitlines()] == improved


def _load_latest(make, snap):
    m = make().to(DEV)
    m.load_state_dict(torch.load(os.path.join(snap, "latest.pth"), map_location=DEV), strict=True)
    return m.eval()


def _two_ranks_2d(tmp_path, use_graph, backend):
    from chap_amd.inference import test_single_volume as score
    from chap_amd.networks.net_factory import net_factory
    snap = tmp_path / "run"
    a = dict(ARGS_2D, use_graph=use_graph, data_parallel=True, dp_backend=backend)
    res = _run_ranks(tmp_path, "dp", [_job("2d", a, snap, "store")] * 2)
    n_iter = a["max_iterations"]
    _check_common(res, str(snap), n_iter)
    assert [x["exchange"] for x in res] == ["HostStagedDist" if backend == "gloo" else "module"] * 2
    # (b) the indices the ranks consumed, put together, are the global sampler's sequence
    B, lbs = a["batch_size"], a["labeled_bs"]
    want = _expected_global_sequence(W.N_LAB_2D, 38, 2, B, lbs, a["seed"], n_iter, use_graph)
    for r in range(2):
        assert [l["global"] for l in res[r]["launches"]] == [[int(i) for i in w] for w in want], r
        for l, w in zip(res[r]["launches"], want):
            assert l["own"] == [int(i) for i in w[r * lbs:(r + 1) * lbs] + w[2 * lbs + r * (B - lbs):2 * lbs + (r + 1) * (B - lbs)]]
    # (d) latest.pth is rank 0's parameters at the last iteration
    make = lambda: net_factory(net_type="dualdecoder", in_chns=1, class_num=4, device=DEV, args=a)
    m = _load_latest(make, str(snap))
    assert torch.equal(m.flat_buffers()[0].cpu(), res[0]["flat"])
    # (e) the logged Dice is the single process's over all volumes in order; per volume, the ranks' values are that process's, bit for bit
    val = W.val_volumes_2d()
    per = [np.array(score(im, lb, m, classes=4, patch_size=a["image_size"], model_type="logit_ensemble", device=torch.device(DEV))) for im, lb in val]
    metric = sum(per) / len(val)
    line = "iteration %d : model1_mean_dice : %f model1_mean_hd95 : %f" % (n_iter, float(np.mean(metric, axis=0)[0]), float(np.mean(metric, axis=0)[1]))
    assert line in open(os.path.join(str(snap), "log.txt")).read().splitlines()
    # each rank scored student then teacher at iterations 3 and 6: the student's values of the last validation are 2 * n_own from the end
    for r in range(2):
        own = list(range(r, len(val), 2))
        got = res[r]["scored"][-2 * len(own):-len(own)]
        assert len(res[r]["scored"]) == 4 * len(own)
        for g, i in zip(got, own):
            assert np.array_equal(g, per[i]), (r, i)
    # (f) an exchange took place: the plain process on rank 0's shard alone ends elsewhere
    alone = _run_ranks(tmp_path, "alone", [_job("2d", dict(ARGS_2D, use_graph=use_graph), tmp_path / "alone", "store", loader_rank=0, loader_world=2)])[0]
    assert [l["own"] for l in alone["launches"]] == [l["own"] for l in res[0]["launches"]]
    assert not torch.equal(alone["flat"], res[0]["flat"])


@pytest.mark.parametrize("use_graph", [True, False])
def test_two_ranks_of_train_2d_on_one_gpu(tmp_path, use_graph):
    _two_ranks_2d(tmp_path, use_graph, "gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="two ranks over RCCL need two GPUs")
def test_two_ranks_of_train_2d_over_rccl(tmp_path):
    _two_ranks_2d(tmp_path, True, "nccl")


@pytest.mark.parametrize("use_graph", [True, False])
def test_exchange_end_to_end_equals_the_plain_run(tmp_path, use_graph):
    """World 2 over gloo, the same fixed batches and (dp_noise_per_rank=False) the same noise on both ranks: (g + g) / 2 is exact and the fold adds
    the two words the plain optimizer launch adds, so after 4 iterations parameters and momentum are the plain train()'s, bit for bit."""
    a = dict(ARGS_2D, use_graph=use_graph, max_iterations=4, val_interval=2, monitor=False, mean_teacher=False)
    res = _run_ranks(tmp_path, "dp", [_job("2d", dict(a, data_parallel=True, dp_backend="gloo", dp_noise_per_rank=False), tmp_path / "dp", "fixed")] * 2)
    plain = _run_ranks(tmp_path, "plain", [_job("2d", a, tmp_path / "plain", "fixed")])[0]
    for r in range(2):
        assert res[r]["iter_num"] == plain["iter_num"] == 4
        assert torch.equal(res[r]["flat"], plain["flat"]) and torch.equal(res[r]["mom"], plain["mom"]), r


def test_two_ranks_of_train_3d_on_one_gpu(tmp_path):
    from chap_amd.networks.net_factory_3d import net_factory_3d
    from chap_amd.test_3d_patch import var_all_case
    snap = tmp_path / "run"
    a = dict(ARGS_3D, data_parallel=True, dp_backend="gloo")
    res = _run_ranks(tmp_path, "dp", [_job("3d", a, snap, "store")] * 2)
    _check_common(res, str(snap), 4)
    make = lambda: net_factory_3d(net_type="dualdecoder", in_chns=1, class_num=2, mode="train", device=DEV, args=a)
    m = _load_latest(make, str(snap))
    assert torch.equal(m.flat_buffers()[0].cpu(), res[0]["flat"])                                       # (d)
    dice = float(var_all_case(m, W.val_volumes_3d(), 2, tuple(a["patch_size"]), a["stride_xy"], a["stride_z"]))      # (e)
    assert "iteration 4 : dice_score : %f" % dice in open(os.path.join(str(snap), "log.txt")).read().splitlines()


def test_one_rank_rccl_group_equals_the_plain_run(tmp_path):
    """The only part that runs real RCCL on a one-GPU box: data_parallel + dp_force_group + nccl, 4 iterations at 64 x 64 from the synthetic loader."""
    a = dict(ARGS_2D, max_iterations=4, val_interval=2, monitor=False, mean_teacher=False)
    got = _run_ranks(tmp_path, "dp", [_job("2d", dict(a, data_parallel=True, dp_force_group=True, dp_backend="nccl"), tmp_path / "dp", "synthetic")])[0]
    plain = _run_ranks(tmp_path, "plain", [_job("2d", a, tmp_path / "plain", "synthetic")])[0]
    assert got["world"] == 1 and got["exchange"] == "module" and plain["exchange"] is None          # a group was built, and it is torch.distributed's own
    assert got["iter_num"] == plain["iter_num"] == 4
    assert torch.equal(got["flat"], plain["flat"]) and torch.equal(got["mom"], plain["mom"])
