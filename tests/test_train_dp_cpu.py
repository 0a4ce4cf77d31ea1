"""The host side of the data-parallel train() (no GPU): the rank-sharded draws of DeviceLoader against the world-1 loader of the global batch,
byte for byte; chap_amd.distributed's helpers in a gloo group of two CPU processes (tests/dist_cpu_worker.py); monitor.merge_rows against the
rows of the whole batch; the launcher (python -m chap_amd.launch) in its dry run.  Every child process is a fresh one under a timeout of its own,
on a free port; after a non-zero exit the test fails at once."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from chap_amd.data import DeviceLoader, SliceStore, VolumeStore
from tests import monitor_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- sharded draws
def _store(dims):
    """Host-resident, draw-only stores.  2D: 11 labelled + 13 unlabelled ragged slices; 3D: volumes smaller and larger than the patch (8, 8, 4)."""
    rng = np.random.default_rng(2)
    if dims == 2:
        shapes = [(17, 19), (23, 16), (16, 16), (31, 18), (20, 20), (16, 29), (25, 25), (18, 17), (33, 16), (16, 21), (22, 22),
                  (19, 30), (17, 17), (26, 16), (16, 24), (21, 18), (30, 30), (18, 27), (24, 19), (16, 18), (27, 23), (20, 16), (29, 17), (23, 23)]
        st = SliceStore([rng.random(s) for s in shapes], [rng.integers(0, 4, s).astype(np.uint8) for s in shapes], "cpu")
        return st, 11, (16, 16), {}
    shapes = [(8, 8, 4), (6, 9, 3), (12, 10, 6), (5, 5, 2), (10, 12, 8), (9, 7, 5), (16, 8, 4), (8, 13, 7), (7, 7, 7), (11, 9, 4), (8, 8, 9), (13, 13, 5),
              (20, 18, 9), (4, 16, 4), (9, 9, 9), (14, 6, 3)]
    st = VolumeStore([rng.random(s) for s in shapes], [rng.integers(0, 2, s).astype(np.uint8) for s in shapes], "cpu")
    return st, 7, (8, 8, 4), dict(pad=True)


def _raw(recs):
    return ctypes.string_at(ctypes.addressof(recs), ctypes.sizeof(recs))


def _draw_sequence(ld, n):
    """n batches of the endless sequence, as next_into walks it: (record bytes, draws) per batch."""
    out = []
    for _ in range(n):
        recs, draws = ld._draw(next(ld._endless))
        out.append((_raw(recs), draws, list(ld.last_global_indices)))
    return out


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_rank_draws_concatenate_to_the_global_loaders(dims, world):
    st, n_lab, out, extra = _store(dims)
    B, lbs = (2, 1)
    mk = lambda b, l, **rw: DeviceLoader(st, range(n_lab), range(n_lab, len(st)), b, l, out, seed=5, **extra, **rw)
    glob = mk(world * B, world * lbs)
    ranks = [mk(B, lbs, rank=r, world=world) for r in range(world)]
    assert len(glob) == n_lab // (world * lbs) and all(len(x) == len(glob) for x in ranks)
    n = 2 * len(glob) + 1                                   # epochs turn over
    want, got = _draw_sequence(glob, n), [_draw_sequence(x, n) for x in ranks]
    size = ctypes.sizeof(glob._rec_t)
    for k in range(n):
        raw, draws, idxs = want[k]
        assert len(raw) == world * B * size
        cat = b"".join(got[r][k][0][:lbs * size] for r in range(world)) + b"".join(got[r][k][0][lbs * size:] for r in range(world))
        assert cat == raw, (k, "records")
        assert [d for r in range(world) for d in got[r][k][1][:lbs]] + [d for r in range(world) for d in got[r][k][1][lbs:]] == draws, (k, "last_draws")
        assert all(got[r][k][2] == idxs for r in range(world))
        assert [d["index"] for d in draws] == idxs


@pytest.mark.parametrize("dims", [2, 3])
def test_without_the_new_arguments_the_loader_is_todays(dims):
    st, n_lab, out, extra = _store(dims)
    a = DeviceLoader(st, range(n_lab), range(n_lab, len(st)), 4, 2, out, seed=9, **extra)
    b = DeviceLoader(st, range(n_lab), range(n_lab, len(st)), 4, 2, out, seed=9, rank=0, world=1, **extra)
    assert (a.rank, a.world) == (0, 1) and len(a) == len(b) == n_lab // 2
    n = 2 * len(a) + 1
    for (ra, da, _), (rb, db, _) in zip(_draw_sequence(a, n), _draw_sequence(b, n)):
        assert ra == rb and da == db
    # and today's loader is: the sampler of (batch_size, batch_size - labeled_bs) under the seed, the draw stream [seed, 1]
    from chap_amd.data import TwoStreamBatchSampler
    s = TwoStreamBatchSampler(range(n_lab), range(n_lab, len(st)), 4, 2, 9)
    c = DeviceLoader(st, range(n_lab), range(n_lab, len(st)), 4, 2, out, seed=9, **extra)
    for idxs in s:
        _, draws = c._draw(next(c._endless))
        assert c.last_global_indices == [int(i) for i in idxs] and [d["index"] for d in draws] == c.last_global_indices


def test_loader_refuses_a_bad_rank_and_too_few_labelled_items():
    st, n_lab, out, _ = _store(2)
    for rank, world in ((2, 2), (-1, 2), (0, 0), (1, 1)):
        with pytest.raises(ValueError, match="rank"):
            DeviceLoader(st, range(n_lab), range(n_lab, len(st)), 4, 2, out, rank=rank, world=world)
    with pytest.raises(ValueError, match="primary"):
        DeviceLoader(st, range(n_lab), range(n_lab, len(st)), 4, 2, out, rank=0, world=6)       # 12 labelled per global batch, 11 there


def test_rng_rebase_keeps_rank_zero():
    from chap_amd.engine import Rng
    r = Rng(1337, "cpu")
    base = r.base
    r.rebase(1337, 0)
    assert r.base == base == 1337
    r.rebase(1337, 3)
    assert r.base == (1337 + 3 * 0x9E3779B1) & 0xFFFFFFFF and r.base != base
    r.rebase(0xFFFFFFFF, 1)
    assert 0 <= r.base <= 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- chap_amd.distributed over gloo, two CPU processes
def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_cpu_ranks(tmp_path, *extra):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_cpu_worker.py"), str(tmp_path)] + list(extra), env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    try:
        for p in procs:
            out, _ = p.communicate(timeout=120)
            assert p.returncode == 0, out.decode(errors="replace")[-4000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return [json.load(open(os.path.join(str(tmp_path), "rank%d.json" % r))) for r in range(2)]


def test_helpers_in_a_gloo_group_of_two(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_cpu_worker as DW
    from chap_amd.distributed import state_digest
    res = _two_cpu_ranks(tmp_path)
    its = DW.items()
    want = (sum(its) / 5).tobytes().hex()                   # the single process: the items in order
    assert [r["shard"] for r in res] == [[0, 2, 4], [1, 3]] and [r["is_main"] for r in res] == [True, False]
    assert [r["mean_hex"] for r in res] == [want, want]
    assert want != (sum(its[::2] + its[1::2]) / 5).tobytes().hex()      # (the check has teeth: rank order would not give these bits)
    assert all(r["one_item_equal"] for r in res)
    assert res[0]["module_digest"] == res[1]["module_digest"]
    assert res[0]["digest"] == res[1]["digest"] == state_digest(torch.arange(64, dtype=torch.float32) * 0.37)
    assert [r["error"] for r in res] == [None, None]


def test_one_flipped_bit_raises_on_every_rank_and_names_the_rank(tmp_path):
    res = _two_cpu_ranks(tmp_path, "flip")
    for r in res:
        assert r["error"] is not None and "the tensor" in r["error"] and "rank 1 against rank 0" in r["error"], r["error"]


def test_state_digest_is_a_wrapping_sum_of_the_raw_bits():
    from chap_amd.distributed import state_digest
    t = torch.tensor([1.0, -2.5, 0.0, 3e38], dtype=torch.float32)
    bits = np.frombuffer(t.numpy().tobytes(), dtype=np.int32).astype(object)
    assert state_digest(t) == int(sum(bits)) % (1 << 64)
    big = torch.full((3,), 0x7FFFFFFFFFFFFFFF, dtype=torch.int64)
    assert state_digest(big) == (3 * 0x7FFFFFFFFFFFFFFF) % (1 << 64)        # wraps, does not saturate
    assert state_digest([t, big]) == (state_digest(t) + state_digest(big)) % (1 << 64)
    u = t.clone()
    u.view(torch.int32)[1] ^= 1
    assert state_digest(u) != state_digest(t)
    assert state_digest([torch.tensor([True, False, True]), torch.ones(2, dtype=torch.bfloat16)]) == 2 + 2 * 0x3F80


def test_plain_context_ignores_the_environment():
    from chap_amd.distributed import init_rank
    env = dict(RANK="3", WORLD_SIZE="8", LOCAL_RANK="3")
    for a in ({}, {"data_parallel": False, "gpu": 0}):
        ctx = init_rank(a, environ=env)
        assert (ctx.rank, ctx.world, ctx.is_main, ctx.group, ctx.dist) == (0, 1, True, None, None) and ctx.device == torch.device("cuda", 0)
        assert ctx.shard([5, 6, 7]) == [5, 6, 7] and ctx.gather_in_order([1.5, 2.5], 2) == [1.5, 2.5]
        ctx.barrier()
        ctx.close()
    ctx = init_rank({"data_parallel": True}, environ={})                    # WORLD_SIZE unset, no dp_force_group: no group at all
    assert ctx.group is None and ctx.world == 1
    with pytest.raises(ValueError, match="dp_backend"):
        init_rank({"data_parallel": True, "dp_backend": "mpi"}, environ=env)


# ---------------------------------------------------------------------------------------------------- monitor.merge_rows
def test_merge_rows_of_two_halves_is_the_whole_batch():
    from chap_amd.monitor import StepMonitor, merge_rows
    rng = np.random.default_rng(8)
    C, P, lbs, ubs = 4, 97, 2, 3                            # per rank: 2 labelled + 3 unlabelled samples of 97 pixels
    halves, scal = [], []
    for r in range(2):
        l1, l2 = mr.quantised_logits(rng, (lbs + ubs, C, P)), mr.quantised_logits(rng, (lbs + ubs, C, P))
        lab = rng.integers(0, C, (lbs + ubs, P))
        maps = [rng.integers(0, C, (lbs + ubs, P)) for _ in range(2)]
        halves.append((l1, l2, lab, maps))
        scal.append(rng.random((3, 16)))
    parts = []
    for r, (l1, l2, lab, maps) in enumerate(halves):
        rows = mr.stack_rows([mr.row_ref(l1, l2, lab, lbs, maps)] * 3, iterations=[4, 5, 6], scalars=scal[r])
        rows.update(dropped=r, scalar_layout="chap")
        parts.append(rows)
    cat = lambda j: np.concatenate([halves[0][j][:lbs], halves[1][j][:lbs], halves[0][j][lbs:], halves[1][j][lbs:]])
    whole = mr.row_ref(cat(0), cat(1), cat(2), 2 * lbs, [np.concatenate([halves[0][3][h][:lbs], halves[1][3][h][:lbs], halves[0][3][h][lbs:], halves[1][3][h][lbs:]])
                                                         for h in range(2)])
    got = merge_rows(parts)
    assert got["iteration"].tolist() == [4, 5, 6] and got["dropped"] == 1 and got["scalar_layout"] == "chap"
    for name in mr.COUNT_FIELDS + ("inter_f", "pred_f"):
        assert np.array_equal(got[name], np.stack([whole[name]] * 3)), name                 # counts: exactly the whole batch's
    for name in ("conf_correct", "conf_err"):
        want = np.stack([whole[name]] * 3)
        assert (np.abs(got[name] - want) <= 1e-12 * np.abs(want)).all(), name               # fp64 sums in another order
    assert np.array_equal(got["scalars"], (scal[0] + scal[1]) / 2)
    d = StepMonitor.derive(got)
    assert d["iteration"].tolist() == [4, 5, 6] and np.isfinite(d["accuracy"]).all()
    one = merge_rows(parts[:1])
    assert all(np.array_equal(one[k], parts[0][k]) for k in mr.COUNT_FIELDS + ("scalars", "conf_correct", "iteration"))
    parts[1]["iteration"] = np.array([4, 5, 7])
    with pytest.raises(ValueError, match="iterations"):
        merge_rows(parts)
    parts[1]["iteration"] = np.array([4, 5])
    with pytest.raises(ValueError, match="iterations"):
        merge_rows(parts)


# ---------------------------------------------------------------------------------------------------- the launcher
def _launch(*argv, timeout=120):
    return subprocess.run([sys.executable, "-m", "chap_amd.launch"] + [str(a) for a in argv], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def test_launcher_dry_run_with_two_ranks(tmp_path):
    p = _launch("--nproc", 2, "--entry", "2d", "--snapshot", tmp_path, "--dry-run", "--timeout", 60)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-4000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == {"dry_run": True, "entry": "2d", "world": 2, "snapshot": str(tmp_path)}      # rank 0 alone reports


def test_launcher_returns_a_failed_ranks_status_and_leaves_no_child(tmp_path):
    """Rank 1 exits with status 3 before the rendezvous; rank 0 would wait there for --timeout.  The launcher must come back long before that, with a
    non-zero status, and with its children gone: they share its stderr pipe, so its end-of-file is reached only once every child has exited."""
    p = subprocess.Popen([sys.executable, "-m", "chap_amd.launch", "--nproc", "2", "--entry", "3d", "--snapshot", str(tmp_path), "--dry-run",
                          "--timeout", "60", "--dry-run-fail-rank", "1"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        out, err = p.communicate(timeout=45)                # returns at end-of-file of both pipes: no child holds them any more
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert p.returncode == 3, err.decode(errors="replace")[-4000:]
    assert b"rank 1 exited with status 3" in err and not [ln for ln in out.decode().splitlines() if ln.startswith("{")]


def test_launcher_refuses_17_ranks_before_anything_starts(tmp_path, monkeypatch):
    p = _launch("--nproc", 17, "--entry", "2d", "--snapshot", tmp_path)
    assert p.returncode != 0 and b"--nproc 17" in p.stderr and not os.listdir(str(tmp_path))
    from chap_amd import launch as LA
    started = []
    monkeypatch.setattr(LA.subprocess, "Popen", lambda *a, **k: started.append(a) or (_ for _ in ()).throw(AssertionError("started a process")))
    with pytest.raises(SystemExit, match="--nproc 17"):
        LA.main(["--nproc", "17", "--entry", "2d", "--snapshot", str(tmp_path), "--dry-run"])
    assert not started
