"""Helper process of tests/test_guard_step_gpu.py (NOT a test module): one data-parallel rank of a guarded ChapStep, two of them on one GPU.

    python tests/guard_dp_worker.py --rank R --world 2 --port P --out DIR

tests/dp_worker.py's fp32 DualDecoder (state recipe 301) on the rank's own shard, every rank on cuda:0 with the gradient buckets all-reduced
through host memory (gloo, chap_amd.parallel.HostStagedDist), a StepGuard(max_norm=1e-3: far below the gradient's norm, every finite step is
clipped) attached.  Three eager iterations: (1) a clipped one; (2) device_step(update=False), then RANK 1 ALONE writes a NaN into its local
bucket 1, then exchange_and_update(): the all-reduce carries the NaN to every rank and every rank skips; (3) a clipped one again, then the
same iteration captured and replayed once (the optimizer graph of the data-parallel capture holds the two guard launches).  After each,
RankContext.assert_replicas_equal on parameters and momentum.  Saves the rank's ring rows and counters, parameters and momentum to
DIR/guard_rank<R>.pt.  A process of its own, so that a problem of the process group cannot take the test session down."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, default=29711)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from chap_amd.distributed import RankContext, replica_state
    from chap_amd.guard import StepGuard
    from chap_amd.networks import DualDecoder
    from chap_amd.parallel import DataParallelSync, HostStagedDist
    from chap_amd.train import ChapStep
    from oracle import init as oinit
    from tests import dp_worker as W
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    ctx = RankContext(a.rank, a.world, dev, HostStagedDist(dist), dist.group.WORLD)
    m = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev).train()
    m.load_state_dict(oinit.dual_decoder_2d_state(301), strict=True)
    guard = StepGuard(max_norm=1e-3, skip_nonfinite=True, ring=8, device=dev)
    step = ChapStep(m, W.args_of("2d", 1), world_size=a.world, guard=guard)
    step.iter_num = W.IT0
    step.grad_sync = DataParallelSync(step.grad_both, ctx.dist, overlap=False)
    vol, lab, inj, box = W.shard_inputs(a.rank)
    inj = {k: ({kk: vv.permute(0, 2, 3, 1).unsqueeze(1).contiguous().to(dev) for kk, vv in v.items()} if k.startswith("drop") else v.to(dev)) for k, v in inj.items()}
    vol, lab = vol.to(dev), lab.to(dev)
    snaps = []

    def check(what):
        torch.cuda.synchronize()
        ctx.assert_replicas_equal(what, replica_state(step))
        snaps.append(m.flat_buffers()[0].clone())

    # (1) clipped
    step.step(vol, lab, box_yx=box, inject=inj)
    check("parameters / momentum after the clipped step")
    # (2) skipped: the NaN is in ONE rank's gradient
    before = [t.clone() for t in replica_state(step)]
    step._hw = tuple(vol.shape[2:])
    step.prepare(box)
    step.device_step(vol, lab, inj, update=False)
    if a.rank == 1:
        step.grad2[step.grad2.numel() // 3] = float("nan")
    step.exchange_and_update()
    step.finish()
    check("parameters / momentum after the skipped step")
    unchanged = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, replica_state(step)))
    buckets_zero = float(step.grad_both.abs().max()) == 0.0
    # (3) clipped again, eager, then captured and replayed
    step.step(vol, lab, box_yx=box, inject=inj)
    check("parameters / momentum after the step behind the skipped one")
    step.capture(vol, lab, warmup=1, inject=inj)
    step.replay(vol, lab, box_yx=box)
    check("parameters / momentum after the replayed step")
    rows = {k: (torch.from_numpy(v) if hasattr(v, "dtype") else v) for k, v in guard.read().items()}
    torch.save({"rows": rows, "unchanged": unchanged, "buckets_zero": buckets_zero, "param": m.flat_buffers()[0].cpu(), "mom": step.opt.mom.cpu(),
                "moved": [not torch.equal(snaps[i], snaps[i + 1]) for i in range(len(snaps) - 1)], "iter_num": step.iter_num,
                "graphs": (step._graph is not None, step._graph_opt is not None)},
               os.path.join(a.out, "guard_rank%d.pt" % a.rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
