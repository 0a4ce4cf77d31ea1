"""Helper process of tests/test_adam_step_gpu.py (NOT a test module): one data-parallel rank of a ChapStep with the fused AdamW, two of them on
one GPU.

    python tests/adam_dp_worker.py --rank R --world 2 --port P --out DIR

tests/guard_dp_worker.py's set-up: tests/dp_worker.py's fp32 DualDecoder (state recipe 301) on the rank's own shard, every rank on cuda:0 with
the gradient buckets all-reduced through host memory (gloo, chap_amd.parallel.HostStagedDist).  The optimizer is FusedAdamW (args
optimizer='adamw') with a StepGuard attached.  Three eager iterations; the guard's max_norm is 1e30 for the first and the third and 1e-3 -- far
below the gradient's norm -- for the second, which is therefore clipped.  After each, RankContext.assert_replicas_equal on
distributed.replica_state: parameters, both moments and the state block.  Saves them and the ring rows to DIR/adam_rank<R>.pt.  A process of
its own, so that a problem of the process group cannot take the test session down."""
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
    ap.add_argument("--port", type=int, default=29811)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from chap_amd.distributed import RankContext, replica_state
    from chap_amd.guard import StepGuard
    from chap_amd.networks import DualDecoder
    from chap_amd.parallel import DataParallelSync, HostStagedDist
    from chap_amd.train import ChapStep, FusedAdamW
    from oracle import init as oinit
    from tests import dp_worker as W
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    ctx = RankContext(a.rank, a.world, dev, HostStagedDist(dist), dist.group.WORLD)
    m = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev).train()
    m.load_state_dict(oinit.dual_decoder_2d_state(301), strict=True)
    guard = StepGuard(max_norm=1e30, skip_nonfinite=True, ring=8, device=dev)
    step = ChapStep(m, dict(W.args_of("2d", 1), optimizer="adamw", base_lr=1e-3, weight_decay=1e-2), world_size=a.world, guard=guard)
    assert isinstance(step.opt, FusedAdamW) and len(replica_state(step)) == 4
    step.iter_num = W.IT0
    step.grad_sync = DataParallelSync(step.grad_both, ctx.dist, overlap=False)
    vol, lab, inj, box = W.shard_inputs(a.rank)
    inj = {k: ({kk: vv.permute(0, 2, 3, 1).unsqueeze(1).contiguous().to(dev) for kk, vv in v.items()} if k.startswith("drop") else v.to(dev)) for k, v in inj.items()}
    vol, lab = vol.to(dev), lab.to(dev)
    snaps = [m.flat_buffers()[0].clone()]
    for k, max_norm in enumerate((1e30, 1e-3, 1e30)):
        guard.max_norm = max_norm
        step.step(vol, lab, box_yx=box, inject=inj)
        torch.cuda.synchronize()
        ctx.assert_replicas_equal("parameters / moments / state block after step %d" % (k + 1), replica_state(step))
        snaps.append(m.flat_buffers()[0].clone())
    rows = {k: (torch.from_numpy(v) if hasattr(v, "dtype") else v) for k, v in guard.read().items()}
    torch.save({"rows": rows, "param": m.flat_buffers()[0].cpu(), "exp_avg": step.opt.exp_avg.cpu(), "exp_avg_sq": step.opt.exp_avg_sq.cpu(),
                "state": step.opt.state.cpu(), "moved": [not torch.equal(snaps[i], snaps[i + 1]) for i in range(len(snaps) - 1)]},
               os.path.join(a.out, "adam_rank%d.pt" % a.rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
