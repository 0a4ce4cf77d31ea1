"""Helper process of tests/test_teacher_uncertainty_step_gpu.py (NOT a test module): one data-parallel rank of a ChapStep with a mean teacher,
its consistency term and the uncertainty mask over T = 2 noisy teacher passes, two of them on one GPU.

    python tests/teacher_uncertainty_dp_worker.py --rank R --world 2 --port P --out DIR

tests/adam_dp_worker.py's set-up: tests/dp_worker.py's fp32 DualDecoder (state recipe 301) on the rank's own shard, every rank on cuda:0 with
the gradient buckets all-reduced through host memory (gloo, chap_amd.parallel.HostStagedDist).  The teacher's noise is drawn, not injected,
from the rank's own stream (engine.Rng.rebase, what distributed.attach_step does under dp_noise_per_rank).  Three eager iterations, each under
a time limit of its own; after each, RankContext.assert_replicas_equal on distributed.replica_state: parameters, momentum and the teacher.
Each rank normalises its term by its own count of certain pixels (no collective in pass B); the gradient exchange averages the two terms.
Saves the replicated state, the six noise tensors, the teacher losses and the counts to DIR/tu_rank<R>.pt.  A process of its own, so that a problem of the process group
cannot take the test session down."""
import argparse
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

STEP_LIMIT_S = 90


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, default=29611)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from chap_amd import ops
    from chap_amd.distributed import RankContext, replica_state
    from chap_amd.networks import DualDecoder
    from chap_amd.parallel import DataParallelSync, HostStagedDist
    from chap_amd.train import ChapStep, build_teacher
    from oracle import init as oinit
    from tests import dp_worker as W
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    ctx = RankContext(a.rank, a.world, dev, HostStagedDist(dist), dist.group.WORLD)
    m = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev).train()
    m.load_state_dict(oinit.dual_decoder_2d_state(301), strict=True)

    def make():
        torch.manual_seed(77)
        return DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev)

    step = ChapStep(m, dict(W.args_of("2d", 1), teacher_consistency=0.7, teacher_noise=0.1, teacher_uncertainty=2), world_size=a.world, teacher=build_teacher(make).eval())
    assert len(replica_state(step)) == 3
    step.iter_num = W.IT0
    step.grad_sync = DataParallelSync(step.grad_both, ctx.dist, overlap=False)
    m._rng.rebase(m._rng.base, a.rank)
    vol, lab, inj, box = W.shard_inputs(a.rank)
    inj = {k: ({kk: vv.permute(0, 2, 3, 1).unsqueeze(1).contiguous().to(dev) for kk, vv in v.items()} if k.startswith("drop") else v.to(dev)) for k, v in inj.items()}
    vol, lab = vol.to(dev), lab.to(dev)
    noise, real_rand = [], ops.rand_uniform

    def rand(out, seed, lo=0.0, hi=1.0, seed_dev=None):
        real_rand(out, seed, lo, hi, seed_dev)
        if lo == -0.1 and hi == 0.1:
            noise.append(out.clone())

    ops.rand_uniform = rand

    def too_long(signum, frame):
        raise TimeoutError("a data-parallel step took more than %d s" % STEP_LIMIT_S)

    signal.signal(signal.SIGALRM, too_long)
    losses, counts = [], []
    for k in range(3):
        signal.alarm(STEP_LIMIT_S)
        out = step.step(vol, lab, box_yx=box, inject=inj)
        torch.cuda.synchronize()
        ctx.assert_replicas_equal("parameters / momentum / teacher after step %d" % (k + 1), replica_state(step))
        signal.alarm(0)
        losses.append(float(out["teacher_loss"]))
        counts.append(int(out["teacher_certain"]))
    torch.save({"param": m.flat_buffers()[0].cpu(), "mom": step.opt.mom.cpu(), "ema": step.opt.ema.cpu(), "iter_num": step.iter_num, "it0": W.IT0,
                "noise": [u.cpu() for u in noise], "teacher_loss": losses, "teacher_certain": counts,
                "pixels": step.teacher_pixels}, os.path.join(a.out, "tu_rank%d.pt" % a.rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
