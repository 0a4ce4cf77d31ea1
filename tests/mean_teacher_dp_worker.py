"""Helper process of tests/test_mean_teacher_step_gpu.py (NOT a test module): tests/dp_worker.py's one-rank iteration with a mean teacher.

    python tests/mean_teacher_dp_worker.py --out DIR [--port P]

The fp32 DualDecoder of dp_worker (state recipe 301, rank 0's shard), a teacher with weights of its own, the captured iteration replayed
twice from iteration 3000 (alpha = 0.99 both times): first as the plain one-graph step (DIR/nodp.pt), then through a 1-rank RCCL group with the
overlap schedule (four graphs, the optimizer's last; DIR/dp.pt), the flat buffers saved.  A process of its own, so that an RCCL problem cannot take the
test session down."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def run(dp, dev, out_dir):
    from chap_amd.networks import DualDecoder
    from chap_amd.parallel import DataParallelSync
    from chap_amd.train import ChapStep, build_teacher
    from oracle import init as oinit
    from tests import dp_worker as W
    m = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev).train()
    m.load_state_dict(oinit.dual_decoder_2d_state(301), strict=True)

    def make():
        torch.manual_seed(77)
        return DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(dev)

    step = ChapStep(m, W.args_of("2d", 1), world_size=1, teacher=build_teacher(make).eval())
    step.iter_num = W.IT0
    ema0 = step.opt.ema.clone()
    if dp:
        step.grad_sync = DataParallelSync(step.grad_both, dist, overlap=True)
    vol, lab, inj, box = W.shard_inputs(0)
    inj = {k: ({kk: vv.permute(0, 2, 3, 1).unsqueeze(1).contiguous().to(dev) for kk, vv in v.items()} if k.startswith("drop") else v.to(dev)) for k, v in inj.items()}
    vol, lab = vol.to(dev), lab.to(dev)
    step.capture(vol, lab, warmup=1, inject=inj)
    for _ in range(2):
        out = step.replay(vol, lab, box_yx=box)
    torch.cuda.synchronize()
    torch.save({"param": m.flat_buffers()[0].cpu(), "mom": step.opt.mom.cpu(), "ema": step.opt.ema.cpu(), "ema0": ema0.cpu(), "buckets": step.grad_both.cpu(),
                "losses": torch.cat([l.reshape(-1).cpu() for l in out["mix_losses"]] + [out["vat_loss"].reshape(-1).cpu()]), "iter_num": step.iter_num,
                "graphs": 4 if step._graphs_dp is not None else 1},
               os.path.join(out_dir, "dp.pt" if dp else "nodp.pt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--port", type=int, default=29533)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    run(False, dev, a.out)                      # the plain step first: no process group exists yet
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    run(True, dev, a.out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
