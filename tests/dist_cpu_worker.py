"""Helper process of tests/test_train_dp_cpu.py (NOT a test module): one CPU rank of a gloo group that exercises chap_amd.distributed.

    python tests/dist_cpu_worker.py OUT_DIR [flip]

The rank comes from the environment, as under torch.distributed.run.  Writes OUT_DIR/rank<r>.json with what the helpers returned; with `flip`,
rank 1 flips one bit of its tensor before assert_replicas_equal and every rank records the error it got."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def items():
    """Five per-item arrays whose sum depends on the order of the additions in the last bits."""
    rng = np.random.default_rng(3)
    small = [rng.standard_normal((3, 2)) for _ in range(5)]
    return [small[0] + 1e16, small[1], small[2] - 1e16, small[3], small[4]]      # item order loses item 1 in 1e16; rank order (0, 2, 4, 1, 3) keeps it


def main():
    out_dir, flip = sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "flip"
    from chap_amd.distributed import init_rank, state_digest
    ctx = init_rank({"data_parallel": True, "dp_backend": "gloo", "dp_timeout_s": 60})
    res = {"rank": ctx.rank, "world": ctx.world, "is_main": ctx.is_main}
    try:
        its = items()
        res["shard"] = ctx.shard(list(range(5)))
        got = ctx.gather_in_order([its[i] for i in ctx.shard(list(range(5)))], 5)
        res["mean_hex"] = (sum(got) / 5).tobytes().hex()
        # one item, two ranks: rank 1's shard is empty and it takes part all the same
        one = ctx.gather_in_order([its[0]] if ctx.rank == 0 else [], 1)
        res["one_item_equal"] = bool(len(one) == 1 and np.array_equal(one[0], its[0]))
        # broadcast_module_state: rank 0's parameters and buffers everywhere
        torch.manual_seed(100 + ctx.rank)
        m = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
        m[1].running_mean.add_(ctx.rank + 0.5)
        ctx.broadcast_module_state(m)
        res["module_digest"] = state_digest(list(m.parameters()) + list(m.buffers()))
        ctx.assert_replicas_equal("the broadcast module", list(m.parameters()) + list(m.buffers()))
        t = torch.arange(64, dtype=torch.float32) * 0.37
        res["digest"] = state_digest(t)
        if flip and ctx.rank == 1:
            t.view(torch.int32)[17] ^= 1
        try:
            ctx.assert_replicas_equal("the tensor", [t])
            res["error"] = None
        except RuntimeError as e:
            res["error"] = str(e)
        ctx.barrier()
    finally:
        ctx.close()
    with open(os.path.join(out_dir, "rank%d.json" % res["rank"]), "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
