"""The rank layer of a data-parallel train(): process groups, shards, and the host-side exchanges around validation and file writes.

`init_rank(args)` reads the contract of `torch.distributed.run` (RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT) when
`args["data_parallel"]` is set and returns a RankContext; without it the context is the plain single process (no group, whatever the
environment says).  Two groups exist side by side: the GRADIENT group (`ctx.dist`, what parallel.DataParallelSync all-reduces through: RCCL, or
gloo behind parallel.HostStagedDist for the one-GPU rehearsal) and a HOST group (`ctx.group`, gloo) for everything else -- validation
metrics, monitor rows, state digests, barriers around file writes.  Nothing the host group does touches a GPU stream or a captured graph.

DESIGN.md section 6 "train() on several ranks" has the rules (shard, noise, validation order) and what is verified."""
import datetime
import os

import torch


class RankContext:
    """rank, world, device, dist (the gradient exchange's `torch.distributed`-like object, None without a group), group (the host-side gloo
    group, None without one), is_main (rank 0: the one that writes files)."""

    def __init__(self, rank=0, world=1, device=None, dist=None, group=None):
        self.rank, self.world, self.device, self.dist, self.group = int(rank), int(world), device, dist, group
        self.is_main = self.rank == 0

    # ---- shards
    def shard(self, seq):
        """The items of `seq` this rank works on: seq[rank::world] (item i belongs to rank i % world)."""
        return seq if self.world == 1 else seq[self.rank::self.world]

    def gather_objects(self, obj):
        """[obj of rank 0, obj of rank 1, ...] on every rank (pickled over the host group: bits are preserved)."""
        if self.group is None:
            return [obj]
        import torch.distributed as dist
        out = [None] * self.world
        dist.all_gather_object(out, obj, group=self.group)
        return out

    def gather_in_order(self, per_item_values, n_items):
        """`per_item_values`: this rank's values for shard(range(n_items)), in that order.  Returns the n_items values in ITEM order, the same
        list on every rank: a sum or mean taken over it is bit-identical to the one of a single process that visits the items in order.  A rank
        whose shard is empty passes [] and takes part all the same."""
        mine = list(per_item_values)
        want = len(range(self.rank, n_items, self.world))
        if len(mine) != want:
            raise ValueError("chap_amd.distributed: rank %d of %d holds %d values for its %d of %d items" % (self.rank, self.world, len(mine), want, n_items))
        parts = self.gather_objects(mine)
        return [parts[i % self.world][i // self.world] for i in range(n_items)]

    def barrier(self):
        if self.group is not None:
            import torch.distributed as dist
            dist.barrier(group=self.group)

    # ---- replicas
    def _broadcast(self, tensors, src):
        if self.group is None:
            return
        import torch.distributed as dist
        with torch.no_grad():
            for t in tensors:
                c = t.detach().cpu().contiguous()           # through host memory: the host group is a CPU group
                dist.broadcast(c, src, group=self.group)
                if self.rank != src:
                    t.copy_(c)

    def broadcast_module_state(self, module, src=0):
        """Rank `src`'s parameters and buffers into every replica, in place (flat-buffer views stay views)."""
        self._broadcast(list(module.parameters()) + list(module.buffers()), src)
        if hasattr(module, "mark_params_dirty"):
            module.mark_params_dirty()

    def broadcast_buffers(self, module, src=0):
        """Rank `src`'s buffers (BatchNorm running statistics) into every replica: DDP's broadcast_buffers, done where they are read."""
        self._broadcast(list(module.buffers()), src)
        if hasattr(module, "mark_params_dirty"):
            module.mark_params_dirty()

    def assert_replicas_equal(self, name, tensors):
        """Raises on EVERY rank when the ranks' state_digest(tensors) differ, naming the ranks that differ from rank 0."""
        digests = self.gather_objects(state_digest(tensors))
        bad = [r for r, d in enumerate(digests) if d != digests[0]]
        if bad:
            raise RuntimeError("chap_amd.distributed: replicas differ in %s: rank%s %s against rank 0 (digests by rank: %s)"
                               % (name, "s" if len(bad) > 1 else "", ", ".join(str(r) for r in bad), ", ".join("%016x" % d for d in digests)))

    def close(self):
        """Leave the process groups (idempotent; the plain context has none)."""
        if self.group is not None:
            import torch.distributed as dist
            self.group, self.dist = None, None
            if dist.is_initialized():
                dist.destroy_process_group()


_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def state_digest(tensors):
    """64-bit wrap-around sum of the raw bits of `tensors` (a tensor or an iterable of them), as a Python int in [0, 2^64): every element
    taken as the signed integer of its own width, added in int64 (which wraps).  Cheap and order-blind: it tells replicas apart that drifted,
    it is no hash."""
    if isinstance(tensors, torch.Tensor):
        tensors = [tensors]
    total = 0
    for t in tensors:
        t = t.detach().contiguous().reshape(-1)
        if t.numel() == 0:
            continue
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        total += int(t.view(_INT_VIEW[t.element_size()]).to(torch.int64).sum().item())
    return total & 0xFFFFFFFFFFFFFFFF


def rank_environment(environ=None):
    """(rank, world, local_rank) from the environment of torch.distributed.run; (0, 1, 0) where it is not set."""
    env = os.environ if environ is None else environ
    world = int(env.get("WORLD_SIZE", "1"))
    rank = int(env.get("RANK", "0"))
    return rank, world, int(env.get("LOCAL_RANK", str(rank)))


def init_rank(a, environ=None):
    """a["data_parallel"] falsy: the plain context (cuda:a["gpu"], no group), whatever RANK / WORLD_SIZE say.  Otherwise the rank of the
    environment; a["dp_backend"] "nccl" (default): device cuda:LOCAL_RANK, RCCL group; "gloo": the one-GPU rehearsal, every rank on
    cuda:a["gpu"], gradients through parallel.HostStagedDist.  WORLD_SIZE unset or 1 gives no group unless a["dp_force_group"] asks for the
    1-rank one.  a["dp_timeout_s"] (600): the groups' timeout.  The gloo and plain paths never touch the GPU (a device OBJECT only: the helpers run on a CPU-only box); the
    nccl path selects its device, which the RCCL group is bound to."""
    gpu = int(a.get("gpu", 0))
    if not a.get("data_parallel"):
        return RankContext(device=torch.device("cuda", gpu))
    env = os.environ if environ is None else environ
    rank, world, local = rank_environment(env)
    backend = a.get("dp_backend", "nccl")
    if backend not in ("nccl", "gloo"):
        raise ValueError("chap_amd.distributed: dp_backend=%r (nccl or gloo)" % (backend,))
    if world < 1 or not 0 <= rank < world:
        raise ValueError("chap_amd.distributed: RANK=%d outside [0, WORLD_SIZE=%d)" % (rank, world))
    device = torch.device("cuda", gpu if backend == "gloo" else local)
    if world == 1 and not a.get("dp_force_group"):
        return RankContext(device=device)
    for k in ("MASTER_ADDR", "MASTER_PORT"):
        if k not in env:
            raise RuntimeError("chap_amd.distributed: data_parallel needs %s in the environment (python -m chap_amd.launch or torch.distributed.run set it)" % k)
    import torch.distributed as dist
    timeout = datetime.timedelta(seconds=float(a.get("dp_timeout_s", 600)))
    kw = dict(rank=rank, world_size=world, timeout=timeout, init_method="tcp://%s:%s" % (env["MASTER_ADDR"], env["MASTER_PORT"]))
    if backend == "gloo":
        from .parallel import HostStagedDist
        dist.init_process_group("gloo", **kw)
        xdist = HostStagedDist(dist)
    else:
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", device_id=device, **kw)
        xdist = dist
    group = dist.new_group(backend="gloo", timeout=timeout)
    return RankContext(rank, world, device, xdist, group)



# ---------------------------------------------------------------------- what the train() entries do with a context
def attach_step(ctx, step, a):
    """Make `step` (train.ChapStep, built with world_size=ctx.world) one replica of the run: identical initial weights on all ranks (rank 0's,
    broadcast and checked), the fold-schedule gradient exchange, and -- a["dp_noise_per_rank"], default on -- a dropout / VAT noise stream of
    the rank's own (engine.Rng.rebase; rank 0 keeps the single-process stream).  Before the first step or capture."""
    if ctx.group is None:
        return
    from .parallel import DataParallelSync
    model = step.model
    ctx.broadcast_module_state(model)
    if step.teacher is not None:
        ctx.broadcast_module_state(step.teacher)
    ctx.assert_replicas_equal("the initial parameters", replica_state(step))
    step.grad_sync = DataParallelSync(step.grad_both, ctx.dist, overlap=False)
    if a.get("dp_noise_per_rank", True):
        model._rng.rebase(model._rng.base, ctx.rank)


def replica_state(step):
    """What must be bitwise equal on all ranks after every update: flat parameters, the optimizer's state (SGD: momentum; Adam: both moments
    and the state block with its step counter) and, with a mean teacher, its average."""
    t = [step.model.flat_buffers()[0]] + list(step.opt.state_tensors())
    if step.teacher is not None:
        t.append(step.opt.ema)
    return t


def sync_for_validation(ctx, step):
    """Head of a validation interval: the replicas must agree (else raise on every rank), then rank 0's BatchNorm running statistics go into
    every replica, so that every rank scores its shard of the validation set with the model rank 0 saves."""
    if ctx.group is None:
        return
    ctx.assert_replicas_equal("parameters / momentum / ema at iteration %d" % step.iter_num, replica_state(step))
    ctx.broadcast_buffers(step.model)


def flush_monitor(ctx, monitor, snapshot_path, log):
    """monitor.flush_to_run for a run of ctx.world ranks: every rank reads its ring, rank 0 merges the rows (monitor.merge_rows) and writes."""
    from . import monitor as M
    if ctx.group is None:
        return M.flush_to_run(monitor, snapshot_path, log)
    parts = ctx.gather_objects(monitor.read())
    if ctx.is_main:
        M.write_rows(M.merge_rows(parts), snapshot_path, log)
