"""python -m chap_amd.launch --nproc N --entry {2d,3d} --snapshot DIR [--args FILE.json] [--set k=v ...] [--one-gpu] [--timeout S] [--dry-run]

Starts the N ranks of one data-parallel train() (chap_amd.train_ours_2D / train_ours_3D with args["data_parallel"]) on this node, one fresh
process per rank with the environment `torch.distributed.run` would give it (RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT), and
watches them: when one exits non-zero the others -- which would wait in a rendezvous or a collective -- are stopped and that status is
returned; `--timeout` bounds the whole run (status 124).  The parent never touches the GPU and never replaces its own program; the port is a
free one (bound as port 0 on 127.0.0.1, then released), never a fixed one.

`--args FILE.json`: the args dict of train(); `--set k=v`: single entries on top, v parsed as JSON where it parses (`--set max_iterations=200`,
`--set image_size=[256,256]`), as a string otherwise.  `--one-gpu`: dp_backend="gloo", every rank on cuda:`gpu` with the gradients exchanged
through host memory (a rehearsal of the rank logic on a one-GPU box, not a way to train).  `--dry-run`: the rank plumbing alone on the CPU
(gloo rendezvous, shard / gather / digest / barrier of chap_amd.distributed, no GPU, no model).

Under `torch.distributed.run` no launcher is needed: the started script calls train({..., "data_parallel": True}, snapshot) itself."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

MAX_RANKS = 16          # processes with the GPU open at once on one node


def free_port():
    """A TCP port nobody listens on right now: bound as port 0 on 127.0.0.1, read back, released."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def parse_set(items):
    out = {}
    for kv in items or []:
        if "=" not in kv:
            raise SystemExit("chap_amd.launch: --set expects k=v, got %r" % kv)
        k, v = kv.split("=", 1)
        try:
            out[k] = json.loads(v)
        except ValueError:
            out[k] = v
    return out


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m chap_amd.launch", description="start the ranks of one data-parallel train() on this node")
    ap.add_argument("--nproc", type=int, required=True, help="number of ranks (<= %d)" % MAX_RANKS)
    ap.add_argument("--entry", choices=["2d", "3d"], required=True)
    ap.add_argument("--snapshot", required=True, help="the run's output directory (rank 0 writes it)")
    ap.add_argument("--args", dest="args_file", default=None, help="JSON file with the args dict of train()")
    ap.add_argument("--set", dest="sets", action="append", default=[], metavar="k=v")
    ap.add_argument("--one-gpu", action="store_true", help="all ranks on one GPU, gradients through host memory (gloo): a rehearsal")
    ap.add_argument("--timeout", type=float, default=0.0, help="seconds for the whole run; 0 = none")
    ap.add_argument("--dry-run", action="store_true", help="the rank plumbing on the CPU: no GPU, no model")
    ap.add_argument("--dry-run-fail-rank", type=int, default=-1, help="(dry run) this rank exits with status 3 before the rendezvous")
    ap.add_argument("--rank-process", action="store_true", help=argparse.SUPPRESS)      # set by the parent on the ranks it starts
    return ap


def train_args(o):
    a = {}
    if o.args_file:
        with open(o.args_file) as f:
            a = json.load(f)
        if not isinstance(a, dict):
            raise SystemExit("chap_amd.launch: %s does not hold a JSON object" % o.args_file)
    a.update(parse_set(o.sets))
    a["data_parallel"] = True
    if o.one_gpu:
        a["dp_backend"] = "gloo"
    return a


def launch(o, argv):
    """Start the ranks, poll them, stop the rest when one fails or the time is up.  Returns the exit status."""
    port = free_port()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))         # the ranks import the package this launcher came from
    env = dict(os.environ, WORLD_SIZE=str(o.nproc), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               PYTHONPATH=os.pathsep.join([root] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    cmd = [sys.executable, "-m", "chap_amd.launch", "--rank-process"] + list(argv)
    procs = []
    rc, why = 0, None
    try:
        for r in range(o.nproc):
            procs.append(subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r))))      # fresh processes, never an exec
        deadline = time.monotonic() + o.timeout if o.timeout > 0 else None
        while True:
            codes = [p.poll() for p in procs]
            bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                rc, why = bad[0][1], "rank %d exited with status %d" % bad[0]
                break
            if all(c == 0 for c in codes):
                break
            if deadline is not None and time.monotonic() > deadline:
                rc, why = 124, "not finished within --timeout %.0f s" % o.timeout
                break
            time.sleep(0.05)
    finally:                    # whatever happened (a failed start, Ctrl-C): no rank outlives the launcher
        if why is not None:
            sys.stderr.write("chap_amd.launch: %s; stopping the other ranks\n" % why)
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    return rc if rc >= 0 else 128 - rc


def dry_rank(o):
    """One rank of --dry-run: the helpers of chap_amd.distributed over gloo, on the CPU."""
    import torch
    from .distributed import init_rank, rank_environment
    rank, world, _ = rank_environment()
    if world != o.nproc:
        raise SystemExit("chap_amd.launch: --nproc %d but WORLD_SIZE=%d" % (o.nproc, world))
    if rank == o.dry_run_fail_rank:
        raise SystemExit(3)
    ctx = init_rank({"data_parallel": True, "dp_backend": "gloo", "dp_force_group": True, "dp_timeout_s": max(o.timeout, 30.0)})
    try:
        items = list(range(2 * world + 1))
        got = ctx.gather_in_order([float(i) * 0.5 for i in ctx.shard(items)], len(items))
        assert got == [float(i) * 0.5 for i in items], got
        t = torch.arange(8, dtype=torch.float32)
        ctx.assert_replicas_equal("the dry run's tensor", [t])
        g = t.clone()
        ctx.dist.all_reduce(g)
        assert torch.equal(g, t * world)
        ctx.barrier()
        if ctx.is_main:
            print(json.dumps({"dry_run": True, "entry": o.entry, "world": world, "snapshot": o.snapshot}), flush=True)
    finally:
        ctx.close()


def run_rank(o):
    a = train_args(o)
    if o.entry == "2d":
        from .train_ours_2D import train
    else:
        from .train_ours_3D import train
    train(a, o.snapshot)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    o = build_parser().parse_args(argv)
    if o.rank_process:
        return dry_rank(o) if o.dry_run else run_rank(o)
    if not 1 <= o.nproc <= MAX_RANKS:
        raise SystemExit("chap_amd.launch: --nproc %d: 1 to %d ranks on one node" % (o.nproc, MAX_RANKS))
    if not o.dry_run:
        train_args(o)           # a broken --args / --set fails here, before anything starts
    return launch(o, argv)


if __name__ == "__main__":
    sys.exit(main())
