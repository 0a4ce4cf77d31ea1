"""Gradient guard: clip by the global gradient norm and skip non-finite steps, on the device.

The kernels (csrc/guard.hip, include/chap_hip_guard.h) sit where the optimizer launch sits: `chap_grad_norm` takes the L2 norm of the gradient
the optimizer is about to apply -- (bucket 0 + bucket 1) * grad_scale, i.e. behind the data-parallel exchange and its 1 / world -- in a fixed
order, and leaves the clip coefficient and a skip flag in a small state block; `chap_sgd_guard_step` is the fused SGD (with or without the
mean teacher's average) reading both from there.  Nothing is read back by the host per iteration and a captured iteration stays one replayed
graph: the state block also holds three counters the kernel advances and a ring of one row per step, which `StepGuard.read()` copies whenever
the host likes (the train() entries: once per validation interval).

Definitions: norm = ||(g + g2) * grad_scale||_2 in fp64; coef = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s
expression; a step is skipped when an element of g + g2 is inf or NaN (and `skip_nonfinite`): parameters, momentum and the teacher's
average keep their bits, the gradient buckets are zeroed.  What the guard does NOT cover is in DESIGN.md section 5 "Gradient guard":
BatchNorm running statistics of a skipped step, and the schedules, which keep following the iteration counter."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import ops

HDR_WORDS = ctypes.sizeof(L.GuardState) // 4
ROW_WORDS = ctypes.sizeof(L.GuardRow) // 4


class StepGuard:
    """Owns the norm kernel's workspace and the state block.  Attach to a step: ChapStep(model, args, guard=StepGuard(max_norm=1.0)), or to
    an optimizer: FusedSGD(model, lr, guard=...).  `max_norm` None or 0: no clipping; `device='cpu'` makes a host-only instance (no kernels)."""

    def __init__(self, max_norm=None, skip_nonfinite=True, ring=256, device="cuda"):
        max_norm = 0.0 if max_norm is None else float(max_norm)
        if max_norm < 0 or max_norm != max_norm:
            raise ValueError("chap_amd StepGuard: max_norm=%r (a norm to clip to, or None / 0 for no clipping)" % (max_norm,))
        if int(ring) < 1:
            raise ValueError("chap_amd StepGuard: ring=%r" % (ring,))
        if max_norm == 0 and not skip_nonfinite:
            raise ValueError("chap_amd StepGuard: neither clipping (max_norm) nor skip_nonfinite is asked for")
        self.max_norm, self.skip_nonfinite, self.R = max_norm, bool(skip_nonfinite), int(ring)
        self.device = torch.device(device)
        cuda = self.device.type == "cuda"
        self.ws = torch.zeros(L.GRADNORM_SLOTS, dtype=torch.float64, device=self.device) if cuda else None
        self.state = torch.zeros(ops.guard_state_words(self.R), dtype=torch.int32, device=self.device)
        self._mirror = torch.zeros_like(self.state, device="cpu")
        self._stream, self._ready, self._copied = None, None, None
        if cuda:
            self._mirror = self._mirror.pin_memory()
            self._stream = torch.cuda.Stream(device=self.device)
            self._ready, self._copied = torch.cuda.Event(), torch.cuda.Event()
        self.last_step = 0          # step number of the newest row read() has delivered
        self.dropped = 0            # rows overwritten before they were read, over all read() calls

    # ---- the optimizer's side
    def launch_norm(self, grad, grad2, grad_scale):
        ops.grad_norm(grad, grad2, self.ws, self.state, self.R, grad_scale, self.max_norm, self.skip_nonfinite)

    # ---- the reader's side
    def _fetch(self):
        if self._stream is not None:
            cur = torch.cuda.current_stream(self.device)
            self._ready.record(cur)
            with torch.cuda.stream(self._stream):
                self._stream.wait_event(self._ready)
                self._mirror.copy_(self.state, non_blocking=True)
                self._copied.record(self._stream)
            self._copied.synchronize()
        else:
            self._mirror.copy_(self.state)
        return self._mirror.numpy()

    def read(self):
        """Rows of every step since the previous read(), oldest first: {'step' int64, 'norm' fp32, 'coef' fp32, 'skip' int64} arrays, the three
        counters 'steps', 'skipped_total', 'clipped_total' and 'dropped' (steps in between whose rows were overwritten before this call).  One
        copy on the guard's own stream behind an event recorded on the current stream: the host waits for that copy alone."""
        return parse_state(self._fetch().copy(), self)

    def snapshot(self):
        """(state copy, last_step): ChapStep.capture() puts its warm-up iterations' rows and counts back with restore()."""
        return self.state.clone(), self.last_step

    def restore(self, snap):
        self.state.copy_(snap[0])
        self.last_step = snap[1]

    def state_dict(self):
        w = self.state[:HDR_WORDS].cpu()
        return {"steps": int(w[3]), "skipped_total": int(w[4]), "clipped_total": int(w[5])}

    def load_state_dict(self, st):
        """The counters of a checkpoint; the rows before it are not in this ring, read() delivers what follows."""
        self.state[3:6].copy_(torch.tensor([int(st["steps"]), int(st["skipped_total"]), int(st["clipped_total"])], dtype=torch.int32))
        self.last_step = int(st["steps"])
        return self


def parse_state(words, guard):
    """read()'s host half on the int32 words of a state block; `guard` carries ring size and last_step / dropped, which it updates."""
    words = np.ascontiguousarray(words, dtype=np.int32)
    R = guard.R
    hdr = words[:HDR_WORDS]
    steps = int(hdr[3])
    rows = words[HDR_WORDS:HDR_WORDS + R * ROW_WORDS].reshape(R, ROW_WORDS)
    first = max(guard.last_step, steps - R) + 1
    want = np.arange(first, steps + 1, dtype=np.int64)
    got = rows[(want - 1) % R] if len(want) else rows[:0]
    ok = got[:, 0] == want
    got = got[ok]
    dropped = max(0, steps - guard.last_step) - int(ok.sum())
    guard.last_step = max(guard.last_step, steps)
    guard.dropped += dropped
    return {"step": got[:, 0].astype(np.int64), "norm": got[:, 1].copy().view(np.float32), "coef": got[:, 2].copy().view(np.float32),
            "skip": got[:, 3].astype(np.int64), "steps": steps, "skipped_total": int(hdr[4]), "clipped_total": int(hdr[5]), "dropped": dropped}


CSV_HEADER = "iteration,grad_norm,coef,skipped"


def csv_lines(rows):
    return ["%d,%.9g,%.9g,%d" % (rows["step"][k], rows["norm"][k], rows["coef"][k], rows["skip"][k]) for k in range(len(rows["step"]))]


def summary_line(rows):
    """The interval's log line: maximum and median of the finite norms, and how many of its steps were clipped and skipped."""
    n = len(rows["step"])
    norms = np.asarray(rows["norm"], dtype=np.float64)
    fin = norms[np.isfinite(norms)]
    skip = np.asarray(rows["skip"]) != 0
    clipped = int(((np.asarray(rows["coef"]) < 1.0) & ~skip).sum())
    mx, med = (float(fin.max()), float(np.median(fin))) if len(fin) else (float("nan"), float("nan"))
    return "guard : iterations %d-%d : max grad norm : %f median grad norm : %f clipped : %d skipped : %d of %d" % (
        rows["step"][0], rows["step"][-1], mx, med, clipped, int(skip.sum()), n)


def write_rows(rows, snapshot_path, log):
    """Append rows that are already read to <snapshot>/guard.csv and log the interval's summary and every skipped iteration by number."""
    import os
    path = os.path.join(snapshot_path, "guard.csv")
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write(CSV_HEADER + "\n")
        for line in csv_lines(rows):
            f.write(line + "\n")
    if rows["dropped"]:
        log.info("guard : %d iterations were overwritten in the ring before they were read" % rows["dropped"])
    if len(rows["step"]):
        log.info(summary_line(rows))
    for k in np.nonzero(np.asarray(rows["skip"]) != 0)[0]:
        log.info("guard : iteration %d skipped : non-finite gradient (norm %s)" % (rows["step"][k], rows["norm"][k]))
    return rows


def flush_to_run(guard, snapshot_path, log):
    """read() the ring and append what came back to the run's files.  The train() entries call it (rank 0 alone: the rows are the same words
    on every rank) every val_interval iterations and at the end."""
    return write_rows(guard.read(), snapshot_path, log)


def first_nonfinite(state_dict):
    """Name of the first floating-point tensor of `state_dict` that holds an inf or a NaN, or None.  One host synchronisation for all of them."""
    names = [k for k, v in state_dict.items() if torch.is_tensor(v) and v.is_floating_point()]
    if not names:
        return None
    flags = torch.stack([torch.isfinite(state_dict[k]).all() for k in names]).cpu().tolist()
    for k, ok in zip(names, flags):
        if not ok:
            return k
    return None


def check_finite_before_save(state_dict, what, iteration):
    """The checkpoint gate of the train() entries: raise, naming the first non-finite tensor, instead of overwriting a good file with it."""
    bad = first_nonfinite(state_dict)
    if bad is not None:
        raise RuntimeError("chap_amd.train: iteration %d: %s holds a non-finite value in %r; the checkpoint files are left as they are" % (iteration, what, bad))
    return state_dict
