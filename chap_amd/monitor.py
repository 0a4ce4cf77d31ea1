"""Device-side training monitor: pseudo-label quality of every iteration, at no host cost per iteration.

The kernels (csrc/monitor.hip, include/chap_hip_monitor.h) count inside the iteration's own streams and leave one fp64 row per iteration in a
ring in device memory; the host copies the ring whenever it likes (`StepMonitor.read()`, e.g. once per validation interval).  Definitions are
pinned to the reference where it has them: acc_conf_analysis (train_ours_2D.py:152-193), the loss line (train_ours_2D.py:404-405), the
head-disagreement ratio (train_ablation_2D.py:180-190).  The split into two groups of samples, C classes instead of four and the Dice of the
maps behind the largest-component filter are this project's own."""
import numpy as np
import torch

from . import ops
from . import _lib as L

# scalar words of a row, by the step that filled them (ChapStep: the four mix_loss triples, then the VAT loss; AblationStep: the two
# supervised losses, the two cross-pseudo-supervision losses, then the VAT loss)
SCALAR_LAYOUTS = {"chap": 13, "ablation": 5}


def row_fields(C):
    """name -> (offset, shape) of the words of one ring row, in the order of chap_hip_monitor.h.  Group-level fields carry a leading
    axis of 2 (group 0, group 1) whose stride is the group's word count."""
    ga, gl = ops.monitor_group_words(C), ops.monitor_label_words(C)
    f = {"iteration": (0, (), 0)}
    o = 1
    for name, off, shape in (("n", 0, ()), ("n_disagree", 1, ()), ("gt", 2, (C,)), ("n_correct", 2 + C, (2,)), ("conf_correct", 4 + C, (2,)),
                             ("conf_err", 6 + C, (2,)), ("inter", 8 + C, (2, C)), ("pred", 8 + 3 * C, (2, C))):
        f[name] = (o + off, shape, ga)
    o += 2 * ga
    f["inter_f"] = (o, (2, C), gl)
    f["pred_f"] = (o + 2 * C, (2, C), gl)
    o += 2 * gl
    f["scalars"] = (o, (L.MONITOR_MAX_SCALARS,), 0)
    assert o + L.MONITOR_MAX_SCALARS == ops.monitor_row_words(C)
    return f


def split_rows(mat, C):
    """[K, row words] fp64 -> dict of named arrays (copies): iteration [K] int64, n / n_disagree [K, 2], gt [K, 2, C], n_correct /
    conf_correct / conf_err [K, 2 groups, 2 heads], inter / pred / inter_f / pred_f [K, 2, 2, C], scalars [K, 16]."""
    mat = np.asarray(mat, dtype=np.float64).reshape(-1, ops.monitor_row_words(C))
    out = {}
    for name, (off, shape, gstride) in row_fields(C).items():
        n = int(np.prod(shape)) if shape else 1
        if gstride:
            a = np.stack([mat[:, off + g * gstride: off + g * gstride + n] for g in range(2)], 1).reshape((mat.shape[0], 2) + shape)
        else:
            a = mat[:, off:off + n].reshape((mat.shape[0],) + shape)
        out[name] = a.astype(np.int64) if name == "iteration" else a.copy()
    return out


class StepMonitor:
    """Owns the kernels' workspace, the ring of `ring` rows and a pinned host mirror of it.  Attach to a step: ChapStep(model, args,
    monitor=StepMonitor(num_classes)).  `device='cpu'` makes a host-only instance (no kernels; the ring bookkeeping of read())."""

    def __init__(self, num_classes, ring=256, device="cuda"):
        if num_classes not in ops.LOSS_CLASSES:
            raise ValueError("chap_amd StepMonitor: num_classes=%d (2..8 built)" % num_classes)
        if ring < 1:
            raise ValueError("chap_amd StepMonitor: ring=%d" % ring)
        self.C, self.R, self.W = int(num_classes), int(ring), ops.monitor_row_words(num_classes)
        self.device = torch.device(device)
        cuda = self.device.type == "cuda"
        self.ws = torch.zeros(ops.monitor_ws_words(self.C), dtype=torch.int64, device=self.device) if cuda else None
        self.ring = torch.zeros(self.R, self.W, dtype=torch.float64, device=self.device)      # iteration 0: a row never written
        self._mirror = torch.zeros(self.R, self.W, dtype=torch.float64)
        self._stream, self._ready, self._copied = None, None, None
        if cuda:
            self._mirror = self._mirror.pin_memory()
            self._stream = torch.cuda.Stream(device=self.device)
            self._ready, self._copied = torch.cuda.Event(), torch.cuda.Event()
        self.count = 0              # rows written so far: the slot of the next one (the step uploads it with its schedule block)
        self.last_iteration = 0     # iteration of the newest row read() has delivered
        self.dropped = 0            # rows overwritten before they were read, over all read() calls
        self.scalar_layout = "chap"

    # ---- the step's side
    def next_slot(self):
        return self.count % self.R

    def advance(self):
        self.count += 1

    def snapshot(self):
        """(count, ring copy): ChapStep.capture() puts its warm-up iterations' rows back with restore()."""
        return self.count, self.ring.clone()

    def restore(self, snap):
        self.count = snap[0]
        self.ring.copy_(snap[1])

    # ---- the reader's side
    def read(self):
        """Rows of every iteration finished since the previous read(), oldest first, as a dict of named numpy arrays (split_rows) plus
        'dropped': how many iterations in between were overwritten before this call (found from the iteration numbers of the rows).  The
        copy runs on the monitor's own stream behind an event recorded on the current stream: the training streams are never synchronised,
        the host waits for that copy alone.  Rows are told apart by their iteration numbers: a step whose counter is set back (a checkpoint loaded
        into it) needs a monitor of its own, or `last_iteration` set back with it."""
        if self._stream is not None:
            cur = torch.cuda.current_stream(self.device)
            self._ready.record(cur)
            with torch.cuda.stream(self._stream):
                self._stream.wait_event(self._ready)
                self._mirror.copy_(self.ring, non_blocking=True)
                self._copied.record(self._stream)
            self._copied.synchronize()
        else:
            self._mirror.copy_(self.ring)
        mat = self._mirror.numpy()
        its = mat[:, 0].astype(np.int64)
        new = np.nonzero(its > self.last_iteration)[0]
        new = new[np.argsort(its[new], kind="stable")]
        rows = split_rows(mat[new], self.C)
        dropped = 0
        if len(new):
            newest = int(its[new[-1]])
            dropped = (newest - self.last_iteration) - len(new)
            self.last_iteration = newest
        self.dropped += dropped
        rows["dropped"] = dropped
        rows["scalar_layout"] = self.scalar_layout
        return rows

    # ---- host arithmetic, fp64
    @staticmethod
    def derive(rows):
        """Per row, in fp64: accuracy, corr_conf = conf_correct / (n_correct + 1e-6), err_conf = conf_err / (n - n_correct + 1e-6) (the + 1e-6
        of train_ours_2D.py:175-179) per group and head; per-class Dice 2 inter / (pred + gt), 0 where that denominator is 0 (as
        medpy.metric.binary.dc), and its mean over the classes 1..C-1 (calculate_avg_dice, which hard-codes three of them), before ('dice',
        'avg_dice') and behind the component filter ('dice_f', 'avg_dice_f'); the head-disagreement ratio per group; loss_l, loss_u, vat_loss."""
        f = {k: np.asarray(v, dtype=np.float64) for k, v in rows.items() if k not in ("dropped", "scalar_layout", "iteration")}
        n, nc = f["n"][:, :, None], f["n_correct"]
        out = {"iteration": np.asarray(rows["iteration"], dtype=np.int64)}
        out["accuracy"] = np.divide(nc, n, out=np.zeros_like(nc), where=n > 0)
        out["corr_conf"] = f["conf_correct"] / (nc + 1e-6)
        out["err_conf"] = f["conf_err"] / (n - nc + 1e-6)
        gt = f["gt"][:, :, None, :]
        for sfx in ("", "_f"):
            inter, den = f["inter" + sfx], f["pred" + sfx] + gt
            d = np.divide(2.0 * inter, den, out=np.zeros_like(inter), where=den > 0)
            out["dice" + sfx] = d
            out["avg_dice" + sfx] = d[..., 1:].mean(-1)
        out["disagree"] = np.divide(f["n_disagree"], f["n"], out=np.zeros_like(f["n"]), where=f["n"] > 0)
        s = f["scalars"]
        if rows.get("scalar_layout", "chap") == "ablation":     # model1_loss + model2_loss parts (train_ablation_2D.py:171-176, 216-217)
            out["loss_l"], out["loss_u"], out["vat_loss"] = s[:, 0] + s[:, 1], s[:, 2] + s[:, 3], s[:, 4]
        else:   # mix_loss returns (loss_image, loss_patch, total): (loss_u_out, loss_l_in) for the unlabelled rows, (loss_l_out, loss_u_in) for the labelled ones
            out["loss_l"] = s[:, 1] + s[:, 4] + s[:, 6] + s[:, 9]
            out["loss_u"] = s[:, 0] + s[:, 3] + s[:, 7] + s[:, 10]
            out["vat_loss"] = s[:, 12]
        return out


CSV_HEADER = ("iteration,loss_l,loss_u,vat_loss,disagree,acc_h1,acc_h2,corr_conf_h1,corr_conf_h2,err_conf_h1,err_conf_h2,"
              "avg_dice_h1,avg_dice_h2,avg_dice_f_h1,avg_dice_f_h2")


def csv_lines(derived):
    """One line per row for <snapshot>/monitor.csv: the per-head values are group 1's (the unlabelled samples)."""
    d = derived
    lines = []
    for k in range(len(d["iteration"])):
        v = [d["loss_l"][k], d["loss_u"][k], d["vat_loss"][k], d["disagree"][k, 1], *d["accuracy"][k, 1], *d["corr_conf"][k, 1], *d["err_conf"][k, 1],
             *d["avg_dice"][k, 1], *d["avg_dice_f"][k, 1]]
        lines.append("%d," % d["iteration"][k] + ",".join("%.9g" % x for x in v))
    return lines


def flush_to_run(monitor, snapshot_path, log):
    """read() the ring and append what came back to the run's files: one line per iteration to <snapshot>/monitor.csv, and the reference's
    'iteration %d : l loss : %f unl loss : %f' (train_ours_2D.py:404-405) to the log.  The train() entries call it every val_interval
    iterations and at the end; the lines of an interval therefore arrive together."""
    return write_rows(monitor.read(), snapshot_path, log)


_SUMMED = ("n", "n_disagree", "gt", "n_correct", "conf_correct", "conf_err", "inter", "pred", "inter_f", "pred_f")


def merge_rows(list_of_rows):
    """The read() results of the data-parallel ranks, one per rank and for the same iterations, as ONE: counts and confidence sums are added (the
    rows of the global batch), the scalar loss words -- each rank's mean over its own samples -- are averaged, 'dropped' is the largest.  The
    iteration words must agree (every rank flushes at the same iterations); ValueError otherwise."""
    if len(list_of_rows) == 0:
        raise ValueError("chap_amd monitor: merge_rows of no rows")
    first = list_of_rows[0]
    its = np.asarray(first["iteration"], dtype=np.int64)
    for r, rows in enumerate(list_of_rows[1:], 1):
        other = np.asarray(rows["iteration"], dtype=np.int64)
        if other.shape != its.shape or (other != its).any():
            raise ValueError("chap_amd monitor: merge_rows: rank %d holds iterations %s, rank 0 holds %s" % (r, other.tolist(), its.tolist()))
        if rows.get("scalar_layout") != first.get("scalar_layout"):
            raise ValueError("chap_amd monitor: merge_rows: rank %d has scalar layout %r, rank 0 %r" % (r, rows.get("scalar_layout"), first.get("scalar_layout")))
    out = {"iteration": its.copy(), "scalar_layout": first.get("scalar_layout", "chap"), "dropped": max(int(rows.get("dropped", 0)) for rows in list_of_rows)}
    for name in _SUMMED + ("scalars",):
        acc = np.array(first[name], dtype=np.float64)
        for rows in list_of_rows[1:]:
            acc = acc + np.asarray(rows[name], dtype=np.float64)
        out[name] = acc / len(list_of_rows) if name == "scalars" else acc
    return out


def write_rows(rows, snapshot_path, log):
    """flush_to_run's writing half, for rows that are already read (one process's, or merge_rows of the ranks')."""
    import os
    d = StepMonitor.derive(rows)
    path = os.path.join(snapshot_path, "monitor.csv")
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write(CSV_HEADER + "\n")
        for line in csv_lines(d):
            f.write(line + "\n")
    if rows["dropped"]:
        log.info("monitor : %d iterations were overwritten in the ring before they were read" % rows["dropped"])
    for k in range(len(d["iteration"])):
        log.info("iteration %d : l loss : %f unl loss : %f" % (d["iteration"][k], d["loss_l"][k], d["loss_u"][k]))
    return d
