"""The training monitor inside the training step, 2D 8 x 1 x 32 x 32 with four classes and 3D 4 x 1 x 16 x 32 x 16 with two:
(a) three iterations with and without a monitor, eager and replayed: every loss word and every parameter is the same -- the monitor does not
change the step; (b) row k is the restatement (tests/monitor_ref.py) of iteration k's pass-A logits, labels and filtered maps, kept by a
subclass of the same step, and its loss words are out['mix_losses'] / out['vat_loss'] bit for bit; (c) rows from graph replay equal rows from
eager; (d) a ring of four, eleven replays, no read: the last four rows and dropped == 7; (e) AblationStep scores its full-batch forward with
n_first = labeled_bs; (f) train() of both entries with monitor=True writes monitor.csv and the reference's loss line and saves the same
latest.pth as without; (g) one recorded monitored iteration has no unordered conflict (tests/launch_order.py), the three entry points
described to the recorder by the access table (tests/launch_access.py)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib, ops
from chap_amd.monitor import StepMonitor
from chap_amd.train import AblationStep, ChapStep
from oracle import init as oinit
from oracle import train_step as ots
from tests import launch_access, launch_order
from tests import monitor_ref as mr
from tests.iteration_parity import inject_2d, inject_3d, to_dev
from tests.test_class_counts_step_gpu import make_net

DEV = "cuda"
ITERS = 3
CLASSES = {2: 4, 3: 2}


@functools.lru_cache(maxsize=None)
def case(dims):
    C = CLASSES[dims]
    if dims == 2:
        B, lbs, sp = 8, 4, (32, 32)
        state = oinit.dual_decoder_2d_state(733, n_class=C)
        vol, lab = ots.synthetic_batch(1551, lbs, B - lbs, *sp, C)
        inj, box = inject_2d(B - lbs, lbs // 2 + (B - lbs) // 2, sp[0], sp[1], 1), (5, 3)
    else:
        B, lbs, sp = 4, 2, (16, 32, 16)
        state = oinit.dual_decoder_3d_state(404, n_class=C)
        vol, lab = ots.synthetic_batch_3d(1339, lbs, B - lbs, *sp, n_classes=C)
        inj, box = inject_3d(B - lbs, lbs // 2 + (B - lbs) // 2, sp, 1), (2, 5, 3)
    return state, vol, lab, box, dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=C), inj


class Keeping:
    """Keeps, per iteration, clones of what the monitor's launches were given (eager only: a clone under capture would be a graph node)."""

    def _monitor_logits(self, logits1, logits2, labels, n_first):
        self._cur = dict(l1=logits1.detach().clone(), l2=logits2.detach().clone(), labels=labels.clone(), n_first=n_first, maps=None)
        super()._monitor_logits(logits1, logits2, labels, n_first)

    def _monitor_maps(self, map1, map2, labels, n_first):
        assert n_first == self._cur["n_first"] and torch.equal(labels, self._cur["labels"])
        self._cur["maps"] = (map1.clone(), map2.clone())
        super()._monitor_maps(map1, map2, labels, n_first)

    def _monitor_finalize(self, scalars, has_labels=True):
        self._cur["scalars"] = torch.cat([s.detach().reshape(1) for s in scalars]).clone()
        self.kept = getattr(self, "kept", []) + [self._cur]
        super()._monitor_finalize(scalars, has_labels)


class KeepingChap(Keeping, ChapStep):
    pass


class KeepingAblation(Keeping, AblationStep):
    pass


def build(dims, monitor, cls=ChapStep, ring=8):
    state, vol, lab, box, args, inj = case(dims)
    m = make_net(dims, CLASSES[dims]).to(DEV).train()
    m.load_state_dict(state, strict=True)
    mon = StepMonitor(CLASSES[dims], ring=ring, device=DEV) if monitor else None
    step = cls(m, dict(args), monitor=mon) if monitor else cls(m, dict(args))
    return step, mon, (vol.to(DEV), lab.to(DEV), box, to_dev(inj, dims))


def snapshot(step, out):
    torch.cuda.synchronize()
    return dict(param=step.model.flat_buffers()[0].clone(), mom=step.opt.mom.clone(),
                losses=torch.stack([l.detach().clone() for l in out["mix_losses"]]), vat=out["vat_loss"].detach().clone(),
                stats={k: v.clone() for k, v in step.model.named_buffers()})


def run(dims, monitor, graph):
    step, mon, (vd, ld, box, injd) = build(dims, monitor, KeepingChap if (monitor and not graph) else ChapStep)
    if graph:
        step.capture(vd, ld, warmup=1, inject=injd)
        assert mon is None or (mon.count == 0 and float(mon.ring.abs().sum()) == 0.0)     # the warm-up iteration's row went with its update
    recs = []
    for _ in range(ITERS):
        out = step.replay(vd, ld, box_yx=box) if graph else step.step(vd, ld, box_yx=box, inject=injd)
        recs.append(snapshot(step, out))
    r = dict(recs=recs)
    if mon is not None:
        r["rows"], r["ring"], r["kept"] = mon.read(), mon.ring.cpu().clone(), getattr(step, "kept", None)
        assert mon.count == ITERS and mon.dropped == 0
    return r


@functools.lru_cache(maxsize=None)
def runs(dims):
    return {(mon, graph): run(dims, mon, graph) for mon in (False, True) for graph in (False, True)}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("param", "mom", "losses", "vat")) and all(torch.equal(a["stats"][k], b["stats"][k]) for k in a["stats"])


@pytest.mark.parametrize("dims", [2, 3])
def test_a_the_monitor_does_not_change_the_step(dims):
    r = runs(dims)
    for graph in (False, True):
        for k, (a, b) in enumerate(zip(r[(False, graph)]["recs"], r[(True, graph)]["recs"])):
            assert same(a, b), "iteration %d (%s): the step differs with a monitor attached" % (k + 1, "replayed" if graph else "eager")
    assert not torch.equal(r[(False, False)]["recs"][0]["param"], r[(False, False)]["recs"][ITERS - 1]["param"])


@pytest.mark.parametrize("dims", [2, 3])
def test_b_rows_are_the_restatement_of_the_iterations_own_tensors(dims):
    C = CLASSES[dims]
    r = runs(dims)[(True, False)]
    rows, kept = r["rows"], r["kept"]
    assert rows["iteration"].tolist() == [1, 2, 3] and rows["dropped"] == 0 and len(kept) == ITERS
    worst = 0.0
    for k, kp in enumerate(kept):
        assert kp["n_first"] == 0 and kp["l1"].shape[0] == case(dims)[4]["batch_size"] - case(dims)[4]["labeled_bs"]
        assert torch.equal(kp["labels"].cpu(), case(dims)[2][case(dims)[4]["labeled_bs"]:])              # the unlabelled samples' own labels
        ref = mr.row_ref(kp["l1"].cpu().numpy(), kp["l2"].cpu().numpy(), kp["labels"].cpu().numpy(), 0, maps=[m.cpu().numpy() for m in kp["maps"]])
        # the arg-max the restatement takes over the logits is the one the step used (ops.pseudo_block on the same logits)
        _, _, p1, p2, _ = ops.pseudo_block(kp["l1"], kp["l2"], want_soft=False)
        for h, p in enumerate((p1, p2)):
            assert ref["pred"][1, h].tolist() == np.bincount(p.cpu().numpy().ravel(), minlength=C).tolist()
        for name in mr.COUNT_FIELDS + ("inter_f", "pred_f"):
            assert np.array_equal(rows[name][k], ref[name]), (name, k, rows[name][k], ref[name])
        for name in ("conf_correct", "conf_err"):
            err, bnd = np.abs(rows[name][k] - ref[name]), ref[name + "_b"]
            print("iteration %d %s |err| %s bound %s" % (k + 1, name, err[1].tolist(), bnd[1].tolist()))
            assert (err <= bnd).all(), (name, k, err, bnd)
            worst = max(worst, float(np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0).max()))
        assert ref["n"][0] == 0 and ref["n"][1] == kp["labels"].numel() and ref["n_correct"][1].min() > 0
        # the loss words, widened exactly
        want = torch.cat([r["recs"][k]["losses"].reshape(-1), r["recs"][k]["vat"].reshape(-1)]).double().cpu().numpy()
        assert torch.equal(kp["scalars"], torch.cat([r["recs"][k]["losses"].reshape(-1), r["recs"][k]["vat"].reshape(-1)]))
        assert np.array_equal(rows["scalars"][k, :13], want) and (rows["scalars"][k, 13:] == 0).all()
    d = StepMonitor.derive(rows)
    m = [r["recs"][0]["losses"][i].double().cpu().numpy() for i in range(4)]
    assert d["loss_l"][0] == m[0][1] + m[1][1] + m[2][0] + m[3][0] and d["loss_u"][0] == m[0][0] + m[1][0] + m[2][1] + m[3][1]
    print("%dD rows vs restatement over %d iterations: worst conf err/bound %.4g" % (dims, ITERS, worst))


@pytest.mark.parametrize("dims", [2, 3])
def test_c_replayed_rows_equal_eager_rows(dims):
    r = runs(dims)
    a, b = r[(True, False)], r[(True, True)]
    assert b["rows"]["iteration"].tolist() == [1, 2, 3]
    assert torch.equal(a["ring"].view(torch.int64), b["ring"].view(torch.int64))


def test_d_a_ring_of_four_reports_what_it_lost():
    step, mon, (vd, ld, box, injd) = build(2, True, ring=4)
    step.capture(vd, ld, warmup=1, inject=injd)
    for _ in range(11):
        step.replay(vd, ld, box_yx=box)
    rows = mon.read()
    assert rows["iteration"].tolist() == [8, 9, 10, 11] and rows["dropped"] == 7 and mon.dropped == 7
    assert (rows["n"][:, 1] == 4 * 32 * 32).all() and (rows["n"][:, 0] == 0).all()
    assert len(mon.read()["iteration"]) == 0


def test_e_ablation_step_scores_both_halves():
    step, mon, (vd, ld, box, injd) = build(2, True, KeepingAblation)
    inj = dict(injd, drop_F=to_dev({"drop_F": oinit.drop_masks_2d(11, 8, 32, 32)}, 2)["drop_F"])
    out = step.step(vd, ld, inject=inj)
    torch.cuda.synchronize()
    rows, kp = mon.read(), step.kept[0]
    lbs = case(2)[4]["labeled_bs"]
    assert kp["n_first"] == lbs and kp["maps"] is None and torch.equal(kp["labels"], ld) and rows["scalar_layout"] == "ablation"
    ref = mr.row_ref(kp["l1"].cpu().numpy(), kp["l2"].cpu().numpy(), ld.cpu().numpy(), lbs)
    for name in mr.COUNT_FIELDS:
        assert np.array_equal(rows[name][0], ref[name]), name
    assert rows["n"][0].tolist() == [lbs * 1024, (8 - lbs) * 1024]
    # group 0 against the labelled half's labels alone
    lab_only = mr.row_ref(kp["l1"][:lbs].cpu().numpy(), kp["l2"][:lbs].cpu().numpy(), ld[:lbs].cpu().numpy(), lbs)
    assert np.array_equal(rows["inter"][0, 0], lab_only["inter"][0]) and np.array_equal(rows["gt"][0, 0], lab_only["gt"][0])
    for name in ("conf_correct", "conf_err"):
        assert (np.abs(rows[name][0] - ref[name]) <= ref[name + "_b"]).all(), name
    assert (rows["inter_f"] == 0).all() and (rows["pred_f"] == 0).all()
    want = torch.cat([t.reshape(1) for t in out["sup_losses"] + out["cps_losses"]] + [out["vat_loss"].reshape(1)]).double().cpu().numpy()
    assert np.array_equal(rows["scalars"][0, :5], want)
    d = StepMonitor.derive(rows)
    assert d["loss_l"][0] == want[0] + want[1] and d["loss_u"][0] == want[2] + want[3]


def _train_pair(train, common, tmp_path):
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    train(dict(common, monitor=True), on)
    train(dict(common), off)
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["monitor.csv"])
    lines = open(os.path.join(on, "monitor.csv")).read().splitlines()
    assert lines[0].startswith("iteration,loss_l,loss_u,vat_loss,disagree,") and [int(ln.split(",")[0]) for ln in lines[1:]] == [1, 2, 3, 4, 5, 6]
    vals = np.array([[float(x) for x in ln.split(",")] for ln in lines[1:]])
    assert np.isfinite(vals).all() and (vals[:, 1] > 0).all() and (vals[:, 4:] >= 0).all() and (vals[:, 4:] <= 1).all()
    log_on, log_off = open(os.path.join(on, "log.txt")).read().splitlines(), open(os.path.join(off, "log.txt")).read().splitlines()
    loss_lines = [ln for ln in log_on if " : l loss : " in ln]
    assert [ln.split(" : ")[0] for ln in loss_lines] == ["iteration %d" % i for i in range(1, 7)] and all(" unl loss : " in ln for ln in loss_lines)
    assert [ln for ln in log_on if ln not in loss_lines] == log_off and not any("l loss" in ln for ln in log_off)
    assert open(os.path.join(on, "latest.pth"), "rb").read() == open(os.path.join(off, "latest.pth"), "rb").read()


def test_f_train_2d_writes_the_monitor_files_and_the_same_weights(tmp_path):
    from chap_amd.train_ours_2D import train
    _train_pair(train, dict(model="dualdecoder", decoder_type="mcnet", num_classes=4, batch_size=8, labeled_bs=4, image_size=[32, 32], max_iterations=6,
                            val_interval=3, base_lr=0.05, gpu=0, seed=1337), tmp_path)


def test_f_train_3d_writes_the_monitor_files_and_the_same_weights(tmp_path):
    from chap_amd.train_ours_3D import train
    _train_pair(train, dict(patch_size=[16, 32, 16], num_classes=2, batch_size=4, labeled_bs=2, max_iterations=6, val_interval=3, stride_xy=8, stride_z=8,
                            seed=3), tmp_path)


# ---- (g) the three entry points are described to the launch recorder by tests/launch_access.py (MODES and RULES, hand-worked in
# tests/test_launch_access_cpu.py): each accumulate launch writes its own region of the workspace, the finalize launch reads both
MONITOR_ENTRIES = ("chap_monitor_accumulate", "chap_monitor_accumulate_labels", "chap_monitor_finalize")


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_g_a_monitored_iteration_has_no_unordered_conflict(mode):
    from tests import issue_trace
    assert all(name in launch_access.MODES and name in launch_access.RULES for name in MONITOR_ENTRIES)
    step, mon, (vd, ld, box, injd) = build(2, True)
    step.iter_num = 4500
    rec = issue_trace.RichRecorder(mode == "captured", issue_trace._Allocations(False), pack_entries=issue_trace._pack_entries_of(step.model))
    with rec.recording():
        if mode == "eager":
            step.step(vd, ld, box_yx=box, inject=injd)
        else:
            step.capture(vd, ld, warmup=1, inject=injd)
    torch.cuda.synchronize()
    rich = rec.rich_text()
    launches = [ln for ln in rich.splitlines() if ln.startswith("L ")]
    for name in MONITOR_ENTRIES:
        mine = [ln for ln in launches if ln.split()[1] == name]
        assert len(mine) == 1 and mine[0].partition(" | ")[2].strip(), name
    an = launch_order.Analysis(rich)
    found = an.findings()
    assert an.counts()["ordered_conflicts"] > 0
    assert found == [], "%d unordered conflicts, the first:\n%s" % (len(found), "\n".join(f["text"] for f in found[:10]))
    # ... and the two accumulate launches sit on different streams, the finalize launch on the first one's
    streams = {name: next(ln for ln in launches if ln.split()[1] == name).split(" | ")[0].split()[2] for name in MONITOR_ENTRIES}
    assert streams["chap_monitor_accumulate"] != streams["chap_monitor_accumulate_labels"]
    assert streams["chap_monitor_finalize"] == streams["chap_monitor_accumulate"]
