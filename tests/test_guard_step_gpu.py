"""The gradient guard inside the training step: DualDecoder at 4 x 1 x 32 x 32 (2 labelled + 2 unlabelled), four classes, fp32, one VAT power
iteration; DualDecoder3d at 4 x 1 x 16 x 16 x 16, two classes.

(a) max_norm = 1e30: three iterations equal the unguarded step bit for bit -- parameters, momentum, losses and, with a teacher, its average --
eager and replayed; the ring's norms are the restatement's (tests/guard_ref.py) of the two buckets of a twin run that stops in front of the
optimizer (device_step(update=False)), within the kernel's bound.  (b) max_norm = half the first norm: the coefficient matches the
restatement to one ulp, the update is the plain optimizer's with grad_scale = that coefficient, bit for bit.  (c) a NaN written into bucket 1
between device_step(update=False) and exchange_and_update(): parameters, momentum and teacher keep their bits, the buckets are zero, and the
next iteration is the one of a twin that never made the poisoned call.  (d) 3D, one iteration.  (e) the launches of a guarded iteration are the
default ones with the optimizer entry replaced by the guard's two.  (f) checkpoint: the counters travel in ChapStep.state_dict(), an old
checkpoint loads.  (g) train() of both entries with the flags set writes guard.csv and the summary line and, with a huge max_norm, the same
latest.pth as without.  (h) two data-parallel ranks on one GPU (tests/guard_dp_worker.py): identical ring rows, replicas equal after a
clipped and after a skipped step, the NaN coming from one rank only.

The 3D case has batch 4 (2 + 2), not 2 (1 + 1): the BCP loop mixes HALVES of the labelled and of the unlabelled samples, and with one of each
pass B's input is empty, which chap_conv_fwd refuses ("empty grid")."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd.guard import StepGuard
from chap_amd.train import ChapStep, build_teacher
from oracle import init as oinit
from oracle import train_step as ots
from tests import guard_ref as gr
from tests.iteration_parity import inject_2d, inject_3d, to_dev
from tests.test_class_counts_step_gpu import make_net

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 3
CLASSES = {2: 4, 3: 2}
HUGE = 1e30


@functools.lru_cache(maxsize=None)
def case(dims):
    C = CLASSES[dims]
    B, lbs = 4, 2
    if dims == 2:
        sp = (32, 32)
        state = oinit.dual_decoder_2d_state(733, n_class=C)
        vol, lab = ots.synthetic_batch(1551, lbs, B - lbs, *sp, C)
        inj, box = inject_2d(B - lbs, lbs // 2 + (B - lbs) // 2, sp[0], sp[1], 1), (5, 3)
    else:
        sp = (16, 16, 16)
        state = oinit.dual_decoder_3d_state(404, n_class=C)
        vol, lab = ots.synthetic_batch_3d(1339, lbs, B - lbs, *sp, n_classes=C)
        inj, box = inject_3d(B - lbs, lbs // 2 + (B - lbs) // 2, sp, 1), (2, 5, 3)
    return state, vol, lab, box, dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=C), inj


def build(dims, guard=None, teacher=False):
    state, vol, lab, box, args, inj = case(dims)
    C = CLASSES[dims]
    m = make_net(dims, C).to(DEV).train()
    m.load_state_dict(state, strict=True)
    kw = {}
    if teacher:
        def make():
            torch.manual_seed(99)
            return make_net(dims, C).to(DEV)
        kw["teacher"] = build_teacher(make).eval()
    if guard is not None:
        kw["guard"] = guard
    step = ChapStep(m, dict(args), **kw)
    step.iter_num = 3000            # consistency weight 0.165: both buckets carry weight
    return step, (vol.to(DEV), lab.to(DEV), box, to_dev(inj, dims))


def snapshot(step, out=None):
    torch.cuda.synchronize()
    rec = dict(param=step.model.flat_buffers()[0].clone(), mom=step.opt.mom.clone(), buckets=step.grad_both.clone())
    if out is not None:
        rec["losses"] = torch.stack([l.detach().clone() for l in out["mix_losses"]])
        rec["vat"] = out["vat_loss"].detach().clone()
    if step.teacher is not None:
        rec["ema"] = step.opt.ema.clone()
    return rec


def same(a, b, keys=("param", "mom", "losses", "vat", "ema")):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys if k in a or k in b)


def new_guard(max_norm=HUGE, skip=True, ring=8):
    return StepGuard(max_norm=max_norm, skip_nonfinite=skip, ring=ring, device=DEV)


def run(dims, guarded, teacher, graph, iters=ITERS):
    g = new_guard() if guarded else None
    step, (vd, ld, box, injd) = build(dims, g, teacher)
    if graph:
        step.capture(vd, ld, warmup=1, inject=injd)
        if g is not None:           # the warm-up iteration's row and count went with its update
            r = g.read()
            assert r["steps"] == 0 and len(r["step"]) == 0
    recs = []
    for _ in range(iters):
        out = step.replay(vd, ld, box_yx=box) if graph else step.step(vd, ld, box_yx=box, inject=injd)
        recs.append(snapshot(step, out))
    return dict(recs=recs, rows=None if g is None else g.read())


@functools.lru_cache(maxsize=None)
def runs(dims, teacher):
    return {(guarded, graph): run(dims, guarded, teacher, graph) for guarded in (False, True) for graph in (False, True)}


def half_step(step, inputs):
    """One iteration up to the optimizer: the buckets are final and still there."""
    vd, ld, box, injd = inputs
    step._hw = tuple(vd.shape[2:])
    step.prepare(box)
    out = step.device_step(vd, ld, injd, update=False)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def twin_bucket_refs(dims):
    """The unguarded step, stopped in front of the optimizer at every iteration: the restatement of the two buckets, then the update."""
    step, inputs = build(dims)
    refs, recs = [], []
    n = step.grad_both.numel() // 2
    for _ in range(ITERS):
        out = half_step(step, inputs)
        b = step.grad_both.cpu()
        refs.append(gr.guard_ref(b[:n], b[n:], 1.0, HUGE))
        step.exchange_and_update()
        step.finish()
        recs.append(snapshot(step, out))
    return refs, recs


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("teacher", [False, True], ids=["student", "teacher"])
def test_a_a_huge_max_norm_changes_nothing(teacher):
    r = runs(2, teacher)
    for graph in (False, True):
        for k, (a, b) in enumerate(zip(r[(False, graph)]["recs"], r[(True, graph)]["recs"])):
            assert same(a, b), "iteration %d (%s): the step differs with a guard attached" % (k + 1, "replayed" if graph else "eager")
            assert float(b["buckets"].abs().max()) == 0.0 and ("ema" in b) == teacher
    for k, (a, b) in enumerate(zip(r[(True, False)]["recs"], r[(True, True)]["recs"])):
        assert same(a, b), "iteration %d: replay differs from eager" % (k + 1)
    assert not torch.equal(r[(True, False)]["recs"][0]["param"], r[(True, False)]["recs"][ITERS - 1]["param"])
    for graph in (False, True):
        rows = r[(True, graph)]["rows"]
        assert rows["step"].tolist() == [1, 2, 3] and rows["coef"].tolist() == [1.0] * 3 and rows["skip"].tolist() == [0] * 3
        assert (rows["steps"], rows["skipped_total"], rows["clipped_total"], rows["dropped"]) == (3, 0, 0, 0)
    assert r[(True, False)]["rows"]["norm"].tobytes() == r[(True, True)]["rows"]["norm"].tobytes()      # replayed rows are the eager ones


def test_a_ring_norms_are_the_restatement_of_the_twins_buckets():
    refs, recs = twin_bucket_refs(2)
    r = runs(2, False)
    for k, (a, b) in enumerate(zip(recs, r[(False, False)]["recs"])):
        assert same(a, b), "iteration %d: stopping in front of the optimizer changed the unguarded step" % (k + 1)
    norms = r[(True, False)]["rows"]["norm"]
    for k, ref in enumerate(refs):
        assert ref["skip"] == 0 and ref["norm64"] > 0
        # the kernel's fp64 norm is within ref['bound'] (relative) of ref['norm64']; what the ring holds is it rounded to fp32
        lo, hi = gr.fl32(ref["norm64"] * (1 - ref["bound"])), gr.fl32(ref["norm64"] * (1 + ref["bound"]))
        print("  iteration %d: ring norm %.9g, restatement %.17g (bound %.3g)" % (k + 1, norms[k], ref["norm64"], ref["bound"]))
        assert lo <= float(norms[k]) <= hi, (k, float(norms[k]), ref["norm64"])


# ---- (b) --------------------------------------------------------------------------------------------------------------------------------
def test_b_clipping_is_the_plain_optimizer_with_the_coefficient_as_grad_scale():
    refs, _ = twin_bucket_refs(2)
    max_norm = gr.fl32(0.5 * refs[0]["norm64"])
    g = new_guard(max_norm)
    step, inputs = build(2, g)
    vd, ld, box, injd = inputs
    out = step.step(vd, ld, box_yx=box, inject=injd)
    got = snapshot(step, out)
    rows = g.read()
    want_coef = min(1.0, max_norm / (refs[0]["norm64"] + 1e-6))
    coef = float(rows["coef"][0])
    print("  max_norm %.9g: coef %.9g, restatement %.17g" % (max_norm, coef, want_coef))
    assert gr.within_one_ulp(coef, gr.fl32(want_coef)) and 0.49 < coef < 0.51
    assert (rows["steps"], rows["clipped_total"], rows["skipped_total"]) == (1, 1, 0) and rows["skip"].tolist() == [0]
    # the plain optimizer on the same buckets with grad_scale = fl32(1 * coef)
    plain, pin = build(2)
    pout = half_step(plain, pin)
    plain.opt.step(grad_scale=coef, grad2=plain.grad2)
    plain.finish()
    want = snapshot(plain, pout)
    assert same(got, want) and float(got["buckets"].abs().max()) == 0.0
    unclipped = runs(2, False)[(False, False)]["recs"][0]
    assert not torch.equal(got["param"], unclipped["param"]) and same(got, unclipped, keys=("losses", "vat"))


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------
def test_c_a_poisoned_gradient_is_skipped_and_the_run_goes_on_as_if_it_had_not_been_applied():
    g = new_guard(max_norm=None)                # skip_nonfinite alone
    step, inputs = build(2, g, teacher=True)
    twin, tin = build(2, None, teacher=True)
    vd, ld, box, injd = inputs
    for s in (step, twin):
        s.step(vd, ld, box_yx=box, inject=injd)
    before = snapshot(step)
    assert same(before, snapshot(twin)) and float(before["mom"].abs().max()) > 0
    # iteration 2: the forward and backward passes run (nothing in them sees a NaN), then one element of bucket 1 is poisoned
    half_step(step, inputs)
    half_step(twin, tin)
    assert torch.equal(step.grad_both, twin.grad_both) and float(step.grad2.abs().max()) > 0
    step.grad2[step.grad2.numel() - 1] = float("nan")
    step.exchange_and_update()
    step.finish()
    twin.grad_both.zero_()                      # the twin never calls the optimizer for this iteration
    twin.finish()
    after = snapshot(step)
    assert same(before, after, keys=("param", "mom", "ema")), "a skipped step wrote parameters, momentum or the teacher"
    assert float(after["buckets"].abs().max()) == 0.0 and not bool(torch.isnan(after["buckets"]).any())
    rows = g.read()
    assert rows["skip"].tolist() == [0, 1] and rows["coef"].tolist() == [1.0, 0.0] and math.isnan(float(rows["norm"][1]))
    assert (rows["steps"], rows["skipped_total"], rows["clipped_total"]) == (2, 1, 0)
    # iteration 3
    a = snapshot(step, step.step(vd, ld, box_yx=box, inject=injd))
    b = snapshot(twin, twin.step(vd, ld, box_yx=box, inject=injd))
    assert same(a, b), "the iteration behind a skipped one differs from the twin's"
    assert not torch.equal(a["param"], before["param"]) and g.read()["skip"].tolist() == [0]


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------
def test_d_3d_one_iteration_equals_the_unguarded_step():
    a, b = run(3, False, False, False, iters=1), run(3, True, False, False, iters=1)
    assert same(a["recs"][0], b["recs"][0]) and float(b["recs"][0]["buckets"].abs().max()) == 0.0
    rows = b["rows"]
    assert rows["step"].tolist() == [1] and rows["coef"].tolist() == [1.0] and float(rows["norm"][0]) > 0 and math.isfinite(float(rows["norm"][0]))


# ---- (e) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_e_launches_are_the_default_ones_with_the_optimizer_entry_replaced(mode):
    from tests.issue_trace import Recorder
    texts = []
    for guarded in (False, True):
        step, (vd, ld, box, injd) = build(2, new_guard() if guarded else None)
        rec = Recorder(only_capturing=(mode == "captured"))
        with rec.recording():
            if mode == "captured":
                step.capture(vd, ld, warmup=1, inject=injd)
            else:
                step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
        texts.append(rec.text())
    plain, guarded = (t.splitlines() for t in texts)
    opt = [i for i, ln in enumerate(plain) if ln.split()[:2] == ["L", "chap_sgd_step"]]
    assert len(opt) == 1 and not any("chap_grad_norm" in ln or "chap_sgd_guard_step" in ln for ln in plain)
    want = list(plain)
    want[opt[0]:opt[0] + 1] = [plain[opt[0]].replace("chap_sgd_step", n) for n in ("chap_grad_norm", "chap_sgd_guard_step")]     # same position, same stream
    assert guarded == want


def test_e_a_guard_needs_the_fused_optimizer():
    state, *_ = case(2)
    m = make_net(2, CLASSES[2]).to(DEV).train()

    class Other:
        lr_dev = torch.zeros(1, device=DEV)
    with pytest.raises(ValueError, match="gradient guard needs the fused optimizer"):
        ChapStep(m, dict(case(2)[4]), optimizer=Other(), guard=new_guard())
    with pytest.raises(ValueError, match="guard lives on"):
        ChapStep(m, dict(case(2)[4]), guard=StepGuard(max_norm=1.0, device="cpu"))


# ---- (f) --------------------------------------------------------------------------------------------------------------------------------
def test_f_counters_travel_with_the_checkpoint_and_an_old_one_loads():
    refs, _ = twin_bucket_refs(2)
    g = new_guard(gr.fl32(0.5 * refs[0]["norm64"]))
    step, (vd, ld, box, injd) = build(2, g)
    for _ in range(2):
        step.step(vd, ld, box_yx=box, inject=injd)
    st = step.state_dict()
    assert st["guard"] == {"steps": 2, "skipped_total": 0, "clipped_total": 2}
    third = snapshot(step, step.step(vd, ld, box_yx=box, inject=injd))
    g2 = new_guard(g.max_norm)
    cont, _ = build(2, g2)
    cont.load_state_dict(st)
    again = snapshot(cont, cont.step(vd, ld, box_yx=box, inject=injd))
    assert same(third, again)
    rows = g2.read()
    assert rows["step"].tolist() == [3] and (rows["steps"], rows["clipped_total"], rows["dropped"]) == (3, 3, 0)
    old = {k: v for k, v in st.items() if k != "guard"}
    g3 = new_guard(g.max_norm)
    build(2, g3)[0].load_state_dict(old)
    assert g3.state_dict() == {"steps": 0, "skipped_total": 0, "clipped_total": 0}
    assert "guard" not in build(2)[0].state_dict()


# ---- (g) --------------------------------------------------------------------------------------------------------------------------------
def _train_case(dims):
    if dims == 2:
        from chap_amd.train_ours_2D import train
        return train, dict(model="dualdecoder", decoder_type="mcnet", num_classes=4, batch_size=4, labeled_bs=2, image_size=[32, 32], max_iterations=4,
                           val_interval=2, base_lr=0.05, gpu=0, seed=1337)
    from chap_amd.train_ours_3D import train
    return train, dict(patch_size=[16, 16, 16], num_classes=2, batch_size=4, labeled_bs=2, max_iterations=4, val_interval=2, stride_xy=8, stride_z=8, seed=3)


@pytest.mark.parametrize("dims", [2, 3])
def test_g_train_writes_guard_csv_and_the_same_checkpoint(tmp_path, dims):
    train, common = _train_case(dims)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    train(dict(common, clip_grad_norm=HUGE, skip_nonfinite=True), on)
    train(dict(common), off)
    assert sorted(os.listdir(off)) == [f for f in sorted(os.listdir(on)) if f != "guard.csv"] and "guard.csv" in os.listdir(on)
    lines = open(os.path.join(on, "guard.csv")).read().splitlines()
    assert lines[0] == "iteration,grad_norm,coef,skipped" and [ln.split(",")[0] for ln in lines[1:]] == ["1", "2", "3", "4"]
    assert all(ln.split(",")[2:] == ["1", "0"] and float(ln.split(",")[1]) > 0 for ln in lines[1:])
    log_on, log_off = open(os.path.join(on, "log.txt")).read().splitlines(), open(os.path.join(off, "log.txt")).read().splitlines()
    glines = [ln for ln in log_on if ln.startswith("guard : ")]
    assert len(glines) == 2 and glines[0].startswith("guard : iterations 1-2 : max grad norm : ") and glines[1].startswith("guard : iterations 3-4 : ")
    assert all(ln.endswith("clipped : 0 skipped : 0 of 2") for ln in glines)
    assert [ln for ln in log_on if not ln.startswith("guard : ")] == log_off
    a, b = (torch.load(os.path.join(d, "latest.pth"), map_location="cpu") for d in (on, off))
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # a small max_norm clips every step and the model differs
    clip = str(tmp_path / "clip")
    train(dict(common, clip_grad_norm=1e-3), clip)
    lines = open(os.path.join(clip, "guard.csv")).read().splitlines()[1:]
    assert len(lines) == 4 and all(0 < float(ln.split(",")[2]) < 1 and ln.endswith(",0") for ln in lines)
    c = torch.load(os.path.join(clip, "latest.pth"), map_location="cpu")
    assert any(not torch.equal(c[k], b[k]) for k in b) and all(torch.isfinite(v).all() for v in c.values() if v.is_floating_point())


# ---- (h) --------------------------------------------------------------------------------------------------------------------------------
def test_h_two_ranks_hold_the_same_rows_and_stay_equal_through_a_clipped_and_a_skipped_step(tmp_path):
    worker = os.path.join(ROOT, "tests", "guard_dp_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29700 + os.getpid() % 90
    procs = [subprocess.Popen([sys.executable, worker, "--rank", str(r), "--world", "2", "--port", str(port), "--out", str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=400)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o.decode(errors="replace")[-4000:]
    r0, r1 = (torch.load(os.path.join(tmp_path, "guard_rank%d.pt" % r)) for r in range(2))
    for k in ("step", "norm", "coef", "skip"):
        assert torch.equal(r0["rows"][k].view(torch.int32) if r0["rows"][k].dtype == torch.float32 else r0["rows"][k],
                           r1["rows"][k].view(torch.int32) if r1["rows"][k].dtype == torch.float32 else r1["rows"][k]), k
    rows = r0["rows"]
    assert rows["step"].tolist() == [1, 2, 3, 4] and rows["skip"].tolist() == [0, 1, 0, 0] and float(rows["coef"][1]) == 0.0
    assert all(0 < float(rows["coef"][k]) < 1 for k in (0, 2, 3)) and not math.isfinite(float(rows["norm"][1]))
    for r in (r0, r1):
        assert (r["rows"]["steps"], r["rows"]["skipped_total"], r["rows"]["clipped_total"]) == (4, 1, 3)
        assert r["unchanged"] and r["buckets_zero"] and r["moved"] == [False, True, True] and r["graphs"] == (True, True)
    assert torch.equal(r0["param"].view(torch.int32), r1["param"].view(torch.int32)) and torch.equal(r0["mom"].view(torch.int32), r1["mom"].view(torch.int32))
    assert bool(torch.isfinite(r0["param"]).all())
