"""The fused Adam / AdamW inside the training step, at tests/test_guard_step_gpu.py's shapes: DualDecoder at 4 x 1 x 32 x 32 (2 labelled + 2
unlabelled), four classes, fp32, one VAT power iteration; DualDecoder3d at 4 x 1 x 16 x 16 x 16, two classes.

(a) three iterations eager against capture() + replay(): parameters, both moments, the state block and the losses bit for bit.  (b) the first
update against the restatement (tests/adam_ref.py) of the buckets of a twin stopped by device_step(update=False), within the kernel's bound.
(c) with a guard: a huge max_norm is the unguarded step, half the first norm is the plain step called with that coefficient, a NaN written into
bucket 1 leaves everything with its bits and the next iteration is a twin's that never made the poisoned call.  (d) with a teacher, its
average within tests/ema_ref.py's bound of the new parameters.  (e) the recorded launches are the default iteration's with chap_sgd_step
replaced by chap_adam_tick, chap_adam_step at the same position on the same stream; optimizer='sgd' records the default list.  (f) checkpoint
and capture(restore=True).  (g) train() of both entries.  (h) two data-parallel ranks on one GPU (tests/adam_dp_worker.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd.guard import StepGuard
from chap_amd.train import ChapStep, FusedAdamW, FusedSGD, build_teacher
from tests import adam_ref as R
from tests import ema_ref
from tests import guard_ref as gr
from tests.test_class_counts_step_gpu import make_net
from tests.test_guard_step_gpu import CLASSES, case, half_step
from tests.iteration_parity import to_dev

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 3
HUGE = 1e30
LR, WD, BETAS, EPS = 1e-3, 1e-2, (0.9, 0.999), 1e-8
ADAM = dict(optimizer="adamw", base_lr=LR, weight_decay=WD)
KEYS = ("param", "m", "v", "state", "losses", "vat", "ema")


def build(dims, guard=None, teacher=False, extra=ADAM):
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
    step = ChapStep(m, dict(args, **extra), **kw)
    step.iter_num = 3000            # consistency weight 0.165: both buckets carry weight
    return step, (vol.to(DEV), lab.to(DEV), box, to_dev(inj, dims))


def snapshot(step, out=None):
    torch.cuda.synchronize()
    rec = dict(param=step.model.flat_buffers()[0].clone(), m=step.opt.exp_avg.clone(), v=step.opt.exp_avg_sq.clone(), state=step.opt.state.clone(),
               buckets=step.grad_both.clone())
    if out is not None:
        rec["losses"] = torch.stack([l.detach().clone() for l in out["mix_losses"]])
        rec["vat"] = out["vat_loss"].detach().clone()
    if step.teacher is not None:
        rec["ema"] = step.opt.ema.clone()
    return rec


def bits(t):
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def same(a, b, keys=KEYS):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in keys if k in a or k in b)


def new_guard(max_norm=HUGE, skip=True, ring=8):
    return StepGuard(max_norm=max_norm, skip_nonfinite=skip, ring=ring, device=DEV)


def run(dims, guarded=False, teacher=False, graph=False, iters=ITERS):
    step, (vd, ld, box, injd) = build(dims, new_guard() if guarded else None, teacher)
    assert isinstance(step.opt, FusedAdamW) and step.opt.decoupled
    if graph:
        step.capture(vd, ld, warmup=1, inject=injd)
    recs = []
    for _ in range(iters):
        out = step.replay(vd, ld, box_yx=box) if graph else step.step(vd, ld, box_yx=box, inject=injd)
        recs.append(snapshot(step, out))
    return recs


@functools.lru_cache(maxsize=None)
def eager(dims):
    return run(dims)


@functools.lru_cache(maxsize=None)
def twin_first(dims):
    """The step stopped in front of the optimizer at the first iteration: its buckets and what it started from, then its update."""
    step, inputs = build(dims)
    before = snapshot(step)
    out = half_step(step, inputs)
    buckets = step.grad_both.cpu()
    step.exchange_and_update()
    step.finish()
    return before, buckets, snapshot(step, out)


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [2, 3])
def test_a_replay_is_eager_bit_for_bit(dims):
    a, b = eager(dims), run(dims, graph=True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert same(x, y), "iteration %d: replay differs from eager" % (k + 1)
        assert int(y["state"][0]) == k + 1 and float(y["buckets"].abs().max()) == 0.0
    assert not torch.equal(a[0]["param"], a[ITERS - 1]["param"]) and float(a[0]["v"].max()) > 0


# ---- (b) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [2, 3])
def test_b_first_update_is_the_restatement_of_the_twins_buckets(dims):
    before, buckets, after = twin_first(dims)
    assert same(after, eager(dims)[0]), "stopping in front of the optimizer changed the step"
    n = buckets.numel() // 2
    hp = R.kernel_hparams(LR, BETAS[0], BETAS[1], EPS, WD, 1.0)
    tick = R.tick_ref(0, hp["lr"], hp["beta1"], hp["beta2"], hp["weight_decay"], True)
    ref = R.step_ref(before["param"].cpu().numpy(), buckets[:n].numpy(), np.zeros(n), np.zeros(n), tick, hp["beta1"], hp["beta2"], hp["eps"],
                     hp["weight_decay"], True, s=1.0, g2=buckets[n:].numpy(), omb1=hp["omb1"], omb2=hp["omb2"])
    assert float(buckets[:n].abs().max()) > 0 and float(buckets[n:].abs().max()) > 0
    for k, name in (("p", "param"), ("m", "m"), ("v", "v")):
        got = after[name].cpu().numpy()
        i, gv, rv, bv, ratio = R.worst(got, ref[k], ref["e_" + k])
        print("  %dD %s: worst element %d: %.9g vs %.17g, |diff| / bound = %.3g" % (dims, name, i, gv, rv, ratio))
        assert R.within(got, ref[k], ref["e_" + k]), (name, i, gv, rv, bv)
    st = after["state"].cpu().numpy()
    assert int(st[0]) == 1
    for k, name in enumerate(("step_size", "bc2_sqrt", "decay"), 1):
        want = np.float32(tick[name])
        assert abs(float(st[k:k + 1].view(np.float32)[0]) - float(want)) <= float(np.spacing(want)), name


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------
def test_c_a_huge_max_norm_changes_nothing():
    for k, (x, y) in enumerate(zip(eager(2), run(2, guarded=True))):
        assert same(x, y), "iteration %d: the step differs with a guard attached" % (k + 1)


def test_c_clipping_is_the_plain_step_with_the_coefficient_as_grad_scale():
    _, buckets, _ = twin_first(2)
    n = buckets.numel() // 2
    norm = gr.guard_ref(buckets[:n], buckets[n:], 1.0, HUGE)["norm64"]
    max_norm = gr.fl32(0.5 * norm)
    g = new_guard(max_norm)
    step, (vd, ld, box, injd) = build(2, g)
    got = snapshot(step, step.step(vd, ld, box_yx=box, inject=injd))
    coef = float(g.read()["coef"][0])
    assert gr.within_one_ulp(coef, gr.fl32(min(1.0, max_norm / (norm + 1e-6)))) and 0.49 < coef < 0.51
    plain, pin = build(2)
    pout = half_step(plain, pin)
    plain.opt.step(grad_scale=coef, grad2=plain.grad2)
    plain.finish()
    want = snapshot(plain, pout)
    assert same(got, want) and float(got["buckets"].abs().max()) == 0.0
    # (Adam's first step hardly depends on the gradient's scale -- m / sqrt(v) does not -- but the moments do)
    assert not torch.equal(got["m"], eager(2)[0]["m"]) and same(got, eager(2)[0], keys=("losses", "vat"))


def test_c_a_poisoned_gradient_is_skipped_and_the_run_goes_on_as_if_it_had_not_been_applied():
    g = new_guard(max_norm=None)                # skip_nonfinite alone
    step, inputs = build(2, g, teacher=True)
    twin, tin = build(2, None, teacher=True)
    vd, ld, box, injd = inputs
    for s in (step, twin):
        s.step(vd, ld, box_yx=box, inject=injd)
    before = snapshot(step)
    assert same(before, snapshot(twin)) and float(before["m"].abs().max()) > 0 and int(before["state"][0]) == 1
    half_step(step, inputs)
    half_step(twin, tin)
    assert torch.equal(step.grad_both, twin.grad_both) and float(step.grad2.abs().max()) > 0
    step.grad2[step.grad2.numel() - 1] = float("nan")
    step.exchange_and_update()
    step.finish()
    twin.grad_both.zero_()                      # the twin never calls the optimizer for this iteration
    twin.finish()
    after = snapshot(step)
    assert same(before, after, keys=("param", "m", "v", "ema", "state")), "a skipped step wrote parameters, moments, the teacher or the step counter"
    assert float(after["buckets"].abs().max()) == 0.0 and not bool(torch.isnan(after["buckets"]).any())
    assert g.read()["skip"].tolist() == [0, 1]
    a = snapshot(step, step.step(vd, ld, box_yx=box, inject=injd))
    b = snapshot(twin, twin.step(vd, ld, box_yx=box, inject=injd))
    assert same(a, b), "the iteration behind a skipped one differs from the twin's"
    assert int(a["state"][0]) == 2 and not torch.equal(a["param"], before["param"])


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------
def test_d_the_teacher_is_the_average_of_the_new_parameters():
    step, (vd, ld, box, injd) = build(2, teacher=True)
    ema0 = step.opt.ema.clone()
    rec = snapshot(step, step.step(vd, ld, box_yx=box, inject=injd))
    assert same(rec, eager(2)[0], keys=("param", "m", "v", "state", "losses", "vat")), "param / m / v depend on the teacher"
    a, b = ema_ref.coefficients(3000, 0.99)
    assert a == gr.fl32(0.99)
    want, bound = ema_ref.ema_ref(ema0.cpu(), rec["param"].cpu(), a, b)
    err = (rec["ema"].cpu().double() - want).abs()
    print("  ema: max |diff| / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()) and not torch.equal(rec["ema"], ema0)


# ---- (e) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_e_launches_are_the_default_ones_with_the_optimizer_entry_replaced(mode):
    from tests.issue_trace import Recorder
    texts = []
    for extra in ({}, dict(optimizer="sgd"), ADAM):
        step, (vd, ld, box, injd) = build(2, extra=extra)
        rec = Recorder(only_capturing=(mode == "captured"))
        with rec.recording():
            if mode == "captured":
                step.capture(vd, ld, warmup=1, inject=injd)
            else:
                step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
        texts.append(rec.text())
    plain, sgd, adam = (t.splitlines() for t in texts)
    assert sgd == plain
    opt = [i for i, ln in enumerate(plain) if ln.split()[:2] == ["L", "chap_sgd_step"]]
    assert len(opt) == 1 and not any("chap_adam" in ln for ln in plain)
    want = list(plain)
    want[opt[0]:opt[0] + 1] = [plain[opt[0]].replace("chap_sgd_step", n) for n in ("chap_adam_tick", "chap_adam_step")]     # same position, same stream
    assert adam == want


def test_e_default_and_named_optimizers():
    assert isinstance(build(2, extra={})[0].opt, FusedSGD) and isinstance(build(2, extra=dict(optimizer="sgd"))[0].opt, FusedSGD)
    o = build(2, extra=dict(optimizer="adam", base_lr=LR, betas=(0.8, 0.99), adam_eps=1e-6))[0].opt
    assert isinstance(o, FusedAdamW) and not o.decoupled and o.betas == (0.8, 0.99) and o.eps == 1e-6
    with pytest.raises(ValueError, match="optimizer='lion'"):
        build(2, extra=dict(optimizer="lion"))


# ---- (f) --------------------------------------------------------------------------------------------------------------------------------
def test_f_checkpoint_continues_bit_for_bit_and_kinds_do_not_mix():
    step, (vd, ld, box, injd) = build(2)
    for _ in range(2):
        step.step(vd, ld, box_yx=box, inject=injd)
    st = step.state_dict()
    assert "momentum" not in st and st["optimizer"]["kind"] == "adam" and sorted(st["optimizer"]) == ["exp_avg", "exp_avg_sq", "kind", "state"]
    assert st["optimizer"]["state"].tolist()[0] == 2
    third = snapshot(step, step.step(vd, ld, box_yx=box, inject=injd))
    assert same(third, eager(2)[2])
    cont, _ = build(2)
    cont.load_state_dict(st)
    assert same(snapshot(cont, cont.step(vd, ld, box_yx=box, inject=injd)), third)
    # SGD: the key it always had, an existing checkpoint dict loads, the kinds do not mix
    sgd, _ = build(2, extra={})
    sgd.step(vd, ld, box_yx=box, inject=injd)
    old = sgd.state_dict()
    assert "optimizer" not in old and torch.equal(old["momentum"], sgd.opt.mom) and float(old["momentum"].abs().max()) > 0
    assert sgd.opt.state_dict()["kind"] == "sgd" and [t.data_ptr() for t in sgd.opt.state_tensors()] == [sgd.opt.mom.data_ptr()]
    fresh, _ = build(2, extra={})
    fresh.load_state_dict(old)
    assert torch.equal(fresh.opt.mom, sgd.opt.mom) and fresh.iter_num == sgd.iter_num
    p0 = cont.model.flat_buffers()[0].clone()
    with pytest.raises(ValueError, match="'sgd'.*'adam'"):
        cont.load_state_dict(old)
    with pytest.raises(ValueError, match="'adam'.*'sgd'"):
        fresh.load_state_dict(st)
    with pytest.raises(ValueError, match="kind"):
        cont.opt.load_state_dict(sgd.opt.state_dict())
    assert torch.equal(cont.model.flat_buffers()[0], p0), "a refused checkpoint was partly loaded"


def test_f_capture_restores_the_moments_and_the_step_counter():
    step, (vd, ld, box, injd) = build(2)
    for _ in range(2):
        step.step(vd, ld, box_yx=box, inject=injd)
    before = snapshot(step)
    step.capture(vd, ld, warmup=2, inject=injd, restore=True)
    after = snapshot(step)
    assert same(before, after, keys=("param", "m", "v", "state")) and int(after["state"][0]) == 2
    assert same(snapshot(step, step.replay(vd, ld, box_yx=box)), eager(2)[2])


# ---- (g) --------------------------------------------------------------------------------------------------------------------------------
def _train_case(dims):
    if dims == 2:
        from chap_amd.train_ours_2D import train
        return train, dict(model="dualdecoder", decoder_type="mcnet", num_classes=4, batch_size=4, labeled_bs=2, image_size=[32, 32], max_iterations=6,
                           val_interval=3, base_lr=0.05, gpu=0, seed=1337)
    from chap_amd.train_ours_3D import train
    return train, dict(patch_size=[16, 16, 16], num_classes=2, batch_size=4, labeled_bs=2, max_iterations=6, val_interval=3, stride_xy=8, stride_z=8, seed=3)


@pytest.mark.parametrize("dims", [2, 3])
def test_g_train_with_adamw_and_with_the_default_named(tmp_path, dims):
    train, common = _train_case(dims)
    lion = tmp_path / "lion"
    with pytest.raises(ValueError, match="optimizer='lion'"):
        train(dict(common, optimizer="lion"), str(lion))
    assert not lion.exists() or os.listdir(lion) == []
    plain, named, adamw = (str(tmp_path / d) for d in ("plain", "named", "adamw"))
    train(dict(common), plain)
    train(dict(common, optimizer="sgd"), named)
    train(dict(common, optimizer="adamw", base_lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.99), adam_eps=1e-7), adamw)
    # the same checkpoint, byte for byte of every tensor in it (torch.save's container differs between any two saves of the same tensors,
    # so the files themselves cannot be compared)
    b, c = (torch.load(os.path.join(d, "latest.pth"), map_location="cpu") for d in (plain, named))
    assert list(b) == list(c) and all(b[k].dtype == c[k].dtype and b[k].numpy().tobytes() == c[k].numpy().tobytes() for k in b)
    assert open(os.path.join(plain, "log.txt")).read() == open(os.path.join(named, "log.txt")).read()
    assert sorted(os.listdir(plain)) == sorted(os.listdir(named))
    a = torch.load(os.path.join(adamw, "latest.pth"), map_location="cpu")
    assert list(a) == list(b) and [(tuple(a[k].shape), a[k].dtype) for k in a] == [(tuple(b[k].shape), b[k].dtype) for k in b]      # the reference's key set
    assert any(not torch.equal(a[k], b[k]) for k in b) and all(torch.isfinite(v).all() for v in a.values() if v.is_floating_point())
    # (a best model and val.csv appear only when a validation improves the score: either run may or may not have them)
    assert {"latest.pth", "log.txt"} <= set(os.listdir(adamw)) <= {"latest.pth", "log.txt", "val.csv", "%s_best_model.pth" % common.get("model", "dualdecoder")}
    line = "optimizer adamw: base_lr 0.001, betas (0.9, 0.99), eps 1e-07, weight_decay 0.01 (decoupled)"
    log = open(os.path.join(adamw, "log.txt")).read().splitlines()
    assert log.count(line) == 1 and not any(ln.startswith("optimizer ") for ln in open(os.path.join(plain, "log.txt")).read().splitlines())
    assert any(ln.startswith("iteration 6 : ") for ln in log)


# ---- (h) --------------------------------------------------------------------------------------------------------------------------------
def test_h_two_ranks_stay_equal_through_a_clipped_step(tmp_path):
    worker = os.path.join(ROOT, "tests", "adam_dp_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29800 + os.getpid() % 90
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, worker, "--rank", str(r), "--world", "2", "--port", str(port), "--out", str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
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
    r0, r1 = (torch.load(os.path.join(tmp_path, "adam_rank%d.pt" % r)) for r in range(2))
    for k in ("param", "exp_avg", "exp_avg_sq", "state"):
        assert torch.equal(bits(r0[k]), bits(r1[k])), k
    rows = r0["rows"]
    assert rows["step"].tolist() == [1, 2, 3] and rows["skip"].tolist() == [0, 0, 0]
    assert float(rows["coef"][0]) == 1.0 and 0 < float(rows["coef"][1]) < 1 and float(rows["coef"][2]) == 1.0
    assert int(r0["state"][0]) == 3 and r0["moved"] == [True, True, True] and bool(torch.isfinite(r0["param"]).all())
    assert float(r0["exp_avg_sq"].max()) > 0
