"""The mean teacher's consistency term inside the training step, at the smallest 2D (8 x 1 x 64 x 64) and 3D (4 x 1 x 16 x 32 x 16) step cases with
two and three classes.  Off (teacher_consistency = 0) the step is the mean-teacher step, launch for launch and bit for bit.  On: the new
launch is checked per element against tests/teacher_ref.py on the tensors it got inside a real step, and its dlogits are the buffers
mix_loss_bwd wrote (the e set with `dropout`); the teacher's logits equal the same module called stand-alone; no BatchNorm buffer notices the
pass; the noise is the restated generator's; capture + replay equals eager; resume is bit-exact; the guard, a clipping guard and AdamW combine
with it; train() of both entries logs the term and writes the teacher; two data-parallel ranks stay equal."""
import contextlib
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from chap_amd.guard import StepGuard
from chap_amd.train import ChapStep, build_teacher
from tests import kernel_ref as kr
from tests import teacher_ref as tr
from tests.issue_trace import Recorder
from tests.iteration_parity import to_dev
from tests.test_class_counts_step_gpu import case_2d, case_3d, make_net

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, DECAY, W_T, NOISE = 5, 0.99, 0.7, 0.1
CASES = [(2, 2), (2, 3), (3, 2), (3, 3)]
IDS = ["2d_c2", "2d_c3", "3d_c2", "3d_c3"]
ON = dict(teacher_consistency=W_T, teacher_noise=NOISE)


def case(dims, C):
    return case_2d(C) if dims == 2 else case_3d(C)


def build(dims, C, guard=None, inject_teacher=True, **extra):
    """(step, model, teacher, device inputs).  `inject_teacher`: static dropout masks and noise for the teacher's pass too (pass B's masks, a
    uniform tensor of its own), so that an eager step and a replay draw nothing."""
    state, vol, lab, box, args, inj = case(dims, C)
    m = make_net(dims, C).to(DEV).train()
    m.load_state_dict(state, strict=True)

    def make():
        torch.manual_seed(99)
        return make_net(dims, C).to(DEV)
    t = build_teacher(make).eval()
    g = None if guard is None else StepGuard(ring=8, device=torch.device(DEV, 0), **guard)
    step = ChapStep(m, dict(args, ema_decay=DECAY, **extra), teacher=t, guard=g)
    injd = to_dev(inj, dims)
    if inject_teacher:
        nb = args["labeled_bs"] // 2 + (args["batch_size"] - args["labeled_bs"]) // 2
        injd["drop_T"] = injd["drop_B"]
        injd["teacher_u"] = ((torch.rand((nb,) + tuple(vol.shape[1:]), generator=torch.Generator().manual_seed(77)) * 2 - 1) * NOISE).to(DEV)
    return step, m, t, (vol.to(DEV), lab.to(DEV), box, injd)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def snapshot(step, out):
    torch.cuda.synchronize()
    rec = dict(param=step.model.flat_buffers()[0].clone(), ema=step.opt.ema.clone(), iter_num=step.iter_num,
               losses=torch.stack([l.detach().clone() for l in out["mix_losses"]]), vat=out["vat_loss"].detach().clone())
    for i, s in enumerate(step.opt.state_tensors()):
        rec["opt%d" % i] = s.clone()
    for k, v in step.model.named_buffers():
        rec["stat." + k] = v.clone()
    for k, v in step.teacher.named_buffers():
        rec["tstat." + k] = v.clone()
    if "teacher_loss" in out:
        rec["teacher_loss"] = out["teacher_loss"].detach().clone()
    return rec


def same(a, b, skip=()):
    bad = [k for k in a if k not in skip and (k not in b or (not torch.equal(bits(a[k]), bits(b[k])) if torch.is_tensor(a[k]) else a[k] != b[k]))]
    return bad + [k for k in b if k not in a and k not in skip]


def run(dims, C, graph=False, iters=ITERS, save_at=None, load=None, start=0, guard=None, **extra):
    step, m, t, (vd, ld, box, injd) = build(dims, C, guard=guard, **extra)
    if load is not None:
        step.load_state_dict(load)
    if graph:
        step.capture(vd, ld, warmup=1, inject=injd)
    recs, saved = [], None
    for k in range(start, iters):
        out = step.replay(vd, ld, box_yx=box) if graph else step.step(vd, ld, box_yx=box, inject=injd)
        recs.append(snapshot(step, out))
        if save_at == k + 1:
            saved = step.state_dict()
    return dict(recs=recs, saved=saved)


@functools.lru_cache(maxsize=None)
def runs_on(dims, C):
    return run(dims, C, save_at=3, **ON), run(dims, C, graph=True, **ON)


# ---- off is the parent ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,C", CASES, ids=IDS)
def test_off_five_iterations_are_the_mean_teacher_steps_bit_for_bit(dims, C):
    parent = run(dims, C)                                               # the arguments absent: the step as it was
    off = run(dims, C, teacher_consistency=0.0, teacher_noise=0.3)
    for k, (a, b) in enumerate(zip(parent["recs"], off["recs"])):
        assert same(a, b) == [], "iteration %d" % (k + 1)
        assert "teacher_loss" not in b


@pytest.mark.parametrize("dims,mode", [(2, "eager"), (2, "captured"), (3, "eager")])
def test_off_the_launch_list_is_the_mean_teacher_steps(dims, mode):
    texts = []
    for extra in ({}, dict(teacher_consistency=0.0)):
        step, m, t, (vd, ld, box, injd) = build(dims, 2, **extra)
        rec = Recorder(only_capturing=(mode == "captured"))
        with rec.recording():
            if mode == "captured":
                step.capture(vd, ld, warmup=1, inject=injd)
            else:
                step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
        texts.append(rec.text())
    assert texts[0] == texts[1] and "chap_teacher_consistency" not in texts[0] and "chap_sgd_ema_step" in texts[0]


# ---- on: the launch inside a real step ----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def spying():
    """Observe ops.teacher_consistency (tensors in and out), the dlogits pointers of every mix_loss backward launch, ops.rand_uniform and
    ops.perturb, and the teacher's forward.  Everything calls through; what was patched is restored."""
    seen = dict(tc=[], bwd=[], rand=[], perturb=[])
    real_tc, real_call, real_rand, real_perturb = ops.teacher_consistency, L.call, ops.rand_uniform, ops.perturb

    def tc(logits, teacher, loss, dlogits=(None, None), gscale=1.0, gscale_dev=None, accumulate=False, ws=None):
        rec = dict(s=[t.detach().clone() for t in logits], t=[t.detach().clone() for t in teacher], prior=[d.clone() for d in dlogits], gscale=gscale,
                   cw=gscale_dev.clone(), accumulate=accumulate, ptrs=[d.data_ptr() for d in dlogits], stream=torch.cuda.current_stream().cuda_stream)
        real_tc(logits, teacher, loss, dlogits, gscale, gscale_dev, accumulate, ws)
        rec.update(g=[d.clone() for d in dlogits], loss=loss.clone())
        seen["tc"].append(rec)

    def call(name, params, stream):
        if name == "chap_mix_loss_bwd":
            seen["bwd"].append([params.dlogits])
        elif name == "chap_mix_loss_multi_bwd":
            seen["bwd"].append([params.term[i].dlogits for i in range(params.nterms)])
        return real_call(name, params, stream)

    def rand(out, seed, lo=0.0, hi=1.0, seed_dev=None):
        real_rand(out, seed, lo, hi, seed_dev)
        seen["rand"].append(dict(out=out, seed=seed, lo=lo, hi=hi, seed_dev=seed_dev, cap=torch.cuda.is_current_stream_capturing()))

    def perturb(x, d, out, alpha, mask=None, sign=False):
        real_perturb(x, d, out, alpha, mask, sign)
        seen["perturb"].append(dict(x=x, d=d, out=out, alpha=alpha, mask=mask, sign=sign))

    try:
        ops.teacher_consistency, L.call, ops.rand_uniform, ops.perturb = tc, call, rand, perturb
        yield seen
    finally:
        ops.teacher_consistency, L.call, ops.rand_uniform, ops.perturb = real_tc, real_call, real_rand, real_perturb


@pytest.mark.parametrize("dims,C,extra", [(2, 2, {}), (2, 2, dict(passb_batch=False)), (2, 3, {}), (2, 2, dict(dropout=True)), (2, 3, dict(dropout=True)),
                                          (3, 2, {}), (3, 3, {})],
                         ids=["2d_c2", "2d_c2_single_terms", "2d_c3", "2d_c2_dropout", "2d_c3_dropout", "3d_c2", "3d_c3"])
def test_on_the_launch_in_a_step_matches_the_restatement_and_adds_to_what_mix_loss_bwd_wrote(dims, C, extra):
    step, m, t, (vd, ld, box, injd) = build(dims, C, **dict(ON, **extra))
    step.iter_num = 3000                                                # a consistency weight that is neither 0 nor 1
    with spying() as seen:
        out = step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
    assert len(seen["tc"]) == 1
    rec = seen["tc"][0]
    cw = float(rec["cw"])
    assert rec["accumulate"] is True and rec["gscale"] == W_T and 0.0 < cw < 1.0 and cw == float(step.cw_dev)
    nb = vd.shape[0] // 2
    assert rec["s"][0].shape[:2] == (nb, C) and rec["t"][0].shape == rec["s"][0].shape
    r = tr.teacher_ref([x.cpu() for x in rec["s"]], [x.cpu() for x in rec["t"]], gscale=W_T, gscale_dev=cw, prior=[x.cpu() for x in rec["prior"]])
    worst = kr.check("teacher_loss", rec["loss"].cpu(), r["loss"], r["loss_b"], "i")
    for h in range(2):
        worst = max(worst, kr.check("dlogits %d" % h, rec["g"][h].cpu(), r["g"][h], r["g_b"][h]))
        assert float((rec["g"][h] - rec["prior"][h]).abs().max()) > 0 and bool(torch.isfinite(rec["prior"][h]).all())
    assert torch.equal(out["teacher_loss"], rec["loss"]) and out["teacher_loss"].shape == (1,) and float(rec["loss"]) > 0
    print("  %dD C=%d %s: the launch inside the step, worst err/bound %.3f, teacher_loss %.6f" % (dims, C, extra, worst, float(rec["loss"])))
    # the buffers it added to: the ones the mix_loss backward wrote for the same rows -- the second set (e) when loss_l / loss_u are taken apart
    split = bool(extra.get("dropout"))
    batched = step.passb_batch and C in ops.MIX_LOSS_MULTI_CLASSES
    if batched:
        assert [len(c) for c in seen["bwd"][:2 if split else 1]] == [4] * (2 if split else 1)
        terms = seen["bwd"][1 if split else 0]
    else:
        calls = [c[0] for c in seen["bwd"][:8 if split else 4]]
        terms = calls[1::2] if split else calls
    half = (nb // 2) * C * rec["s"][0][0, 0].numel() * 4                # lsub rows of [C][P] floats
    assert len(terms) == 4 and rec["ptrs"] == [terms[2], terms[3]] and terms[0] == terms[2] + half and terms[1] == terms[3] + half
    if split:
        first = seen["bwd"][0] if batched else [c[0] for c in seen["bwd"][:8]][0::2]
        assert not set(first) & set(terms)                              # the d set is another pair of buffers


def test_on_teacher_logits_are_the_modules_own_and_no_batchnorm_buffer_notices():
    dims, C = 2, 3
    step, m, t, (vd, ld, box, injd) = build(dims, C, inject_teacher=False, **ON)
    off, m_off, t_off, _ = build(dims, C, inject_teacher=False, teacher_consistency=0.0)
    t_before = {k: v.clone() for k, v in t.named_buffers()}
    calls = []
    real_forward = t.forward

    def forward(x, *a, **k):
        count = m._rng.count                                            # where the pass found the student's seed counter
        o = real_forward(x, *a, **k)
        calls.append(dict(x=x.clone(), a=a, k=k, out=[v.clone() for v in o], count=count, training=t.training, rng_is_students=t._rng is m._rng,
                          hold_is_students=t._shift_hold is m._shift_hold and t._shift_hold is not None, shift=t._shift_hold.clone(), grad=torch.is_grad_enabled()))
        return o

    t.forward = forward
    try:
        step._hw = tuple(vd.shape[2:])
        step.prepare(box)
        with spying() as seen:
            step.device_step(vd, ld, injd, update=False)                # the teacher's weights stay what the pass read
            torch.cuda.synchronize()
    finally:
        del t.forward
    assert len(calls) == 1
    c = calls[0]
    assert c["training"] and c["rng_is_students"] and c["hold_is_students"] and not c["grad"] and c["k"].get("update_stats") is False
    assert not t.training and t._shift_hold is None and t._rng is not m._rng            # ... and everything is put back
    # its input: pass B's mixed batch plus the recorded noise
    noise = [p for p in seen["perturb"] if p["out"].shape == c["x"].shape and torch.equal(p["out"], c["x"])]
    assert len(noise) == 1 and noise[0]["alpha"] == 1.0 and noise[0]["mask"] is None and noise[0]["sign"] is False
    # stand-alone: the same module, input, seeds (the student's counter where the pass found it) and shift snapshot
    u_draw = [r for r in seen["rand"] if r["out"] is noise[0]["d"]]
    assert len(u_draw) == 1 and u_draw[0]["seed"] == (m._rng.base << 20) + c["count"]         # the noise seed: the draw right in front of the pass's own
    assert m._rng.count > c["count"]                                    # the pass drew its dropout seeds from the student's generator
    saved = (t._rng, t._shift_hold, t.training, m._rng.count)
    try:
        m._rng.count = c["count"]
        t._rng, t._shift_hold, t.training = m._rng, c["shift"], True
        with torch.no_grad():
            again = real_forward(c["x"], update_stats=False, drop_masks=None)
        torch.cuda.synchronize()
    finally:
        t._rng, t._shift_hold, t.training = saved[:3]
        m._rng.count = saved[3]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, c["out"]))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(seen["tc"][0]["t"], c["out"]))         # what the consistency launch read
    # BatchNorm buffers: the teacher's are untouched, the student's are those of the step without the term (one iteration: the gradients differ from then on)
    assert all(torch.equal(v, t_before[k]) for k, v in t.named_buffers())
    off._hw = step._hw
    off.prepare(box)
    off.device_step(vd, ld, injd, update=False)
    torch.cuda.synchronize()
    sb, ob = dict(m.named_buffers()), dict(m_off.named_buffers())
    assert all(torch.equal(sb[k], ob[k]) for k in sb) and any(not torch.equal(v, t_before[k]) for k, v in sb.items() if k.endswith("running_mean"))
    assert not torch.equal(step.grad_both, off.grad_both)               # the term reached the gradient


def test_on_the_noise_is_the_restated_generators_and_new_at_every_replay():
    dims, C = 2, 2
    step, m, t, (vd, ld, box, injd) = build(dims, C, inject_teacher=False, **ON)
    with spying() as seen:
        step.capture(vd, ld, warmup=1, inject=injd)
    mine = [r for r in seen["rand"] if r["lo"] == -NOISE and r["hi"] == NOISE and r["cap"]]
    assert len(mine) == 1
    r = mine[0]
    pert = [p for p in seen["perturb"] if p["d"] is r["out"]]
    assert len(pert) == 1 and pert[0]["alpha"] == 1.0 and pert[0]["mask"] is None and not pert[0]["sign"] and r["seed_dev"] is m._rng.seed_dev
    us = []
    for k in range(2):
        step.replay(vd, ld, box_yx=box)
        torch.cuda.synchronize()
        u, x, xt = r["out"].clone(), pert[0]["x"].clone(), pert[0]["out"].clone()          # kept alive since the capture: the graph's own buffers
        sd = int(m._rng.seed_dev.item())
        lo32, hi32 = torch.tensor(-NOISE, dtype=torch.float32), torch.tensor(NOISE, dtype=torch.float32)
        assert float(u.min()) >= float(lo32) and float(u.max()) < float(hi32)                # [-a, a) at the fp32 values of the bounds
        assert torch.equal(xt, x + u)                                   # the teacher's input minus x is that noise: x + 1 * u, one rounding
        # lo + fl(hi - lo) * u01 with u01 the 64-bit-integer restatement, exactly: the multiply-add fused (one rounding) or not (two)
        u01 = (kr.u01_int(r["seed"], u.numel(), sd).double() / 16777216.0).reshape(u.shape)
        prod = float(hi32 - lo32) * u01
        fused, unfused = (float(lo32) + prod).float(), (prod.float().double() + float(lo32)).float()
        got = u.cpu()
        assert bool(((got == fused) | (got == unfused)).all())
        us.append(u)
    assert not torch.equal(us[0], us[1])


def test_noise_zero_issues_neither_noise_launch():
    counts = {}
    for name, extra in (("off", dict(teacher_consistency=0.0)), ("zero", dict(teacher_consistency=W_T, teacher_noise=0.0)), ("on", ON)):
        step, m, t, (vd, ld, box, injd) = build(2, 2, inject_teacher=False, **extra)
        rec = Recorder()
        with rec.recording():
            step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
        lines = rec.text().splitlines()
        counts[name] = {k: sum(ln.split()[:2] == ["L", k] for ln in lines) for k in ("chap_rand_uniform", "chap_perturb", "chap_teacher_consistency", "chap_pack_multi")}
    assert counts["zero"]["chap_rand_uniform"] == counts["off"]["chap_rand_uniform"] and counts["zero"]["chap_perturb"] == counts["off"]["chap_perturb"]
    assert counts["on"]["chap_rand_uniform"] == counts["off"]["chap_rand_uniform"] + 1 and counts["on"]["chap_perturb"] == counts["off"]["chap_perturb"] + 1
    assert (counts["off"]["chap_teacher_consistency"], counts["zero"]["chap_teacher_consistency"], counts["on"]["chap_teacher_consistency"]) == (0, 1, 1)


# ---- replay, resume, combinations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,C", CASES, ids=IDS)
def test_replay_equals_eager_teacher_and_teacher_loss_included(dims, C):
    eager, graph = runs_on(dims, C)
    assert len(eager["recs"]) == len(graph["recs"]) == ITERS
    for k, (a, b) in enumerate(zip(eager["recs"], graph["recs"])):
        assert same(a, b) == [], "iteration %d" % (k + 1)
        assert "teacher_loss" in a and bool(torch.isfinite(a["teacher_loss"]).all()) and float(a["teacher_loss"]) >= 0
    # the first update makes the teacher the student; from the second iteration on they differ and so do their predictions
    assert float(eager["recs"][-1]["teacher_loss"]) > 0
    assert len({float(r["teacher_loss"]) for r in eager["recs"]}) > 1


def test_the_term_changes_the_training():
    on, off = runs_on(2, 2)[0], run(2, 2)
    assert not torch.equal(on["recs"][0]["param"], off["recs"][0]["param"])
    assert same({k: v for k, v in on["recs"][0].items() if k.startswith(("stat.", "tstat."))}, {k: v for k, v in off["recs"][0].items() if k.startswith(("stat.", "tstat."))}) == []


def test_resume_three_plus_two_equals_five():
    eager = runs_on(2, 2)[0]
    saved = eager["saved"]
    assert saved["iter_num"] == 3 and set(saved) == set(run(2, 2, iters=1, save_at=1)["saved"])          # state_dict needs nothing new
    cont = run(2, 2, load=saved, start=3, **ON)
    assert len(cont["recs"]) == 2
    for a, b in zip(eager["recs"][3:], cont["recs"]):
        assert same(a, b) == []


@pytest.mark.parametrize("name,kw", [("guard", dict(guard=dict(max_norm=0.0, skip_nonfinite=True))), ("clip", dict(guard=dict(max_norm=1e-3, skip_nonfinite=True))),
                                     ("adamw", dict(optimizer="adamw", base_lr=1e-3, weight_decay=1e-2))], ids=["guard", "clip", "adamw"])
def test_combinations_replay_equals_eager(name, kw):
    eager, graph = run(2, 2, iters=3, **dict(ON, **kw)), run(2, 2, iters=3, graph=True, **dict(ON, **kw))
    for k, (a, b) in enumerate(zip(eager["recs"], graph["recs"])):
        assert same(a, b) == [], "%s iteration %d" % (name, k + 1)
    plain = runs_on(2, 2)[0]
    if name == "guard":                                                 # a guard that neither clips nor skips changes no bit
        assert same(eager["recs"][2], plain["recs"][2]) == []
    else:
        assert not torch.equal(eager["recs"][2]["param"], plain["recs"][2]["param"])


# ---- train() ------------------------------------------------------------------------------------------------------------------------------
def _check_run(path, model_name, log_key):
    names = sorted(os.listdir(path))
    assert {"ema_latest.pth", "%s_ema_best_model.pth" % model_name, "latest.pth", "log.txt"} <= set(names)
    log = open(os.path.join(path, "log.txt")).read()
    lines = [ln for ln in log.splitlines() if "teacher loss" in ln]
    assert len(lines) == 1 and lines[0].startswith("iteration 4 : teacher loss : ") and float(lines[0].rsplit(":", 1)[1]) >= 0
    assert "iteration 4 : %s : " % log_key in log
    for f in ("latest.pth", "ema_latest.pth"):
        assert all(torch.isfinite(v).all() for v in torch.load(os.path.join(path, f), map_location="cpu").values() if v.is_floating_point())
    return log


def test_train_2d_with_the_term(tmp_path):
    from chap_amd.train_ours_2D import train
    common = dict(model="dualdecoder", decoder_type="mcnet", num_classes=3, batch_size=8, labeled_bs=4, image_size=[64, 64], max_iterations=4, val_interval=2,
                  base_lr=0.05, gpu=0, seed=1337, mean_teacher=True)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    train(dict(common, teacher_consistency=0.5), on)
    train(dict(common), off)
    log = _check_run(on, "dualdecoder", "ema_mean_dice")
    assert "teacher loss" not in open(os.path.join(off, "log.txt")).read()
    assert [ln.split(" : ")[0] for ln in log.splitlines() if "teacher loss" not in ln] == [ln.split(" : ")[0] for ln in open(os.path.join(off, "log.txt")).read().splitlines()]


def test_train_3d_with_the_term(tmp_path):
    from chap_amd.train_ours_3D import train
    common = dict(patch_size=[16, 32, 16], num_classes=2, batch_size=4, labeled_bs=2, max_iterations=4, val_interval=2, stride_xy=8, stride_z=8, seed=3,
                  mean_teacher=True)
    on = str(tmp_path / "on")
    train(dict(common, teacher_consistency=0.5), on)
    _check_run(on, "dualdecoder", "ema_dice_score")


# ---- two ranks on one GPU -----------------------------------------------------------------------------------------------------------------
def test_two_ranks_stay_equal_and_draw_their_own_teacher_noise(tmp_path):
    worker = os.path.join(ROOT, "tests", "teacher_consistency_dp_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29600 + os.getpid() % 90
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
    r0, r1 = (torch.load(os.path.join(tmp_path, "tc_rank%d.pt" % r)) for r in range(2))
    for k in ("param", "mom", "ema"):
        assert torch.equal(bits(r0[k]), bits(r1[k])), k
    assert r0["iter_num"] == r1["iter_num"] == r0["it0"] + 3 and bool(torch.isfinite(r0["param"]).all())
    assert not torch.equal(r0["ema"], r0["param"])
    assert all(not torch.equal(a, b) for a, b in zip(r0["noise"], r1["noise"])) and len(r0["noise"]) == 3          # dp_noise_per_rank: each rank its own stream
    assert all(float(u.abs().max()) <= 0.1 for u in r0["noise"] + r1["noise"])
    assert all(float(l) > 0 for l in r0["teacher_loss"][1:])
