"""The uncertainty-aware teacher consistency inside the training step, at the step cases of tests/test_teacher_consistency_step_gpu.py (2D
8 x 1 x 64 x 64, 3D 4 x 1 x 16 x 32 x 16, two and three classes), whose helpers this file uses.  Off (teacher_uncertainty = 0) the step is the
teacher-consistency step, launch for launch and bit for bit.  On: the two launches are checked against tests/uncertainty_ref.py on the tensors
they got inside a real step -- the recorded teacher logits of all T passes, the threshold word of the schedule block -- and the gradient is added
to the buffers mix_loss_bwd wrote (the e set with `dropout`); the T noise draws are the restated generator's and differ; T = 1 runs the
teacher once; capture + replay equals eager, teacher_loss and teacher_certain included; the threshold word follows the schedule across replays;
resume is bit-exact; a guard and a clipping guard combine with it; train() of both entries logs the share and the threshold; two data-parallel
ranks stay equal."""
import contextlib
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from chap_amd.train import uncertainty_threshold
from tests import kernel_ref as kr
from tests import test_teacher_consistency_step_gpu as base
from tests import uncertainty_ref as ur
from tests.issue_trace import Recorder

DEV = "cuda"
ROOT = base.ROOT
ITERS, W_T, NOISE = 5, base.W_T, base.NOISE
ON_TC = base.ON
bits, same = base.bits, base.same


def on(T, **extra):
    return dict(ON_TC, teacher_uncertainty=T, **extra)


def build(dims, C, T=0, per_pass_noise=True, **extra):
    """base.build with the option; the injected teacher noise becomes one static tensor per pass (the dropout masks stay shared)."""
    step, m, t, (vd, ld, box, injd) = base.build(dims, C, **(on(T, **extra) if T else dict(ON_TC, **extra)))
    if T > 1 and per_pass_noise and "teacher_u" in injd:
        u0 = injd["teacher_u"]
        injd["teacher_u"] = [u0] + [((torch.rand(u0.shape, generator=torch.Generator().manual_seed(78 + k)) * 2 - 1) * NOISE).to(DEV) for k in range(1, T)]
    return step, m, t, (vd, ld, box, injd)


def snapshot(step, out):
    rec = base.snapshot(step, out)
    if "teacher_certain" in out:
        rec["teacher_certain"] = out["teacher_certain"].detach().clone()
    return rec


def run(dims, C, T=0, graph=False, iters=ITERS, save_at=None, load=None, start=0, **extra):
    step, m, t, (vd, ld, box, injd) = build(dims, C, T, **extra)
    if load is not None:
        step.load_state_dict(load)
    if graph:
        step.capture(vd, ld, warmup=1, inject=injd)
    recs, saved, thr = [], None, []
    for k in range(start, iters):
        out = step.replay(vd, ld, box_yx=box) if graph else step.step(vd, ld, box_yx=box, inject=injd)
        recs.append(snapshot(step, out))
        if step.thr_dev is not None:
            thr.append((step.iter_num - 1, float(step.thr_dev)))
        if save_at == k + 1:
            saved = step.state_dict()
    return dict(recs=recs, saved=saved, thr=thr, pixels=step.teacher_pixels)


@functools.lru_cache(maxsize=None)
def runs_on(dims, C, T=2):
    return run(dims, C, T, save_at=3), run(dims, C, T, graph=True)


# ---- off is the parent ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,C", base.CASES, ids=base.IDS)
def test_off_five_iterations_are_the_teacher_consistency_steps_bit_for_bit(dims, C):
    parent = base.run(dims, C, **ON_TC)                                 # the arguments absent: the step as it was
    off = run(dims, C, teacher_uncertainty=0, uncertainty_threshold=(0.5, 0.6))
    for k, (a, b) in enumerate(zip(parent["recs"], off["recs"])):
        assert same(a, b) == [], "iteration %d" % (k + 1)
        assert "teacher_certain" not in b and "teacher_loss" in b


@pytest.mark.parametrize("dims,mode", [(2, "eager"), (2, "captured"), (3, "eager")])
def test_off_the_launch_list_is_the_teacher_consistency_steps(dims, mode):
    texts = []
    for extra in ({}, dict(teacher_uncertainty=0)):
        step, m, t, (vd, ld, box, injd) = base.build(dims, 2, **dict(ON_TC, **extra))
        assert step._sched.numel() == 10 and step.thr_dev is None
        rec = Recorder(only_capturing=(mode == "captured"))
        with rec.recording():
            if mode == "captured":
                step.capture(vd, ld, warmup=1, inject=injd)
            else:
                step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
        texts.append(rec.text())
    assert texts[0] == texts[1] and "chap_teacher_uncertainty" not in texts[0] and "chap_teacher_consistency_masked" not in texts[0]
    assert "chap_teacher_consistency" in texts[0]


# ---- on: the two launches inside a real step ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def spying():
    """base.spying() plus ops.teacher_uncertainty and ops.teacher_consistency_masked (tensors in and out).  Everything calls through."""
    real_tu, real_tm = ops.teacher_uncertainty, ops.teacher_consistency_masked
    with base.spying() as seen:
        seen.update(tu=[], tm=[])

        def tu(passes, threshold=0.0, threshold_dev=None, want_entropy=False, ws=None):
            out = real_tu(passes, threshold, threshold_dev, want_entropy, ws)
            seen["tu"].append(dict(passes=[[z.detach().clone() for z in pair] for pair in passes], ptrs=[[z.data_ptr() for z in pair] for pair in passes],
                                   thr=threshold_dev.clone(), mask=out[0].clone(), count=out[1].clone(), out=out, stream=torch.cuda.current_stream().cuda_stream))
            return out

        def tm(logits, teacher, mask, count, loss, dlogits=(None, None), gscale=1.0, gscale_dev=None, accumulate=False, ws=None):
            rec = dict(s=[t.detach().clone() for t in logits], t=[t.detach().clone() for t in teacher], tptrs=[t.data_ptr() for t in teacher], mask=mask, count=count,
                       prior=[d.clone() for d in dlogits], gscale=gscale, cw=gscale_dev.clone(), accumulate=accumulate, ptrs=[d.data_ptr() for d in dlogits],
                       stream=torch.cuda.current_stream().cuda_stream)
            real_tm(logits, teacher, mask, count, loss, dlogits, gscale, gscale_dev, accumulate, ws)
            rec.update(g=[d.clone() for d in dlogits], loss=loss.clone())
            seen["tm"].append(rec)
        try:
            ops.teacher_uncertainty, ops.teacher_consistency_masked = tu, tm
            yield seen
        finally:
            ops.teacher_uncertainty, ops.teacher_consistency_masked = real_tu, real_tm


@pytest.mark.parametrize("dims,C,T,extra", [(2, 2, 1, {}), (2, 2, 3, {}), (2, 2, 3, dict(passb_batch=False)), (2, 3, 3, {}), (2, 2, 1, dict(dropout=True)),
                                            (2, 3, 3, dict(dropout=True)), (3, 2, 3, {}), (3, 3, 1, {})],
                         ids=["2d_c2_t1", "2d_c2_t3", "2d_c2_t3_single_terms", "2d_c3_t3", "2d_c2_t1_dropout", "2d_c3_t3_dropout", "3d_c2_t3", "3d_c3_t1"])
def test_on_the_launches_in_a_step_match_the_restatement_and_add_to_what_mix_loss_bwd_wrote(dims, C, T, extra):
    step, m, t, (vd, ld, box, injd) = build(dims, C, T, **extra)
    step.iter_num = 3000                                                # a consistency weight that is neither 0 nor 1
    with spying() as seen:
        out = step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
    assert len(seen["tu"]) == 1 and len(seen["tm"]) == 1 and seen["tc"] == []          # the masked launch REPLACES the plain one
    u, rec = seen["tu"][0], seen["tm"][0]
    # the uncertainty launch: all T passes, the threshold word of the schedule block (this iteration's value)
    thr = float(u["thr"])
    assert len(u["passes"]) == T and thr == kr._fp32_scalar(uncertainty_threshold(3000, step.args)) == float(step.thr_dev) and u["stream"] == rec["stream"]
    assert len({p for pair in u["ptrs"] for p in pair}) == 2 * T
    nb = vd.shape[0] // 2
    assert all(z.shape[:2] == (nb, C) for pair in u["passes"] for z in pair)
    if T > 1:
        assert not torch.equal(u["passes"][0][0], u["passes"][1][0])   # its own noise: another prediction
    r = ur.uncertainty_ref([[z.cpu() for z in pair] for pair in u["passes"]], thr)
    # (a network's logits are no test vector: the band's share is whatever the model gives, so only the decided pixels and the count's range are asserted)
    got = u["mask"].cpu().reshape(r["mask"].shape)
    assert not bool(((got.bool() != r["mask"]) & ~r["undecided"]).any())
    count = int(u["count"])
    assert count == int(got.sum()) and r["sure"] <= count <= r["sure"] + r["n_undecided"]
    assert step.teacher_pixels == got.numel() and 0 <= count <= got.numel()
    # the masked launch: pass 0 is the target, the kernel's own mask and count, the same gscale / cw / accumulate as the plain term
    cw = float(rec["cw"])
    assert rec["accumulate"] is True and rec["gscale"] == W_T and 0.0 < cw < 1.0 and cw == float(step.cw_dev)
    assert rec["tptrs"] == u["ptrs"][0] and rec["mask"] is u["out"][0] and rec["count"] is u["out"][1]
    mr = ur.masked_ref([x.cpu() for x in rec["s"]], [x.cpu() for x in rec["t"]], got, count, gscale=W_T, gscale_dev=cw, prior=[x.cpu() for x in rec["prior"]])
    worst = kr.check("teacher_loss", rec["loss"].cpu(), mr["loss"], mr["loss_b"], "i")
    off = (got == 0).unsqueeze(1)
    for h in range(2):
        worst = max(worst, kr.check("dlogits %d" % h, rec["g"][h].cpu(), mr["g"][h], mr["g_b"][h]))
        assert bool(torch.isfinite(rec["prior"][h]).all())
        sel = off.expand_as(rec["g"][h]).to(rec["g"][h].device)
        assert torch.equal(bits(rec["g"][h])[sel], bits(rec["prior"][h])[sel])           # masked out: what mix_loss_bwd wrote, bit for bit
        if count:
            assert float((rec["g"][h] - rec["prior"][h]).abs().max()) > 0
    assert torch.equal(out["teacher_loss"], rec["loss"]) and out["teacher_loss"].shape == (1,)
    assert out["teacher_certain"] is u["out"][1] and out["teacher_certain"].dtype == torch.int64
    print("  %dD C=%d T=%d %s: worst err/bound %.3f, teacher_loss %.6f, certain %d of %d, threshold %.4f" % (dims, C, T, extra, worst, float(rec["loss"]), count, got.numel(), thr))
    # the buffers it added to: the ones the mix_loss backward wrote for the same rows -- the second set (e) when loss_l / loss_u are taken apart
    split = bool(extra.get("dropout"))
    batched = step.passb_batch and C in ops.MIX_LOSS_MULTI_CLASSES
    if batched:
        terms = seen["bwd"][1 if split else 0]
    else:
        calls = [c[0] for c in seen["bwd"][:8 if split else 4]]
        terms = calls[1::2] if split else calls
    half = (nb // 2) * C * rec["s"][0][0, 0].numel() * 4
    assert len(terms) == 4 and rec["ptrs"] == [terms[2], terms[3]] and terms[0] == terms[2] + half and terms[1] == terms[3] + half


def test_the_noise_draws_are_the_restated_generators_and_the_teacher_runs_t_times():
    """Drawn, not injected.  T draws from the student's generator, behind pass B's own seeds, each the restated generator's and each another tensor;
    T = 1 runs the teacher as often as the plain term does (once), T = 3 three times; the student's pass B draws what it draws without the option."""
    dims, C = 2, 2
    calls, draws, counts = {}, {}, {}
    for T in (0, 1, 3):
        step, m, t, (vd, ld, box, injd) = base.build(dims, C, inject_teacher=False, **(on(T) if T else ON_TC))
        n, real_forward = [], t.forward

        def forward(x, *a, _n=n, _f=real_forward, _m=m, **k):
            _n.append(_m._rng.count)
            return _f(x, *a, **k)
        t.forward = forward
        try:
            with spying() as seen:
                step.step(vd, ld, box_yx=box, inject=injd)
                torch.cuda.synchronize()
        finally:
            del t.forward
        calls[T], counts[T] = len(n), n
        mine = [r for r in seen["rand"] if r["lo"] == -NOISE and r["hi"] == NOISE]
        draws[T] = mine
        sd = int(m._rng.seed_dev.item())
        lo32, hi32 = torch.tensor(-NOISE, dtype=torch.float32), torch.tensor(NOISE, dtype=torch.float32)
        for r, c in zip(mine, n):
            assert r["seed"] == (m._rng.base << 20) + c - 1 or r["seed"] == (m._rng.base << 20) + c          # the draw right in front of the pass's own
            u = r["out"]
            u01 = (kr.u01_int(r["seed"], u.numel(), sd).double() / 16777216.0).reshape(u.shape)
            prod = float(hi32 - lo32) * u01
            fused, unfused = (float(lo32) + prod).float(), (prod.float().double() + float(lo32)).float()
            assert bool(((u.cpu() == fused) | (u.cpu() == unfused)).all())
    assert (calls[0], calls[1], calls[3]) == (1, 1, 3) and [len(draws[T]) for T in (0, 1, 3)] == [1, 1, 3]
    assert counts[0][0] == counts[1][0] == counts[3][0]                 # pass 0 finds the student's counter where the plain term's pass finds it
    assert draws[3][0]["seed"] == draws[0][0]["seed"] and len({r["seed"] for r in draws[3]}) == 3
    assert torch.equal(draws[3][0]["out"], draws[0][0]["out"])
    assert not torch.equal(draws[3][0]["out"], draws[3][1]["out"]) and not torch.equal(draws[3][1]["out"], draws[3][2]["out"])


# ---- replay, schedule, resume, combinations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,C", base.CASES, ids=base.IDS)
def test_replay_equals_eager_teacher_loss_and_count_included(dims, C):
    eager, graph = runs_on(dims, C)
    assert len(eager["recs"]) == len(graph["recs"]) == ITERS
    for k, (a, b) in enumerate(zip(eager["recs"], graph["recs"])):
        assert same(a, b) == [], "iteration %d" % (k + 1)
        assert bool(torch.isfinite(a["teacher_loss"]).all()) and float(a["teacher_loss"]) >= 0 and 0 <= int(a["teacher_certain"]) <= eager["pixels"]
    assert eager["pixels"] > 0 and any(int(r["teacher_certain"]) > 0 for r in eager["recs"])
    assert eager["thr"] == graph["thr"]


def test_the_threshold_word_follows_the_schedule_across_replays():
    """max_iterations = 8: the ramp moves at every step.  The word is the LAST of the schedule block, behind the teacher's two."""
    extra = dict(max_iterations=8, uncertainty_threshold=(0.5, 0.95))
    for graph in (False, True):
        r = run(2, 2, 2, graph=graph, iters=4, **extra)
        assert [i for i, _ in r["thr"]] == [0, 1, 2, 3]
        want = [kr._fp32_scalar((0.5 + 0.45 * math.exp(-5.0 * (1.0 - i / 8.0) ** 2)) * math.log(2)) for i in range(4)]
        assert [v for _, v in r["thr"]] == want and len(set(want)) == 4
    step, m, t, _ = build(2, 2, 2, **extra)
    assert step._sched.numel() == 11 and step.thr_dev.data_ptr() == step._sched[10:].data_ptr()
    assert step.opt.ema_coef.data_ptr() == step._sched[8:10].data_ptr() and step.cw_dev.data_ptr() == step._sched[6:7].data_ptr()


def test_the_mask_changes_the_training_and_t1_differs_from_the_plain_term():
    masked, plain = run(2, 2, 1, iters=3), base.run(2, 2, iters=3, **ON_TC)
    assert not torch.equal(masked["recs"][2]["param"], plain["recs"][2]["param"])
    assert any(int(r["teacher_certain"]) < masked["pixels"] for r in masked["recs"])


def test_resume_three_plus_two_equals_five():
    eager = runs_on(2, 2)[0]
    saved = eager["saved"]
    assert saved["iter_num"] == 3 and set(saved) == set(base.run(2, 2, iters=1, save_at=1)["saved"])          # state_dict gains nothing
    cont = run(2, 2, 2, load=saved, start=3)
    assert len(cont["recs"]) == 2
    for a, b in zip(eager["recs"][3:], cont["recs"]):
        assert same(a, b) == []


@pytest.mark.parametrize("name,kw", [("guard", dict(guard=dict(max_norm=0.0, skip_nonfinite=True))), ("clip", dict(guard=dict(max_norm=1e-3, skip_nonfinite=True)))],
                         ids=["guard", "clip"])
def test_guard_combinations_replay_equals_eager(name, kw):
    eager, graph = run(2, 2, 2, iters=3, **kw), run(2, 2, 2, iters=3, graph=True, **kw)
    for k, (a, b) in enumerate(zip(eager["recs"], graph["recs"])):
        assert same(a, b) == [], "%s iteration %d" % (name, k + 1)
    plain = runs_on(2, 2)[0]
    if name == "guard":                                                 # a guard that neither clips nor skips changes no bit
        assert same(eager["recs"][2], plain["recs"][2]) == []
    else:
        assert not torch.equal(eager["recs"][2]["param"], plain["recs"][2]["param"])


# ---- train() ------------------------------------------------------------------------------------------------------------------------------
def _check_log(path, C, max_iterations, lo_hi):
    log = open(os.path.join(path, "log.txt")).read()
    lines = [ln for ln in log.splitlines() if "teacher loss" in ln]
    assert len(lines) == 1 and lines[0].startswith("iteration %d : teacher loss : " % max_iterations)
    f = [s.strip() for s in lines[0].split(" : ")]
    assert f[1] == "teacher loss" and f[3] == "certain share" and f[5] == "entropy threshold" and len(f) == 7
    assert float(f[2]) >= 0 and 0.0 <= float(f[4]) <= 1.0
    want = uncertainty_threshold(max_iterations - 1, dict(num_classes=C, max_iterations=max_iterations, uncertainty_threshold=lo_hi))
    assert abs(float(f[6]) - want) < 1e-6
    assert {"ema_latest.pth", "latest.pth"} <= set(os.listdir(path))


def test_train_2d_logs_the_share_and_the_threshold(tmp_path):
    from chap_amd.train_ours_2D import train
    common = dict(model="dualdecoder", decoder_type="mcnet", num_classes=3, batch_size=8, labeled_bs=4, image_size=[64, 64], max_iterations=4, val_interval=2,
                  base_lr=0.05, gpu=0, seed=1337, mean_teacher=True, teacher_consistency=0.5)
    path = str(tmp_path / "on")
    train(dict(common, teacher_uncertainty=2, uncertainty_threshold=(0.6, 0.9)), path)
    _check_log(path, 3, 4, (0.6, 0.9))


def test_train_3d_logs_the_share_and_the_threshold(tmp_path):
    from chap_amd.train_ours_3D import train
    common = dict(patch_size=[16, 32, 16], num_classes=2, batch_size=4, labeled_bs=2, max_iterations=4, val_interval=2, stride_xy=8, stride_z=8, seed=3,
                  mean_teacher=True, teacher_consistency=0.5)
    path = str(tmp_path / "on")
    train(dict(common, teacher_uncertainty=1), path)
    _check_log(path, 2, 4, (0.75, 1.0))


# ---- two ranks on one GPU -----------------------------------------------------------------------------------------------------------------
def test_two_ranks_stay_equal_each_with_its_own_count(tmp_path):
    worker = os.path.join(ROOT, "tests", "teacher_uncertainty_dp_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29700 + os.getpid() % 90
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
    r0, r1 = (torch.load(os.path.join(tmp_path, "tu_rank%d.pt" % r)) for r in range(2))
    for k in ("param", "mom", "ema"):
        assert torch.equal(bits(r0[k]), bits(r1[k])), k
    assert r0["iter_num"] == r1["iter_num"] == r0["it0"] + 3 and bool(torch.isfinite(r0["param"]).all())
    assert len(r0["noise"]) == len(r1["noise"]) == 6                    # two passes a step, each rank its own stream
    assert all(not torch.equal(a, b) for a, b in zip(r0["noise"], r1["noise"]))
    assert all(0 <= c <= r0["pixels"] for c in r0["teacher_certain"] + r1["teacher_certain"]) and r0["pixels"] == r1["pixels"] > 0
    assert all(math.isfinite(l) and l >= 0 for l in r0["teacher_loss"] + r1["teacher_loss"])
