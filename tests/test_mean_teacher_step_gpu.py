"""The mean teacher inside the training step, at the smallest 2D (8 x 1 x 64 x 64) and 3D (4 x 1 x 16 x 32 x 16) shapes of the existing step tests,
with two and three classes: the student does not notice it (bit for bit), the teacher is the student after the first update and follows the
fp64 recurrence of tests/ema_ref.py over the recorded student parameters afterwards, capture + replay equals eager (the coefficient
changes with every replay: it is read from device memory), the iteration's launches are the default ones with the optimizer entry replaced,
resume is bit-exact, sync_teacher_stats + eval equals a fresh model loaded with the teacher's state dict, train() of both entries writes the
teacher's files only when asked to, and a 1-rank RCCL group equals the plain step, teacher included."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd.train import ChapStep, build_teacher
from oracle import init as oinit
from tests import ema_ref
from tests import kernel_ref as kr
from tests.iteration_parity import to_dev
from tests.test_class_counts_step_gpu import case_2d, case_3d, make_net

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, DECAY = 5, 0.99
CASES = [(2, 2), (2, 3), (3, 2), (3, 3)]
IDS = ["2d_c2", "2d_c3", "3d_c2", "3d_c3"]


def case(dims, C):
    return case_2d(C) if dims == 2 else case_3d(C)


def build(dims, C, teacher, seed=99, **extra):
    """(step, model, teacher or None, device inputs).  The teacher is initialised with weights of its own (seed): nothing of them may survive."""
    state, vol, lab, box, args, inj = case(dims, C)
    m = make_net(dims, C).to(DEV).train()
    m.load_state_dict(state, strict=True)
    t = None
    if teacher:
        def make():
            torch.manual_seed(seed)
            return make_net(dims, C).to(DEV)
        t = build_teacher(make).eval()
    step = ChapStep(m, dict(args, ema_decay=DECAY, **extra), teacher=t)
    return step, m, t, (vol.to(DEV), lab.to(DEV), box, to_dev(inj, dims))


def snapshot(step, out):
    torch.cuda.synchronize()
    rec = dict(param=step.model.flat_buffers()[0].clone(), mom=step.opt.mom.clone(), iter_num=step.iter_num,
               losses=torch.stack([l.detach().clone() for l in out["mix_losses"]]), vat=out["vat_loss"].detach().clone(),
               stats={k: v.clone() for k, v in step.model.named_buffers()})
    if step.teacher is not None:
        rec["ema"] = step.opt.ema.clone()
        rec["coef"] = step.opt.ema_coef.clone()
    return rec


def run(dims, C, teacher, graph=False, iters=ITERS, save_at=None, load=None, start=0):
    step, m, t, (vd, ld, box, injd) = build(dims, C, teacher)
    ema0 = None if t is None else step.opt.ema.clone()
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
    return dict(recs=recs, ema0=ema0, saved=saved, step=step)


@functools.lru_cache(maxsize=None)
def runs(dims, C):
    plain = run(dims, C, False)
    eager = run(dims, C, True, save_at=3)
    graph = run(dims, C, True, graph=True)
    for r in (plain, graph):
        r.pop("step")
    return plain, eager, graph


def same_student(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("param", "mom", "losses", "vat")) and \
        all(torch.equal(a["stats"][k], b["stats"][k]) for k in a["stats"])


@pytest.mark.parametrize("dims,C", CASES, ids=IDS)
def test_student_is_unchanged_and_teacher_follows_the_recurrence(dims, C):
    plain, eager, _ = runs(dims, C)
    assert len(plain["recs"]) == len(eager["recs"]) == ITERS
    for k, (a, b) in enumerate(zip(plain["recs"], eager["recs"])):
        assert same_student(a, b), "iteration %d: the student differs with a teacher attached" % (k + 1)
        assert b["iter_num"] == k + 1
    first = eager["recs"][0]
    assert not torch.equal(eager["ema0"], first["param"])              # the teacher started elsewhere ...
    assert torch.equal(first["ema"].view(torch.int32), first["param"].view(torch.int32))        # ... and is the student after the first update
    coefs = [ema_ref.coefficients(k, DECAY) for k in range(ITERS)]
    assert coefs[0] == (0.0, 1.0) and [c[0] for c in coefs[1:3]] == [0.5, kr._fp32_scalar(2.0 / 3.0)]
    worst = 0.0
    for k, (rec, (e, bnd)) in enumerate(zip(eager["recs"], ema_ref.ema_recurrence(eager["ema0"].cpu(), [r["param"].cpu() for r in eager["recs"]], coefs))):
        assert rec["coef"].tolist() == list(coefs[k])                  # the words the kernel read at iteration k + 1
        worst = max(worst, kr.check("teacher after iteration %d" % (k + 1), rec["ema"].cpu(), e, bnd, "i"))
    assert float((eager["recs"][-1]["ema"] - eager["recs"][-1]["param"]).abs().max()) > 0          # an average by now, not a copy
    print("  %s teacher vs fp64 recurrence over %d iterations: worst err/bound %.3f" % (IDS[CASES.index((dims, C))], ITERS, worst))


@pytest.mark.parametrize("dims,C", CASES, ids=IDS)
def test_replay_equals_eager_teacher_included(dims, C):
    _, eager, graph = runs(dims, C)
    for k, (a, b) in enumerate(zip(eager["recs"], graph["recs"])):
        assert same_student(a, b), "iteration %d: replay differs from eager" % (k + 1)
        assert torch.equal(a["ema"].view(torch.int32), b["ema"].view(torch.int32)), "iteration %d: the replayed teacher differs" % (k + 1)
        assert torch.equal(a["coef"], b["coef"])
    assert len({tuple(r["coef"].tolist()) for r in graph["recs"]}) == ITERS        # a new coefficient at every replay of the one graph


@pytest.mark.parametrize("dims,mode", [(2, "eager"), (2, "captured"), (3, "eager")])
def test_launches_are_the_default_ones_with_the_optimizer_entry_replaced(dims, mode):
    from tests.issue_trace import Recorder
    texts = []
    for teacher in (False, True):
        step, m, t, (vd, ld, box, injd) = build(dims, 2, teacher)
        rec = Recorder(only_capturing=(mode == "captured"))
        with rec.recording():
            if mode == "captured":
                step.capture(vd, ld, warmup=1, inject=injd)
            else:
                step.step(vd, ld, box_yx=box, inject=injd)
        torch.cuda.synchronize()
        texts.append(rec.text())
    plain, ema = (t.splitlines() for t in texts)
    opt = [i for i, ln in enumerate(plain) if ln.split()[:2] == ["L", "chap_sgd_step"]]
    assert len(opt) == 1 and not any("chap_sgd_ema_step" in ln for ln in plain)
    assert not any(ln.split()[:2] == ["L", "chap_sgd_step"] for ln in ema)
    want = list(plain)
    want[opt[0]] = plain[opt[0]].replace("chap_sgd_step", "chap_sgd_ema_step")          # same position, same stream label
    assert ema == want


def test_resume_is_bit_exact_and_an_old_checkpoint_starts_the_teacher_at_the_student():
    dims, C = 2, 2
    _, eager, _ = runs(dims, C)
    saved = eager["saved"]
    assert saved["iter_num"] == 3 and torch.equal(saved["ema"], eager["recs"][2]["ema"])
    cont = run(dims, C, True, load=saved, start=3)
    for a, b in zip(eager["recs"][3:], cont["recs"]):
        assert same_student(a, b) and torch.equal(a["ema"].view(torch.int32), b["ema"].view(torch.int32)) and torch.equal(a["coef"], b["coef"])
    assert cont["recs"][-1]["iter_num"] == ITERS
    # a checkpoint written without a teacher
    old = {k: v for k, v in saved.items() if k != "ema"}
    step, m, t, _ = build(dims, C, True, seed=5)
    assert not torch.equal(step.opt.ema, m.flat_buffers()[0])
    step.load_state_dict(old)
    torch.cuda.synchronize()
    assert torch.equal(step.opt.ema, m.flat_buffers()[0]) and torch.equal(m.flat_buffers()[0], eager["recs"][2]["param"])
    assert "ema" not in build(dims, C, False)[0].state_dict()


@pytest.mark.parametrize("dims", [2, 3])
def test_sync_teacher_stats_and_eval_equal_a_fresh_model_with_the_teachers_state(dims):
    C = 2
    step, t = runs(dims, C)[1]["step"], runs(dims, C)[1]["step"].teacher
    m = step.model
    sb, tb = dict(m.named_buffers()), dict(t.named_buffers())
    assert any(not torch.equal(sb[k], tb[k]) for k in sb)              # five iterations moved the student's statistics only
    step.sync_teacher_stats()
    assert list(sb) == list(tb) and all(torch.equal(sb[k], tb[k]) for k in sb)
    assert all(not p.requires_grad for p in t.parameters()) and t.compute_dtype == m.compute_dtype
    assert all(torch.equal(p, v) for p, v in zip(t.parameters(), m.grad_views_of(step.opt.ema).values()))    # its parameters ARE the averaged buffer
    x = case(dims, C)[1][:2].to(DEV)
    t.eval()
    fresh = make_net(dims, C).to(DEV).eval()
    fresh.load_state_dict(t.state_dict(), strict=True)
    with torch.no_grad():
        got, want = t(x), fresh(x)
        other = m.eval()(x)
        m.train()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(got[0], other[0])                            # ... and not the student's logits


def _listing(d):
    return sorted(os.listdir(d))


def test_train_2d_writes_the_teacher_only_when_asked(tmp_path):
    from chap_amd.train_ours_2D import train
    C = 3
    common = dict(model="dualdecoder", decoder_type="mcnet", num_classes=C, batch_size=8, labeled_bs=4, image_size=[64, 64], max_iterations=4, val_interval=2,
                  base_lr=0.05, gpu=0, seed=1337)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    train(dict(common, mean_teacher=True), on)
    train(dict(common), off)
    ema_files = ["dualdecoder_ema_best_model.pth", "ema_latest.pth"]
    assert set(ema_files) <= set(_listing(on)) and _listing(off) == [f for f in _listing(on) if f not in ema_files]
    assert {"latest.pth", "log.txt"} <= set(_listing(off)) <= {"latest.pth", "log.txt", "dualdecoder_best_model.pth", "val.csv"}
    log_on, log_off = open(os.path.join(on, "log.txt")).read(), open(os.path.join(off, "log.txt")).read()
    assert "iteration 2 : ema_mean_dice : " in log_on and "iteration 4 : ema_mean_dice : " in log_on and "ema" not in log_off
    assert [ln for ln in log_on.splitlines() if "ema_" not in ln] == log_off.splitlines()       # the student's lines, figures included
    keys = list(oinit.dual_decoder_2d_state(1, n_class=C).keys())
    student = torch.load(os.path.join(on, "latest.pth"), map_location="cpu")
    student_off = torch.load(os.path.join(off, "latest.pth"), map_location="cpu")
    assert all(torch.equal(student[k], student_off[k]) for k in keys)  # same seeds: building and averaging the teacher took nothing from the student
    for f in ema_files:
        ck = torch.load(os.path.join(on, f), map_location="cpu")
        assert list(ck.keys()) == keys
        make_net(2, C).load_state_dict(ck, strict=True)
        assert all(torch.isfinite(v).all() for v in ck.values())
    ck = torch.load(os.path.join(on, "ema_latest.pth"), map_location="cpu")
    assert all(torch.equal(ck[k], student[k]) for k in keys if k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    assert any(not torch.equal(ck[k], student[k]) for k in keys if k.endswith("weight"))


def test_train_3d_writes_the_teacher_only_when_asked(tmp_path):
    from chap_amd.train_ours_3D import train
    C = 2
    common = dict(patch_size=[16, 32, 16], num_classes=C, batch_size=4, labeled_bs=2, max_iterations=4, val_interval=2, stride_xy=8, stride_z=8, seed=3)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    train(dict(common, mean_teacher=True), on)
    train(dict(common), off)
    ema_files = ["dualdecoder_ema_best_model.pth", "ema_latest.pth"]
    assert set(ema_files) <= set(_listing(on)) and _listing(off) == [f for f in _listing(on) if f not in ema_files]
    log_on, log_off = open(os.path.join(on, "log.txt")).read(), open(os.path.join(off, "log.txt")).read()
    assert "iteration 2 : ema_dice_score : " in log_on and "iteration 4 : ema_dice_score : " in log_on and "ema" not in log_off
    assert [ln for ln in log_on.splitlines() if "ema_" not in ln] == log_off.splitlines()
    keys = list(oinit.dual_decoder_3d_state(1, n_class=C).keys())
    student = torch.load(os.path.join(on, "latest.pth"), map_location="cpu")
    student_off = torch.load(os.path.join(off, "latest.pth"), map_location="cpu")
    assert all(torch.equal(student[k], student_off[k]) for k in keys)
    for f in ema_files:
        ck = torch.load(os.path.join(on, f), map_location="cpu")
        assert list(ck.keys()) == keys
        make_net(3, C).load_state_dict(ck, strict=True)
        assert all(torch.isfinite(v).all() for v in ck.values())


def test_one_rank_rccl_group_equals_the_plain_step_teacher_included(tmp_path):
    """tests/test_parallel_gpu.py::test_one_rank_nccl_group_equals_the_plain_step with a teacher (tests/mean_teacher_dp_worker.py): the four-graph
    replay ends in the optimizer graph, which now holds the fused entry."""
    worker = os.path.join(ROOT, "tests", "mean_teacher_dp_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29500 + os.getpid() % 100
    p = subprocess.run([sys.executable, worker, "--out", str(tmp_path), "--port", str(port)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    ref, got = torch.load(os.path.join(tmp_path, "nodp.pt")), torch.load(os.path.join(tmp_path, "dp.pt"))
    assert float(got["buckets"].abs().max()) == 0.0 and got["iter_num"] == ref["iter_num"] and (ref["graphs"], got["graphs"]) == (1, 4)
    for k in ("param", "mom", "ema", "losses"):
        assert torch.equal(ref[k].view(torch.int32), got[k].view(torch.int32)), k
    assert not torch.equal(ref["ema"], ref["param"]) and not torch.equal(ref["ema"], ref["ema0"])
