"""Host side of the uncertainty-aware teacher consistency (no GPU): the fp64 restatements of tests/uncertainty_ref.py against autograd, their
bounds against an fp32 emulation of each kernel and against seven planted faults, the undecided share of every input case, the header
include/chap_hip_uncertainty.h against the binding, the entries' argument checks (which return before anything is launched),
check_teacher_uncertainty's refusals in ChapStep, AblationStep and both train() entries, and the threshold schedule."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from tests import kernel_ref as kr
from tests import uncertainty_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chap_hip_uncertainty.h")
ENTRIES = ["chap_teacher_consistency_masked", "chap_teacher_uncertainty"]


@pytest.mark.parametrize("C", [3, 8])
def test_restatements_are_the_masked_loss_and_its_gradient(C):
    """uncertainty_ref against a plain fp64 formula, masked_ref against fp64 autograd of sum_h sum m (softmax(s_h) - q)^2 / (C count + 1e-16)."""
    x = ur.inputs(C, ur.SCALAR, 2)
    thr = ur.threshold(0.75, C)
    r = ur.uncertainty_ref(x["t"], thr)
    pbar = sum(torch.softmax(z.double(), 1) for pair in x["t"] for z in pair) / 4
    H = -(pbar * torch.log(pbar + 1e-6)).sum(1)
    assert (r["H"] - H).abs().max() <= 1e-14 and torch.equal(r["mask"], H < thr)
    assert 0 < int(r["mask"].sum()) < H.numel()
    mask, count = r["mask"].to(torch.uint8), int(r["mask"].sum())
    s = [t.double().requires_grad_(True) for t in x["s"]]
    q = 0.5 * (torch.softmax(x["t"][0][0].double(), 1) + torch.softmax(x["t"][0][1].double(), 1))
    m = r["mask"].unsqueeze(1).double()
    loss = sum((m * (torch.softmax(t, 1) - q) ** 2).sum() for t in s) / (C * count + 1e-16)
    loss.backward()
    loss = loss.detach()
    mr = ur.masked_ref(x["s"], x["t"][0], mask, count)
    assert abs(float(mr["loss"]) - float(loss)) <= 1e-13 * float(loss) and float(loss) > 1e-3
    for h in range(2):
        assert (mr["g"][h] - s[h].grad).abs().max() <= 1e-15 and s[h].grad.abs().max() > 1e-6
        assert bool((mr["g"][h][(m == 0).expand_as(mr["g"][h])] == 0).all())
    prior = (torch.randn_like(x["s"][0]), None)
    m2 = ur.masked_ref(x["s"], x["t"][0], mask, count, gscale=0.25, gscale_dev=3.0, prior=prior)
    assert (m2["g"][0] - (prior[0].double() + 0.75 * s[0].grad)).abs().max() <= 1e-15
    assert (m2["g"][1] - 0.75 * s[1].grad).abs().max() <= 1e-15 and m2["loss"] == mr["loss"]
    # count = 0: loss 0, gradient 0 (the prior), no NaN
    z = ur.masked_ref(x["s"], x["t"][0], torch.zeros_like(mask), 0, prior=prior)
    assert float(z["loss"]) == 0.0 and torch.equal(z["g"][0], prior[0].double()) and float(z["g"][1].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [ur.SCALAR, ur.QUADS], ids=["17x19", "16x20"])
@pytest.mark.parametrize("T", ur.PASSES)
@pytest.mark.parametrize("C", ur.CLASSES)
def test_undecided_share_and_both_mask_values_on_the_reference_alone(C, T, shape):
    x = ur.inputs(C, shape, T)
    for frac in ur.FRACTIONS:
        r = ur.uncertainty_ref(x["t"], ur.threshold(frac, C))
        assert r["n_undecided"] / r["mask"].numel() <= ur.UNDECIDED_CAP, (frac, r["n_undecided"])
        assert 0 < r["sure"] < r["mask"].numel() - r["n_undecided"]                     # both values occur
        flat = lambda v: v.reshape(x["N"], x["P"])
        und, H = flat(r["undecided"]), flat(r["H"])
        # the planted pixels are outside the band: saturated agreement, one-hot contradiction, uniform
        assert not bool(und[0, 3::31].any()) and float(H[0, 3::31].max()) < 1e-3
        assert not bool(und[0, 7::43].any()) and float((H[0, 7::43] - math.log(2)).abs().max()) < 1e-4
        assert not bool(und[-1, 13::47].any()) and float((H[-1, 13::47] - math.log(C)).abs().max()) < 1e-4
        if C == 2:
            assert not bool(flat(r["mask"])[0, 7::43].any())


@pytest.mark.parametrize("shape", [ur.SCALAR, ur.QUADS], ids=["17x19", "16x20"])
@pytest.mark.parametrize("C", ur.CLASSES)
def test_fp32_emulations_are_inside_the_bounds_and_every_planted_fault_is_outside(C, shape):
    for T in (1, 3):
        x = ur.inputs(C, shape, T)
        thr = ur.threshold(0.9, C)
        r = ur.uncertainty_ref(x["t"], thr)
        H, mask, count = ur.emulate_uncertainty_f32(x["t"], thr)
        assert kr.check("H", H, r["H"], r["H_b"]) <= 1.0
        ur.check_mask("mask", mask, count, r)
        for fault in ur.UNCERTAINTY_FAULTS:
            Hf, _, _ = ur.emulate_uncertainty_f32(x["t"], thr, fault=fault)
            with pytest.raises(AssertionError, match="worst element"):
                kr.check("H " + fault, Hf, r["H"], r["H_b"])
        g = torch.Generator().manual_seed(9)
        prior = tuple(0.01 * torch.randn(x["s"][0].shape, generator=g) for _ in range(2))
        m8, cnt = r["mask"].to(torch.uint8), int(r["mask"].sum())
        for pr, gs, gd in (((None, None), 1.0, None), (prior, 0.3, 0.7)):
            mr = ur.masked_ref(x["s"], x["t"][0], m8, cnt, gscale=gs, gscale_dev=gd, prior=pr)
            loss, gg = ur.emulate_masked_f32(x["s"], x["t"][0], m8, cnt, gscale=gs, gscale_dev=gd, prior=pr)
            assert kr.check("loss", loss, mr["loss"], mr["loss_b"], "i") <= 1.0
            for h in range(2):
                assert kr.check("g%d" % h, gg[h], mr["g"][h], mr["g_b"][h]) <= 1.0
            for fault in ur.MASKED_FAULTS:
                loss_f, gf = ur.emulate_masked_f32(x["s"], x["t"][0], m8, cnt, gscale=gs, gscale_dev=gd, prior=pr, fault=fault)
                for h in range(2):
                    with pytest.raises(AssertionError, match="worst element"):
                        kr.check("g%d %s" % (h, fault), gf[h], mr["g"][h], mr["g_b"][h])
                if fault != "mask_loss_only":
                    with pytest.raises(AssertionError, match="worst element"):
                        kr.check("loss " + fault, loss_f, mr["loss"], mr["loss_b"], "i")


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const char\*)\s+(chap_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entries_and_abi_is_still_9():
    from chap_amd import _lib
    src = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s_params\s*\*\s*p\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (name, name), src)
    assert re.search(r'^#include "chap_hip\.h"$', src, flags=re.M)
    assert re.search(r"#define\s+CHAP_ABI_VERSION\s+9\b", open(os.path.join(ROOT, "include", "chap_hip.h")).read())
    assert _declared(HEADER) == sorted(_lib._UNCERTAINTY_SIGS) == ENTRIES
    others = (set(_lib._SIGS) | set(_lib._SIGS_EXT) | set(_lib._SIGS_MONITOR) | set(_lib._SIGS_GUARD) | set(_lib._OPTIM_SIGS) | set(_lib._TEACHER_SIGS)
              | set(_lib._SIZE_FNS))
    assert not set(_lib._UNCERTAINTY_SIGS) & others
    assert not [n for n in vars(_lib) if n.startswith("_SIGS") and getattr(_lib, n) is _lib._UNCERTAINTY_SIGS]
    assert _lib._UNCERTAINTY_SIGS["chap_teacher_uncertainty"] is _lib.TeacherUncertaintyParams
    assert _lib._UNCERTAINTY_SIGS["chap_teacher_consistency_masked"] is _lib.TeacherConsistencyMaskedParams
    lib = _lib.lib()
    assert lib.chap_abi_version() == _lib.ABI_VERSION == 9
    for name in ENTRIES:
        assert hasattr(lib, name)
        fn = _lib._fn(name)
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(_lib._UNCERTAINTY_SIGS[name])


@pytest.mark.parametrize("name", ENTRIES)
def test_ctypes_structs_match_header(tmp_path, name):
    from chap_amd import _lib, ops
    st = _lib._UNCERTAINTY_SIGS[name]
    fields = [f[0] for f in st._fields_]
    c = tmp_path / "sz.c"
    body = 'printf("size %%zu\\n", sizeof(%s_params));\n' % name
    body += "".join('printf("%s %%zu\\n", offsetof(%s_params, %s));\n' % (f, name, f) for f in fields)
    body += 'printf("slots %d\\n", CHAP_LOSS_SLOTS);\nprintf("maxt %d\\n", CHAP_UNCERTAINTY_MAX_T);\n'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip_uncertainty.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got["size"]) == ctypes.sizeof(st)
    for f in fields:
        assert int(got[f]) == getattr(st, f).offset, f
    assert int(got["slots"]) == _lib.LOSS_SLOTS and ops.teacher_uncertainty_ws_words() == 1 + _lib.LOSS_SLOTS
    assert int(got["maxt"]) == _lib.UNCERTAINTY_MAX_T == 8


def _uparams(**over):
    """Made-up, aligned, non-null addresses: every check below fails before a launch, nothing is dereferenced."""
    from chap_amd import _lib
    q = _lib.TeacherUncertaintyParams()
    v = dict(T=2, N=4, C=4, P=320, mask=0x70000, count=0x80000, ws=0x90000, entropy=0xa0000, null_pass=None, odd=None)
    v.update(over)
    for k in range(8):
        for h in range(2):
            q.teacher[k][h] = 0x100000 * (1 + 2 * k + h) if k < max(v["T"], 0) else 0
    if v["null_pass"] is not None:
        q.teacher[v["null_pass"]][1] = 0
    if v["odd"] is not None:
        q.teacher[v["odd"]][0] = q.teacher[v["odd"]][0] + 2
    q.mask, q.count, q.ws, q.entropy, q.threshold = v["mask"], v["count"], v["ws"], v["entropy"], 0.5
    q.T, q.N, q.C, q.P = v["T"], v["N"], v["C"], v["P"]
    return q


@pytest.mark.parametrize("over,match", [(dict(C=9), r"chap_teacher_uncertainty: C=9 \(2\.\.8 built\)"), (dict(C=1), r"chap_teacher_uncertainty: C=1 \(2\.\.8 built\)"),
                                        (dict(T=0), r"chap_teacher_uncertainty: T=0 \(1\.\.8 built\)"), (dict(T=9), r"chap_teacher_uncertainty: T=9 \(1\.\.8 built\)"),
                                        (dict(T=3, null_pass=2), "null teacher logits in pass 2 of T=3"), (dict(N=0), "chap_teacher_uncertainty: N=0, P=320"),
                                        (dict(N=1 << 16, P=1 << 16), "exceeds the 32-bit pixel index"), (dict(mask=0), "null mask, count or ws"),
                                        (dict(count=0), "null mask, count or ws"), (dict(ws=0), "null mask, count or ws"),
                                        (dict(odd=1), "4-byte aligned"), (dict(entropy=0xa0002), "4-byte aligned"), (dict(count=0x80004), "8-byte aligned")])
def test_uncertainty_argument_checks_refuse_by_value(over, match):
    from chap_amd import _lib
    with pytest.raises(_lib.ChapError, match=match):
        _lib.call("chap_teacher_uncertainty", _uparams(**over), 0)


def _mparams(**over):
    from chap_amd import _lib
    q = _lib.TeacherConsistencyMaskedParams()
    v = dict(l0=0x10000, l1=0x20000, t0=0x30000, t1=0x40000, d0=0x50000, d1=0x60000, loss=0x70000, ws=0x80000, mask=0x90000, count=0xa0000, N=4, C=4, P=320)
    v.update(over)
    q.logits[0], q.logits[1], q.teacher[0], q.teacher[1], q.dlogits[0], q.dlogits[1] = v["l0"], v["l1"], v["t0"], v["t1"], v["d0"], v["d1"]
    q.mask, q.count, q.loss, q.ws, q.gscale, q.N, q.C, q.P = v["mask"], v["count"], v["loss"], v["ws"], 1.0, v["N"], v["C"], v["P"]
    return q


@pytest.mark.parametrize("over,match", [(dict(C=9), r"chap_teacher_consistency_masked: C=9 \(2\.\.8 built\)"), (dict(C=1), r"C=1 \(2\.\.8 built\)"),
                                        (dict(N=0), "chap_teacher_consistency_masked: N=0, P=320"), (dict(P=0), "N=4, P=0"),
                                        (dict(N=1 << 16, P=1 << 16), "exceeds the 32-bit pixel index"), (dict(l1=0), "chap_teacher_consistency_masked: null"),
                                        (dict(mask=0), "chap_teacher_consistency_masked: null"), (dict(count=0), "chap_teacher_consistency_masked: null"),
                                        (dict(loss=0), "chap_teacher_consistency_masked: null"), (dict(d0=0x50002), "4-byte aligned"),
                                        (dict(count=0xa0004), "8-byte aligned")])
def test_masked_argument_checks_refuse_by_value(over, match):
    from chap_amd import _lib
    with pytest.raises(_lib.ChapError, match=match):
        _lib.call("chap_teacher_consistency_masked", _mparams(**over), 0)


def test_defaults_are_off():
    from chap_amd import train, train_ours_2D, train_ours_3D
    for d in (train.DEFAULT_ARGS, train_ours_2D.FLAG_DEFAULTS, train_ours_3D.FLAG_DEFAULTS):
        assert d["teacher_uncertainty"] == 0 and tuple(d["uncertainty_threshold"]) == (0.75, 1.0)
    assert train.check_teacher_uncertainty({}) == 0
    assert train.check_teacher_uncertainty({"teacher_uncertainty": 0, "uncertainty_threshold": "never read"}) == 0
    assert train.check_teacher_uncertainty({"teacher_uncertainty": 4, "teacher_consistency": 0.5}) == 4


ON = dict(teacher_consistency=0.5, mean_teacher=True)


@pytest.mark.parametrize("args,match", [(dict(ON, teacher_uncertainty=9), "teacher_uncertainty=9"), (dict(ON, teacher_uncertainty=-1), "teacher_uncertainty=-1"),
                                        (dict(ON, teacher_uncertainty=1.5), "teacher_uncertainty=1.5"), (dict(ON, teacher_uncertainty=True), "teacher_uncertainty=True"),
                                        (dict(mean_teacher=True, teacher_uncertainty=2), "teacher_uncertainty=2 needs teacher_consistency > 0"),
                                        (dict(ON, teacher_uncertainty=2, uncertainty_threshold=(0.0, 1.0)), "uncertainty_threshold"),
                                        (dict(ON, teacher_uncertainty=2, uncertainty_threshold=(0.9, 0.8)), "uncertainty_threshold"),
                                        (dict(ON, teacher_uncertainty=2, uncertainty_threshold=(0.5, float("inf"))), "uncertainty_threshold"),
                                        (dict(ON, teacher_uncertainty=2, uncertainty_threshold=0.75), "uncertainty_threshold"),
                                        (dict(ON, teacher_uncertainty=2, uncertainty_threshold=(0.5, 0.6, 0.7)), "uncertainty_threshold")])
def test_check_refuses_by_value_everywhere_before_anything_is_written(tmp_path, args, match):
    import importlib
    from chap_amd import train
    step_args = {k: v for k, v in args.items() if k != "mean_teacher"}
    with pytest.raises(ValueError, match=match):
        train.check_teacher_uncertainty(step_args, "x")
    with pytest.raises(ValueError, match="ChapStep: .*" + match):
        train.ChapStep(object(), step_args, teacher=object())            # raised ahead of the first use of the model or the teacher
    for entry in ("train_ours_2D", "train_ours_3D"):
        T = importlib.import_module("chap_amd." + entry)
        run = tmp_path / entry
        with pytest.raises(ValueError, match=entry + ": .*" + match):
            T.train(dict(args, max_iterations=2), str(run))
        assert not run.exists()
    assert os.listdir(tmp_path) == []


def test_steps_refuse_it_without_the_teacher_and_the_ablation_step_always():
    from chap_amd import train
    with pytest.raises(ValueError, match="ChapStep: teacher_consistency=0.5 needs the mean teacher"):
        train.ChapStep(object(), {"teacher_consistency": 0.5, "teacher_uncertainty": 2})
    with pytest.raises(ValueError, match="AblationStep: teacher_uncertainty=2"):
        train.AblationStep(object(), {"teacher_uncertainty": 2})
    with pytest.raises(ValueError, match="AblationStep: teacher_consistency=0.5"):
        train.AblationStep(object(), {"teacher_consistency": 0.5, "teacher_uncertainty": 2}, teacher=object())


def test_threshold_schedule_against_hand_worked_values():
    """C = 2, (lo, hi) = (0.75, 1.0), max_iterations = 1000: ramp = exp(-5 (1 - t)^2) is exp(-5) at 0, exp(-1.25) at the middle, 1 at the end."""
    from chap_amd import train
    a = dict(num_classes=2, max_iterations=1000, uncertainty_threshold=(0.75, 1.0))
    ln2 = 0.6931471805599453
    assert abs(train.uncertainty_threshold(0, a) - (0.75 + 0.25 * 0.006737946999085467) * ln2) < 1e-15          # 0.521027...
    assert abs(train.uncertainty_threshold(500, a) - (0.75 + 0.25 * 0.2865047968601901) * ln2) < 1e-15          # 0.569507...
    assert train.uncertainty_threshold(1000, a) == ln2 == train.uncertainty_threshold(5000, a)
    assert abs(train.uncertainty_threshold(0, a) - 0.5210279) < 1e-6 and abs(train.uncertainty_threshold(500, a) - 0.5695073) < 1e-6
    b = dict(num_classes=4, max_iterations=1000, uncertainty_threshold=(0.5, 0.5))
    assert all(abs(train.uncertainty_threshold(i, b) - 0.5 * math.log(4)) < 1e-15 for i in (0, 500, 1000))
