"""Host side of the mean teacher's consistency term (no GPU): the fp64 restatement tests/teacher_ref.py against autograd, its error bound against
an fp32 emulation of the kernel and against four planted faults, the header include/chap_hip_teacher.h against the binding, the entry's argument
checks (which return before anything is launched) and the argument checks of ChapStep, AblationStep and both train() entries."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import kernel_ref as kr
from tests import teacher_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chap_hip_teacher.h")


@pytest.mark.parametrize("C", [2, 3, 8])
def test_restatement_is_the_gradient_of_the_softmax_mse(C):
    """teacher_ref against fp64 autograd of ((softmax(s) - q)**2).mean() summed over the heads, q = the mean of the teacher's two softmax outputs."""
    x = tr.inputs(C, tr.SCALAR)
    s = [t.double().requires_grad_(True) for t in x["s"]]
    q = 0.5 * (torch.softmax(x["t"][0].double(), 1) + torch.softmax(x["t"][1].double(), 1))
    loss = sum(((torch.softmax(t, 1) - q) ** 2).mean() for t in s)
    loss.backward()
    loss = loss.detach()
    r = tr.teacher_ref(x["s"], x["t"])
    assert abs(float(r["loss"]) - float(loss)) <= 1e-13 * float(loss) and float(loss) > 0.1          # saturated softmaxes that disagree: a loss of order 1
    assert abs(float(r["head"][0] + r["head"][1]) - float(loss)) <= 1e-13 * float(loss)
    for h in range(2):
        assert (r["g"][h] - s[h].grad).abs().max() <= 1e-15
        assert s[h].grad.abs().max() > 1e-6
    # gscale, the device word and a prior enter linearly
    prior = (torch.randn_like(x["s"][0]), None)
    r2 = tr.teacher_ref(x["s"], x["t"], gscale=0.25, gscale_dev=3.0, prior=prior)
    assert (r2["g"][0] - (prior[0].double() + 0.75 * s[0].grad)).abs().max() <= 1e-15
    assert (r2["g"][1] - 0.75 * s[1].grad).abs().max() <= 1e-15 and r2["loss"] == r["loss"]


@pytest.mark.parametrize("shape", [tr.SCALAR, tr.QUADS], ids=["17x19", "16x20"])
@pytest.mark.parametrize("C", tr.CLASSES)
def test_fp32_emulation_is_inside_the_bound_and_every_planted_fault_is_outside(C, shape):
    """The bound is not loose enough to hide a wrong formula: the kernel's arithmetic in fp32 passes it, with and without a prior to accumulate
    onto, and each of the four faults fails it (in the gradient; the two that change the loss value fail there as well).  No comparison here
    rests on an absolute floor: every term of the bound is relative to the element's own quantities."""
    x = tr.inputs(C, shape)
    g = torch.Generator().manual_seed(9)
    prior = tuple(0.01 * torch.randn(x["s"][0].shape, generator=g) for _ in range(2))
    for pr, gs, gd in (((None, None), 1.0, None), (prior, 0.3, 0.7)):
        r = tr.teacher_ref(x["s"], x["t"], gscale=gs, gscale_dev=gd, prior=pr)
        loss, gg = tr.emulate_f32(x["s"], x["t"], gscale=gs, gscale_dev=gd, prior=pr)
        assert kr.check("loss", loss, r["loss"], r["loss_b"], "i") <= 1.0
        for h in range(2):
            assert kr.check("g%d" % h, gg[h], r["g"][h], r["g_b"][h]) <= 1.0
        for fault in tr.FAULTS:
            loss_f, gf = tr.emulate_f32(x["s"], x["t"], gscale=gs, gscale_dev=gd, prior=pr, fault=fault)
            for h in range(2):
                with pytest.raises(AssertionError, match="worst element"):
                    kr.check("g%d %s" % (h, fault), gf[h], r["g"][h], r["g_b"][h])
            if fault in ("div_np", "one_head"):
                with pytest.raises(AssertionError, match="worst element"):
                    kr.check("loss " + fault, loss_f, r["loss"], r["loss_b"], "i")


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const char\*)\s+(chap_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_and_abi_is_still_9():
    from chap_amd import _lib
    src = open(HEADER).read()
    assert re.search(r"\bint\s+chap_teacher_consistency\s*\(\s*const\s+chap_teacher_consistency_params\s*\*\s*p\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r'^#include "chap_hip\.h"$', src, flags=re.M)
    assert re.search(r"#define\s+CHAP_ABI_VERSION\s+9\b", open(os.path.join(ROOT, "include", "chap_hip.h")).read())
    assert _declared(HEADER) == sorted(_lib._TEACHER_SIGS) == ["chap_teacher_consistency"]
    others = set(_lib._SIGS) | set(_lib._SIGS_EXT) | set(_lib._SIGS_MONITOR) | set(_lib._SIGS_GUARD) | set(_lib._OPTIM_SIGS) | set(_lib._SIZE_FNS)
    assert not set(_lib._TEACHER_SIGS) & others
    assert not [n for n in vars(_lib) if n.startswith("_SIGS") and getattr(_lib, n) is _lib._TEACHER_SIGS]       # out of the access table's walk, as _OPTIM_SIGS
    assert _lib._TEACHER_SIGS["chap_teacher_consistency"] is _lib.TeacherConsistencyParams
    lib = _lib.lib()
    assert hasattr(lib, "chap_teacher_consistency") and lib.chap_abi_version() == _lib.ABI_VERSION == 9
    fn = _lib._fn("chap_teacher_consistency")
    assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(_lib.TeacherConsistencyParams)


def test_ctypes_struct_matches_header(tmp_path):
    from chap_amd import _lib
    st = _lib.TeacherConsistencyParams
    fields = [f[0] for f in st._fields_]
    c = tmp_path / "sz.c"
    body = 'printf("size %zu\\n", sizeof(chap_teacher_consistency_params));\n'
    body += "".join('printf("%s %%zu\\n", offsetof(chap_teacher_consistency_params, %s));\n' % (f, f) for f in fields)
    body += 'printf("slots %d\\n", CHAP_LOSS_SLOTS);\n'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip_teacher.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got["size"]) == ctypes.sizeof(st)
    for f in fields:
        assert int(got[f]) == getattr(st, f).offset, f
    from chap_amd import ops
    assert int(got["slots"]) == _lib.LOSS_SLOTS and ops.teacher_consistency_ws_words() == (1 + _lib.LOSS_SLOTS) * 2


def _params(**over):
    """Made-up, aligned, non-null addresses: every check below fails before a launch, nothing is dereferenced."""
    from chap_amd import _lib
    q = _lib.TeacherConsistencyParams()
    v = dict(l0=0x10000, l1=0x20000, t0=0x30000, t1=0x40000, d0=0x50000, d1=0x60000, loss=0x70000, ws=0x80000, N=4, C=4, P=320)
    v.update(over)
    q.logits[0], q.logits[1], q.teacher[0], q.teacher[1], q.dlogits[0], q.dlogits[1] = v["l0"], v["l1"], v["t0"], v["t1"], v["d0"], v["d1"]
    q.loss, q.ws, q.gscale, q.N, q.C, q.P = v["loss"], v["ws"], 1.0, v["N"], v["C"], v["P"]
    return q


@pytest.mark.parametrize("over,match", [(dict(C=9), r"chap_teacher_consistency: C=9 \(2\.\.8 built\)"), (dict(C=1), r"chap_teacher_consistency: C=1 \(2\.\.8 built\)"),
                                        (dict(N=0), "chap_teacher_consistency: N=0, P=320"), (dict(P=0), "chap_teacher_consistency: N=4, P=0"),
                                        (dict(N=-1), "chap_teacher_consistency: N=-1"), (dict(N=1 << 16, P=1 << 16), "exceeds the 32-bit pixel index"),
                                        (dict(l1=0), "chap_teacher_consistency: null"), (dict(t0=0), "chap_teacher_consistency: null"),
                                        (dict(loss=0), "chap_teacher_consistency: null"), (dict(ws=0), "chap_teacher_consistency: null"),
                                        (dict(d0=0x50002), "4-byte aligned")])
def test_argument_checks_refuse_by_name(over, match):
    from chap_amd import _lib
    with pytest.raises(_lib.ChapError, match=match):
        _lib.call("chap_teacher_consistency", _params(**over), 0)


def test_defaults_are_off():
    from chap_amd import train, train_ours_2D, train_ours_3D
    for d in (train.DEFAULT_ARGS, train_ours_2D.FLAG_DEFAULTS, train_ours_3D.FLAG_DEFAULTS):
        assert d["teacher_consistency"] == 0.0 and d["teacher_noise"] == 0.1
    assert train.check_teacher_consistency({}, False) == 0.0 and train.check_teacher_consistency({"teacher_consistency": 0.5}, True) == 0.5


@pytest.mark.parametrize("entry", ["train_ours_2D", "train_ours_3D"])
def test_train_refuses_the_term_without_a_teacher_before_it_writes(tmp_path, entry):
    import importlib
    T = importlib.import_module("chap_amd." + entry)
    run = tmp_path / "run"
    with pytest.raises(ValueError, match="teacher_consistency=0.5 needs the mean teacher"):
        T.train(dict(teacher_consistency=0.5, max_iterations=2), str(run))
    with pytest.raises(ValueError, match="teacher_noise"):
        T.train(dict(teacher_consistency=0.5, mean_teacher=True, teacher_noise=-1.0, max_iterations=2), str(run))
    with pytest.raises(ValueError, match="teacher_consistency"):
        T.train(dict(teacher_consistency=-0.5, mean_teacher=True, max_iterations=2), str(run))
    assert not run.exists() and os.listdir(tmp_path) == []


def test_steps_refuse_the_term_without_a_teacher_before_they_allocate():
    """Raised ahead of the first use of the model: an object() in its place is never touched."""
    from chap_amd import train
    with pytest.raises(ValueError, match="ChapStep: teacher_consistency=0.5 needs the mean teacher"):
        train.ChapStep(object(), {"teacher_consistency": 0.5})
    with pytest.raises(ValueError, match="AblationStep: teacher_consistency=0.5"):
        train.AblationStep(object(), {"teacher_consistency": 0.5})
    with pytest.raises(ValueError, match="AblationStep: teacher_consistency=0.5"):
        train.AblationStep(object(), {"teacher_consistency": 0.5}, teacher=object())
