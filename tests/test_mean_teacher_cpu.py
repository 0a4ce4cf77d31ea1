"""Host side of the mean teacher (no GPU): the chap_sgd_ema_step entry in the header (include/chap_hip_ext.h, through chap_hip.h), the binding and the argument checks (which return
before anything is launched), the schedule of the averaging coefficient, and that with the feature off neither train() entry nor the
optimizer touches any of it."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import ema_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chap_hip.h")


EXT_HEADER = os.path.join(ROOT, "include", "chap_hip_ext.h")


def _declared(path):
    """tests/test_abi_cpu.py::_declared_functions on another header."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const char\*)\s+(chap_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_entry_and_abi_is_still_9():
    """The entry is declared in include/chap_hip_ext.h, the fragment include/chap_hip.h ends on (a C file that includes chap_hip.h alone sees it:
    the sizeof probe below), and bound in _lib._SIGS_EXT.  The tables of the default iteration's entry points (_lib._SIGS, which the access
    table tests/launch_access.py classifies entry by entry) are the parent's: the extension is held to the same header <-> binding equality here."""
    from chap_amd import _lib
    src, ext = open(HEADER).read(), open(EXT_HEADER).read()
    assert re.search(r'^#include "chap_hip_ext\.h"$', src, flags=re.M) and src.index('#include "chap_hip_ext.h"') > src.index("int chap_abi_version(void);")
    assert re.search(r"\bint\s+chap_sgd_ema_step\s*\(\s*const\s+chap_sgd_ema_params\s*\*\s*p\s*,\s*void\s*\*\s*stream\s*\)\s*;", ext)
    assert re.search(r"#define\s+CHAP_ABI_VERSION\s+9\b", src)
    assert "train_ours_2D.py:50-54" in ext
    assert _declared(EXT_HEADER) == sorted(_lib._SIGS_EXT) == ["chap_sgd_ema_step"]         # every declared extension entry is bound and vice versa
    assert not set(_lib._SIGS_EXT) & (set(_lib._SIGS) | set(_lib._SIZE_FNS)) and not set(_declared(EXT_HEADER)) & set(_declared(HEADER))
    assert _lib._SIGS_EXT["chap_sgd_ema_step"] is _lib.SgdEmaParams
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in _lib._SIGS_EXT) and lib.chap_abi_version() == _lib.ABI_VERSION == 9
    fn = _lib._fn("chap_sgd_ema_step")
    assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(_lib.SgdEmaParams)


def test_ctypes_struct_size_matches_header(tmp_path):
    from chap_amd import _lib
    pairs = {"chap_sgd_params": _lib.SgdParams, "chap_sgd_ema_params": _lib.SgdEmaParams}
    c = tmp_path / "sz.c"
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in pairs)
    body += 'printf("ema %zu\\ncoef %zu\\n", offsetof(chap_sgd_ema_params, ema), offsetof(chap_sgd_ema_params, coef));\n'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for name, st in pairs.items():
        assert int(sizes[name]) == ctypes.sizeof(st), (name, sizes[name], ctypes.sizeof(st))
    assert int(sizes["ema"]) == _lib.SgdEmaParams.ema.offset and int(sizes["coef"]) == _lib.SgdEmaParams.coef.offset
    assert _lib.SgdEmaParams.sgd.offset == 0                 # chap_sgd_params first: the update's own arguments are chap_sgd_step's


def _params(**over):
    """Made-up, aligned, non-null addresses: every check below fails before a launch, nothing is dereferenced."""
    from chap_amd import _lib
    q = _lib.SgdEmaParams()
    v = dict(param=0x10000, grad=0x20000, grad2=0, mom=0x30000, lr=0x40000, ema=0x50000, coef=0x60000, n=1000)
    v.update(over)
    q.sgd.param, q.sgd.grad, q.sgd.grad2, q.sgd.mom, q.sgd.lr, q.sgd.n = v["param"], v["grad"], v["grad2"], v["mom"], v["lr"], v["n"]
    q.sgd.momentum, q.sgd.weight_decay, q.sgd.grad_scale, q.sgd.zero_grad = 0.9, 1e-4, 1.0, 1
    q.ema, q.coef = v["ema"], v["coef"]
    return q


@pytest.mark.parametrize("over,match", [(dict(ema=0), "chap_sgd_ema_step: null ema"), (dict(coef=0), "chap_sgd_ema_step: null coef"),
                                        (dict(ema=0x50004), "chap_sgd_ema_step: buffers must be 16-byte aligned"),
                                        (dict(param=0), "chap_sgd_ema_step: bad argument"), (dict(n=0), "chap_sgd_ema_step: bad argument"),
                                        (dict(mom=0x30008), "chap_sgd_ema_step: buffers must be 16-byte aligned")])
def test_argument_checks_refuse_by_name(over, match):
    from chap_amd import _lib
    with pytest.raises(_lib.ChapError, match=match):
        _lib.call("chap_sgd_ema_step", _params(**over), 0)


def test_ema_alpha_is_the_reference_expression():
    from chap_amd.train import ema_alpha, ema_coefficients
    for d in (0.9, 0.99, 0.999):
        for s in range(201):
            assert ema_alpha(s, d) == min(1 - 1 / (s + 1), d) == ema_ref.alpha_of(s, d)        # update_ema_variables' line, in double
            a, b = ema_coefficients(s, d)
            al = min(1 - 1 / (s + 1), d)
            assert a == float(torch.tensor(al, dtype=torch.float64).float()) and b == float(torch.tensor(1 - al, dtype=torch.float64).float())
            assert (a, b) == ema_ref.coefficients(s, d)
        assert ema_alpha(0, d) == 0.0 and ema_coefficients(0, d) == (0.0, 1.0)
    for d, first in ((0.9, 9), (0.99, 99), (0.999, 999)):            # constant from s >= 1 / (1 - d) - 1
        assert all(ema_alpha(s, d) == d for s in range(first, first + 300))
        assert all(ema_alpha(s, d) < d for s in range(first - 1))
        assert all(ema_alpha(s, d) < ema_alpha(s + 1, d) for s in range(first - 1))


class _FakeModel:
    def __init__(self, n=12):
        self.flat, self.grad, self.dirty = torch.zeros(n), torch.zeros(n), 0

    def flat_buffers(self):
        return self.flat, self.grad

    def mark_params_dirty(self):
        self.dirty += 1


def test_fused_sgd_issues_the_plain_entry_without_ema(monkeypatch):
    from chap_amd import train
    calls = []
    monkeypatch.setattr(train.ops, "sgd_step", lambda *a, **k: calls.append(("sgd_step", a)))
    monkeypatch.setattr(train.ops, "sgd_ema_step", lambda *a, **k: calls.append(("sgd_ema_step", a)))
    m = _FakeModel()
    opt = train.FusedSGD(m, 0.01)
    assert opt.ema is None and opt.ema_coef is None and opt.ema_decay == 0.99
    opt.step(grad_scale=0.5, grad2=None)
    assert [c[0] for c in calls] == ["sgd_step"] and m.dirty == 1
    assert calls[0][1][0] is m.flat and calls[0][1][2] is opt.mom and calls[0][1][6] == 0.5
    # ... and the new entry with one, reading (a, b) from the optimizer's device words
    t = _FakeModel()
    ema = torch.ones(12)
    opt2 = train.FusedSGD(m, 0.01, ema=ema, ema_decay=0.9)
    opt2.ema_model = t
    opt2.set_ema_step(1)
    assert opt2.ema_coef.tolist() == [0.5, 0.5]
    opt2.set_ema_step(50)
    assert opt2.ema_coef.tolist() == list(ema_ref.coefficients(50, 0.9)) and abs(opt2.ema_coef[0].item() - 0.9) < 1e-7
    opt2.step()
    assert [c[0] for c in calls] == ["sgd_step", "sgd_ema_step"] and t.dirty == 1 and m.dirty == 2
    assert calls[1][1][6] is ema and calls[1][1][7] is opt2.ema_coef
    with pytest.raises(ValueError, match="flat parameter buffer"):
        train.FusedSGD(m, 0.01, ema=torch.ones(11))


class _FakeStep:
    """ChapStep as the entries build it with the feature off: (model, args), no teacher argument."""
    def __init__(self, model, a):
        self.iter_num = 0

    def step(self, v, l):
        self.iter_num += 1
        return {"mix_losses": [torch.zeros(3)], "vat_loss": torch.zeros(1)}


class _FakeNet(torch.nn.Module):
    def set_compute_dtype(self, d):
        return self


def _no_teacher(*a, **k):
    raise AssertionError("build_teacher called with mean_teacher off")


@pytest.mark.parametrize("flags", [dict(mean_teacher=False), dict()], ids=["off", "default"])
def test_train_2d_without_the_flag_builds_no_teacher(tmp_path, monkeypatch, flags):
    from chap_amd import train_ours_2D as T
    assert T.FLAG_DEFAULTS["mean_teacher"] is False and T.FLAG_DEFAULTS["ema_decay"] == 0.99
    monkeypatch.setattr(T, "ChapStep", _FakeStep)
    monkeypatch.setattr(T, "build_teacher", _no_teacher)
    monkeypatch.setattr(T, "net_factory", lambda **kw: _FakeNet())
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch, "device", lambda *a, **k: "cpu")
    loader = [{"image": torch.zeros(2, 1, 4, 4), "label": torch.zeros(2, 4, 4, dtype=torch.int64)}]
    T.train(dict(flags, trainloader=loader, val_volumes=[], max_iterations=3, val_interval=1000, use_graph=False, image_size=[4, 4]), str(tmp_path / "run"))
    assert sorted(os.listdir(tmp_path / "run")) == ["log.txt"]


@pytest.mark.parametrize("flags", [dict(mean_teacher=False), dict()], ids=["off", "default"])
def test_train_3d_without_the_flag_builds_no_teacher(tmp_path, monkeypatch, flags):
    from chap_amd import train_ours_3D as T
    assert T.FLAG_DEFAULTS["mean_teacher"] is False and T.FLAG_DEFAULTS["ema_decay"] == 0.99
    monkeypatch.setattr(T, "ChapStep", _FakeStep)
    monkeypatch.setattr(T, "build_teacher", _no_teacher)
    monkeypatch.setattr(T, "net_factory_3d", lambda **kw: _FakeNet())
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch, "device", lambda *a, **k: "cpu")
    loader = [{"image": torch.zeros(2, 1, 4, 4, 4), "label": torch.zeros(2, 4, 4, 4, dtype=torch.int64)}]
    T.train(dict(flags, trainloader=loader, val_volumes=[], max_iterations=3, val_interval=1000, use_graph=False, patch_size=[4, 4, 4]), str(tmp_path / "run"))
    assert sorted(os.listdir(tmp_path / "run")) == ["log.txt"]
