"""Host side of the gradient guard (no GPU): the fp64 restatement (tests/guard_ref.py) against torch.nn.utils.clip_grad_norm_, the header
include/chap_hip_guard.h against the binding table _lib._SIGS_GUARD, the struct sizes, the argument checks of the two entries (which return
before anything is launched), StepGuard's argument errors and ring bookkeeping, guard.csv / log formatting from hand-made rows, what
FusedSGD.step issues with a guard, and the checkpoint gate of both train() entries with a stubbed step."""
import ctypes
import logging
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import guard_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chap_hip.h")
GUARD_HEADER = os.path.join(ROOT, "include", "chap_hip_guard.h")
ENTRIES = ["chap_grad_norm", "chap_sgd_guard_step"]


def _declared(path):
    """tests/test_abi_cpu.py::_declared_functions on another header."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const char\*)\s+(chap_[a-z0-9_]+)\s*\(", src)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e30])
def test_restatement_is_clip_grad_norm(max_norm):
    """Torch takes its norm in fp32 and multiplies every gradient by its fp32 coefficient: the clipped gradients agree at rtol 1e-6."""
    g = torch.Generator().manual_seed(11)
    shapes = [(16, 1, 3, 3), (16,), (32, 16, 3, 3), (7,)]
    grads = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    flat = torch.cat([t.reshape(-1) for t in grads])
    r = gr.guard_ref(flat, None, 1.0, max_norm)
    total, clipped = gr.clip_like_torch(grads, max_norm)
    assert abs(r["norm64"] - total) <= 1e-6 * total and r["skip"] == 0 and not r["nonfinite"]
    want = torch.cat([t.reshape(-1) for t in clipped])
    assert torch.allclose(flat * r["coef"], want, rtol=1e-6, atol=0)
    assert (r["coef"] < 1.0) == (total > max_norm)
    # two buckets and a scale: the norm of (g + g2) * grad_scale
    a, b = flat * 0.25, flat * 0.75
    r2 = gr.guard_ref(a, b, 0.5, max_norm)
    assert abs(r2["norm64"] - 0.5 * r["norm64"]) <= 1e-6 * r["norm64"]


def test_restatement_exact_and_nonfinite_cases():
    z = torch.zeros(9)
    g = z.clone(); g[1], g[7] = 3.0, 4.0
    r = gr.guard_ref(g, None, 1.0, 2.5)
    assert r["norm64"] == 5.0 and r["coef"] == gr.fl32(2.5 / (5.0 + 1e-6)) and r["skip"] == 0
    a, b = z.clone(), z.clone(); a[1], b[7] = 3.0, -4.0
    assert gr.guard_ref(a, b, 2.0, 0.0)["norm64"] == 10.0 and gr.guard_ref(a, b, 2.0, 0.0)["coef"] == 1.0
    for bad in (float("nan"), float("inf"), -float("inf")):
        g = torch.ones(9); g[8] = bad
        r = gr.guard_ref(g, None, 1.0, 1.0, True)
        assert (r["skip"], r["coef"], r["nonfinite"]) == (1, 0.0, True) and not np.isfinite(r["norm"])
        r = gr.guard_ref(g, None, 1.0, 0.0, False)
        assert (r["skip"], r["coef"], r["nonfinite"]) == (0, 1.0, True)
    a, b = torch.ones(5), torch.ones(5)
    a[2], b[2] = float("inf"), -float("inf")            # h = NaN
    assert gr.guard_ref(a, b)["skip"] == 1
    a[2], b[2] = 3e38, 3e38                             # h overflows in fp32: what the optimizer would see
    assert gr.guard_ref(a, b)["skip"] == 1 and gr.guard_ref(a, None)["skip"] == 0


# ---- header, binding, structs ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_abi_is_still_9():
    from chap_amd import _lib
    src = open(GUARD_HEADER).read()
    assert re.search(r"#define\s+CHAP_ABI_VERSION\s+9\b", open(HEADER).read())
    assert re.search(r"#define\s+CHAP_GRADNORM_SLOTS\s+512\b", src) and _lib.GRADNORM_SLOTS == 512
    assert _declared(GUARD_HEADER) == sorted(_lib._SIGS_GUARD) == ENTRIES                 # every declared entry is bound and vice versa
    others = set(_lib._SIGS) | set(_lib._SIGS_EXT) | set(_lib._SIGS_MONITOR) | set(_lib._SIZE_FNS)
    assert not set(_lib._SIGS_GUARD) & others and not set(ENTRIES) & set(_declared(HEADER))
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in ENTRIES) and lib.chap_abi_version() == _lib.ABI_VERSION == 9
    for n in ENTRIES:
        fn = _lib._fn(n)
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(_lib._SIGS_GUARD[n])


def test_ctypes_struct_sizes_match_header(tmp_path):
    from chap_amd import _lib, guard, ops
    pairs = {"chap_guard_state": _lib.GuardState, "chap_guard_row": _lib.GuardRow, "chap_grad_norm_params": _lib.GradNormParams,
             "chap_sgd_guard_params": _lib.SgdGuardParams}
    offs = [("chap_guard_state", f, _lib.GuardState) for f in ("scale", "skip", "norm", "steps", "skipped_total", "clipped_total")] + \
           [("chap_guard_row", f, _lib.GuardRow) for f in ("step", "norm", "coef", "skip")] + \
           [("chap_grad_norm_params", f, _lib.GradNormParams) for f in ("grad2", "n", "grad_scale", "max_norm", "skip_nonfinite", "ring", "ws", "state")] + \
           [("chap_sgd_guard_params", "state", _lib.SgdGuardParams)]
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in pairs)
    body += "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (s, f, s, f) for s, f, _ in offs)
    body += 'printf("bytes7 %zu\\n", (size_t)CHAP_GUARD_STATE_BYTES(7));\n'
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip_guard.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for name, st in pairs.items():
        assert int(sizes[name]) == ctypes.sizeof(st), (name, sizes[name], ctypes.sizeof(st))
    for s, f, st in offs:
        assert int(sizes["%s.%s" % (s, f)]) == getattr(st, f).offset, (s, f)
    assert _lib.SgdGuardParams.se.offset == 0
    assert int(sizes["bytes7"]) == 4 * ops.guard_state_words(7) == 4 * (guard.HDR_WORDS + 7 * guard.ROW_WORDS)
    assert ctypes.sizeof(_lib.GuardState) % 16 == 0 and ctypes.sizeof(_lib.GuardRow) == 16       # rows are 16-byte aligned behind the header


def _norm_params(**over):
    """Made-up, aligned, non-null addresses: every check below fails before a launch, nothing is dereferenced."""
    from chap_amd import _lib
    p = _lib.GradNormParams()
    v = dict(grad=0x10000, grad2=0, n=1000, ring=4, ws=0x20000, state=0x30000)
    v.update(over)
    p.grad, p.grad2, p.n, p.ring, p.ws, p.state = v["grad"], v["grad2"], v["n"], v["ring"], v["ws"], v["state"]
    p.grad_scale, p.max_norm, p.skip_nonfinite = 1.0, 1.0, 1
    return p


def _step_params(**over):
    from chap_amd import _lib
    q = _lib.SgdGuardParams()
    v = dict(param=0x10000, grad=0x20000, grad2=0, mom=0x30000, lr=0x40000, ema=0, coef=0, n=1000, state=0x70000)
    v.update(over)
    s = q.se.sgd
    s.param, s.grad, s.grad2, s.mom, s.lr, s.n = v["param"], v["grad"], v["grad2"], v["mom"], v["lr"], v["n"]
    s.momentum, s.weight_decay, s.grad_scale, s.zero_grad = 0.9, 1e-4, 1.0, 1
    q.se.ema, q.se.coef, q.state = v["ema"], v["coef"], v["state"]
    return q


@pytest.mark.parametrize("name,params,match", [
    ("chap_grad_norm", _norm_params(grad=0), "chap_grad_norm: bad argument"),
    ("chap_grad_norm", _norm_params(ws=0), "chap_grad_norm: bad argument"),
    ("chap_grad_norm", _norm_params(state=0), "chap_grad_norm: bad argument"),
    ("chap_grad_norm", _norm_params(n=0), "chap_grad_norm: bad argument"),
    ("chap_grad_norm", _norm_params(ring=0), "chap_grad_norm: ring=0"),
    ("chap_grad_norm", _norm_params(grad2=0x50004), "chap_grad_norm: grad, grad2 and state must be 16-byte"),
    ("chap_grad_norm", _norm_params(state=0x30008), "chap_grad_norm: grad, grad2 and state must be 16-byte"),
    ("chap_grad_norm", _norm_params(ws=0x20004), "ws 8-byte aligned"),
    ("chap_sgd_guard_step", _step_params(param=0), "chap_sgd_guard_step: bad argument"),
    ("chap_sgd_guard_step", _step_params(n=0), "chap_sgd_guard_step: bad argument"),
    ("chap_sgd_guard_step", _step_params(state=0), "chap_sgd_guard_step: null state"),
    ("chap_sgd_guard_step", _step_params(ema=0x50000), "chap_sgd_guard_step: null coef"),
    ("chap_sgd_guard_step", _step_params(ema=0x50004, coef=0x60000), "chap_sgd_guard_step: buffers must be 16-byte aligned"),
    ("chap_sgd_guard_step", _step_params(mom=0x30008), "chap_sgd_guard_step: buffers must be 16-byte aligned"),
    ("chap_sgd_guard_step", _step_params(state=0x70004), "chap_sgd_guard_step: buffers must be 16-byte aligned"),
])
def test_argument_checks_refuse_by_name(name, params, match):
    from chap_amd import _lib
    with pytest.raises(_lib.ChapError, match=match):
        _lib.call(name, params, 0)


# ---- StepGuard -------------------------------------------------------------------------------------------------------------------------
def test_step_guard_argument_errors():
    from chap_amd.guard import StepGuard
    with pytest.raises(ValueError, match="max_norm"):
        StepGuard(max_norm=-1.0, device="cpu")
    with pytest.raises(ValueError, match="ring"):
        StepGuard(max_norm=1.0, ring=0, device="cpu")
    for mn in (None, 0, 0.0):
        with pytest.raises(ValueError, match="neither"):
            StepGuard(max_norm=mn, skip_nonfinite=False, device="cpu")
    g = StepGuard(device="cpu")                         # the default: skip non-finite steps, no clipping
    assert (g.max_norm, g.skip_nonfinite, g.R, g.ws) == (0.0, True, 256, None)
    g = StepGuard(max_norm=2, skip_nonfinite=False, ring=3, device="cpu")
    assert (g.max_norm, g.skip_nonfinite, g.R) == (2.0, False, 3) and g.state.numel() == 8 + 4 * 3 and g.state.dtype == torch.int32


def _write_step(guard, norm, coef, skip):
    """What chap_grad_norm's totals kernel does to the state block, on a host-only guard."""
    from chap_amd.guard import HDR_WORDS, ROW_WORDS
    w = guard.state.numpy()
    bits = lambda v: int(np.float32(v).view(np.int32))
    steps = int(w[3])
    w[0], w[1], w[2], w[3] = bits(coef), skip, bits(norm), steps + 1
    w[4] += skip
    w[5] += int(not skip and coef < 1.0)
    o = HDR_WORDS + (steps % guard.R) * ROW_WORDS
    w[o:o + 4] = [steps + 1, bits(norm), bits(coef), skip]


def test_read_delivers_new_rows_in_order_and_counts_overwritten_ones():
    from chap_amd.guard import StepGuard
    g = StepGuard(max_norm=1.0, ring=4, device="cpu")
    r = g.read()
    assert len(r["step"]) == 0 and (r["steps"], r["skipped_total"], r["clipped_total"], r["dropped"]) == (0, 0, 0, 0)
    _write_step(g, 0.5, 1.0, 0); _write_step(g, 2.0, 0.5, 0); _write_step(g, float("inf"), 0.0, 1)
    r = g.read()
    assert r["step"].tolist() == [1, 2, 3] and r["coef"].tolist() == [1.0, 0.5, 0.0] and r["skip"].tolist() == [0, 0, 1]
    assert r["norm"][:2].tolist() == [0.5, 2.0] and np.isinf(r["norm"][2]) and r["norm"].dtype == np.float32
    assert (r["steps"], r["skipped_total"], r["clipped_total"], r["dropped"]) == (3, 1, 1, 0)
    assert len(g.read()["step"]) == 0                   # nothing new
    for k in range(6):                                  # steps 4..9 into a ring of 4: 4 and 5 are gone
        _write_step(g, float(k), 1.0, 0)
    r = g.read()
    assert r["step"].tolist() == [6, 7, 8, 9] and r["norm"].tolist() == [2.0, 3.0, 4.0, 5.0] and r["dropped"] == 2 and g.dropped == 2
    # the counters of a checkpoint: the rows before it are not in this ring
    st = g.state_dict()
    assert st == {"steps": 9, "skipped_total": 1, "clipped_total": 1}
    h = StepGuard(max_norm=1.0, ring=4, device="cpu").load_state_dict(st)
    assert h.state_dict() == st and len(h.read()["step"]) == 0 and h.dropped == 0
    _write_step(h, 7.0, 1.0, 0)
    assert h.read()["step"].tolist() == [10]
    # snapshot / restore (capture()'s warm-up): rows and counts go back, unread rows stay unread
    _write_step(g, 1.0, 1.0, 0)
    snap = g.snapshot()
    _write_step(g, 9.0, 0.1, 0); _write_step(g, 9.0, 0.1, 0)
    g.restore(snap)
    r = g.read()
    assert r["step"].tolist() == [10] and (r["steps"], r["clipped_total"]) == (10, 1)


def test_csv_and_log_lines_from_hand_made_rows(tmp_path):
    from chap_amd import guard as G
    rows = {"step": np.array([201, 202, 203, 204]), "norm": np.array([1.5, 4.0, np.inf, 0.25], dtype=np.float32),
            "coef": np.array([1.0, 0.5, 0.0, 1.0], dtype=np.float32), "skip": np.array([0, 0, 1, 0]), "steps": 204, "skipped_total": 1,
            "clipped_total": 1, "dropped": 0}
    assert G.CSV_HEADER == "iteration,grad_norm,coef,skipped"
    assert G.csv_lines(rows) == ["201,1.5,1,0", "202,4,0.5,0", "203,inf,0,1", "204,0.25,1,0"]
    assert G.summary_line(rows) == "guard : iterations 201-204 : max grad norm : 4.000000 median grad norm : 1.500000 clipped : 1 skipped : 1 of 4"
    seen = []
    log = logging.getLogger("test_guard_cpu")
    log.setLevel(logging.INFO)
    h = logging.Handler()
    h.emit = lambda rec: seen.append(rec.getMessage())
    log.addHandler(h)
    try:
        G.write_rows(rows, str(tmp_path), log)
        G.write_rows(dict(rows, step=np.array([205]), norm=np.array([2.0], dtype=np.float32), coef=np.array([1.0], dtype=np.float32), skip=np.array([0]), dropped=3),
                     str(tmp_path), log)
        G.write_rows(dict(rows, step=np.array([], dtype=np.int64), norm=np.array([], dtype=np.float32), coef=np.array([], dtype=np.float32),
                          skip=np.array([], dtype=np.int64)), str(tmp_path), log)
    finally:
        log.removeHandler(h)
    assert open(tmp_path / "guard.csv").read().splitlines() == [G.CSV_HEADER, "201,1.5,1,0", "202,4,0.5,0", "203,inf,0,1", "204,0.25,1,0", "205,2,1,0"]
    assert seen == [G.summary_line(rows), "guard : iteration 203 skipped : non-finite gradient (norm inf)",
                    "guard : 3 iterations were overwritten in the ring before they were read",
                    "guard : iterations 205-205 : max grad norm : 2.000000 median grad norm : 2.000000 clipped : 0 skipped : 0 of 1"]


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------------
class _FakeModel:
    def __init__(self, n=12):
        self.flat, self.grad, self.dirty = torch.zeros(n), torch.zeros(n), 0

    def flat_buffers(self):
        return self.flat, self.grad

    def mark_params_dirty(self):
        self.dirty += 1


class _FakeGuard:
    def __init__(self):
        self.ws, self.device, self.state, self.calls = torch.zeros(1, dtype=torch.float64), torch.device("cpu"), torch.zeros(12, dtype=torch.int32), []

    def launch_norm(self, grad, grad2, grad_scale):
        self.calls.append((grad, grad2, grad_scale))


def test_fused_sgd_issues_norm_then_the_guarded_entry(monkeypatch):
    from chap_amd import train
    calls = []
    for n in ("sgd_step", "sgd_ema_step", "sgd_guard_step"):
        monkeypatch.setattr(train.ops, n, lambda *a, _n=n, **k: calls.append((_n, a)))
    m, g = _FakeModel(), _FakeGuard()
    opt = train.FusedSGD(m, 0.01)
    assert opt.guard is None
    opt.step()
    assert [c[0] for c in calls] == ["sgd_step"] and g.calls == []           # without a guard: the parent's launch
    opt.set_guard(g)
    g2 = torch.ones(12)
    opt.step(grad_scale=0.5, grad2=g2)
    assert [c[0] for c in calls] == ["sgd_step", "sgd_guard_step"] and len(g.calls) == 1
    assert g.calls[0][0] is m.grad and g.calls[0][1] is g2 and g.calls[0][2] == 0.5
    a = calls[1][1]
    assert a[0] is m.flat and a[1] is m.grad and a[2] is opt.mom and a[6] is g.state and a[7] is None and a[9] == 0.5 and a[11] is g2
    # with a teacher: the same entry, handed the average and its coefficients
    t, ema = _FakeModel(), torch.ones(12)
    opt2 = train.FusedSGD(m, 0.01, ema=ema, guard=g)
    opt2.ema_model = t
    opt2.step()
    assert [c[0] for c in calls][2:] == ["sgd_guard_step"] and calls[2][1][7] is ema and calls[2][1][8] is opt2.ema_coef and t.dirty == 1
    opt2.set_guard(None)
    opt2.step()
    assert [c[0] for c in calls][3:] == ["sgd_ema_step"]
    host_only = _FakeGuard()
    host_only.ws = None
    with pytest.raises(ValueError, match="guard lives on"):
        train.FusedSGD(m, 0.01, guard=host_only)


# ---- train(): flags and the checkpoint gate ----------------------------------------------------------------------------------------------
class _FakeStep:
    """ChapStep as the entries build it with the feature off: (model, args), no guard argument."""
    def __init__(self, model, a):
        self.iter_num = 0

    def step(self, v, l):
        self.iter_num += 1
        return {"mix_losses": [torch.zeros(3)], "vat_loss": torch.zeros(1)}


class _FakeNet(torch.nn.Module):
    poison = False

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.ones(3))
        self.w = torch.nn.Parameter(torch.full((2, 2), float("nan")) if _FakeNet.poison else torch.ones(2, 2))
        self.register_buffer("count", torch.zeros((), dtype=torch.int64))

    def set_compute_dtype(self, d):
        return self


def _no_guard(*a, **k):
    raise AssertionError("StepGuard built with the flags off")


def _entry(dims, monkeypatch):
    if dims == 2:
        from chap_amd import train_ours_2D as T
        monkeypatch.setattr(T, "net_factory", lambda **kw: _FakeNet())
        monkeypatch.setattr(T, "test_single_volume", lambda *a, **k: [(0.5, 1.0)] * 3)
        size = dict(image_size=[4, 4])
        loader = [{"image": torch.zeros(2, 1, 4, 4), "label": torch.zeros(2, 4, 4, dtype=torch.int64)}]
    else:
        from chap_amd import train_ours_3D as T
        monkeypatch.setattr(T, "net_factory_3d", lambda **kw: _FakeNet())
        monkeypatch.setattr(T, "var_each_case", lambda model, cases, *a, **k: [0.5] * len(cases))
        size = dict(patch_size=[4, 4, 4])
        loader = [{"image": torch.zeros(2, 1, 4, 4, 4), "label": torch.zeros(2, 4, 4, 4, dtype=torch.int64)}]
    monkeypatch.setattr(T, "ChapStep", _FakeStep)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    return T, dict(size, trainloader=loader, val_volumes=[(None, None)], use_graph=False)


@pytest.mark.parametrize("dims", [2, 3])
def test_train_checkpoint_gate_refuses_a_nonfinite_model_and_keeps_the_files(tmp_path, monkeypatch, dims):
    T, common = _entry(dims, monkeypatch)
    assert T.FLAG_DEFAULTS["clip_grad_norm"] == 0.0 and T.FLAG_DEFAULTS["skip_nonfinite"] is False
    monkeypatch.setattr(T, "StepGuard", _no_guard)      # ... and with them off no guard is built: _FakeStep takes no such argument either
    run = str(tmp_path / "run")
    _FakeNet.poison = False
    T.train(dict(common, max_iterations=2, val_interval=2), run)
    files = ["dualdecoder_best_model.pth", "latest.pth"]
    assert sorted(f for f in os.listdir(run) if f.endswith(".pth")) == files and "guard.csv" not in os.listdir(run)
    before = {f: open(os.path.join(run, f), "rb").read() for f in files}
    _FakeNet.poison = True
    try:
        with pytest.raises(RuntimeError, match=r"iteration 2: the model holds a non-finite value in 'w'"):
            T.train(dict(common, max_iterations=4, val_interval=2), run)
    finally:
        _FakeNet.poison = False
    assert {f: open(os.path.join(run, f), "rb").read() for f in files} == before
    assert sorted(f for f in os.listdir(run) if f.endswith(".pth")) == files


def test_first_nonfinite_names_the_first_bad_tensor():
    from chap_amd.guard import check_finite_before_save, first_nonfinite
    sd = {"a": torch.ones(3), "n": torch.tensor(7), "b": torch.tensor([1.0, float("inf")]), "c": torch.tensor([float("nan")])}
    assert first_nonfinite(sd) == "b" and first_nonfinite({"a": torch.ones(3), "n": torch.tensor(7)}) is None and first_nonfinite({}) is None
    good = {"a": torch.ones(2)}
    assert check_finite_before_save(good, "the model", 5) is good
    with pytest.raises(RuntimeError, match="'b'"):
        check_finite_before_save(sd, "the model", 5)
