"""Adam / AdamW without a GPU: the fp64 restatement of include/chap_hip_optim.h (tests/adam_ref.py) against torch.optim.AdamW and torch.optim.Adam,
the fp32 emulation of the kernels and four planted faults against the restatement's error bound, the struct sizes against the header, and the
binding table's name."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import adam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 257
STEPS = 6
SKIPPED = 3                         # the step in the middle that the guard skips (torch: step() is not called)
CLIPPED = 4                         # the step whose gradient is clipped
GRAD_SCALE = 0.5
LRS = (1e-3, 7e-4, 1.3e-3, 9e-4, 2e-3, 5e-4)       # changed between the steps
BETAS, EPS = (0.9, 0.999), 1e-8


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(N)
    grads = [(rng.standard_normal(N), 0.3 * rng.standard_normal(N)) for _ in range(STEPS)]      # two buckets
    return p0, grads


@pytest.mark.parametrize("decoupled", [True, False])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_restatement_is_torch_adam(decoupled, wd):
    """Six steps in fp64: lr changed between steps, two buckets summed, grad_scale 0.5, one step clipped with clip_grad_norm_'s coefficient, one
    skipped.  1e-12 relative, per element: both sides are fp64 and differ in the order of the same operations."""
    p0, grads = _inputs()
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([tp], lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=wd)
    p, m, v, step = p0.copy(), np.zeros(N), np.zeros(N), 0
    for k in range(STEPS):
        g, g2 = grads[k]
        skip = k == SKIPPED
        # ---- torch
        for grp in opt.param_groups:
            grp["lr"] = LRS[k]
        tp.grad = (torch.tensor(g) + torch.tensor(g2)) * GRAD_SCALE
        max_norm = 0.5 * float(tp.grad.norm()) if k == CLIPPED else 0.0
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        if not skip:
            opt.step()
        # ---- the restatement
        coef = 1.0
        if max_norm > 0:
            norm = float(np.sqrt(np.sum((g + g2) ** 2))) * GRAD_SCALE
            coef = min(1.0, max_norm / (norm + 1e-6))
            assert coef < 0.51
        tick = R.tick_ref(step, LRS[k], BETAS[0], BETAS[1], wd, decoupled, skip=skip)
        if tick is not None:
            out = R.step_ref(p, g, m, v, tick, BETAS[0], BETAS[1], EPS, wd, decoupled, s=GRAD_SCALE * coef, g2=g2)
            p, m, v, step = out["p"], out["m"], out["v"], tick["step"]
        st = opt.state[tp]
        if st:
            assert int(st["step"]) == step
            for name, mine, theirs in (("p", p, tp.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
                theirs = theirs.numpy()
                err = np.abs(mine - theirs)
                assert np.all(err <= 1e-12 * np.abs(theirs)), (k, name, float(np.max(err / np.maximum(np.abs(theirs), 1e-300))))
    assert step == STEPS - 1


def _sequence(decoupled, wd, fault=None, ema=True):
    """The fp32 emulation (with `fault` planted) beside the restatement over four steps from t = 0, the third skipped: every step of the
    emulation starts from the restatement's fp32 state, so each step's error is that step's alone.  Some elements have v = 0, g = 0 and m != 0.
    Returns whether every element of every step is inside the bound."""
    rng = np.random.default_rng(5)
    f = np.float32
    hp = R.kernel_hparams(1e-3, BETAS[0], BETAS[1], EPS, wd, GRAD_SCALE)
    p = rng.standard_normal(N).astype(f)
    m = (0.1 * rng.standard_normal(N)).astype(f)
    v = (0.01 * rng.random(N)).astype(f)
    e = rng.standard_normal(N).astype(f)
    zero = np.arange(N) % 9 == 0
    v[zero] = 0
    coef = (f(0.75), f(0.25))
    state, step_ref_t = (0, f(0), f(0), f(0)), 0
    ok = True
    for k in range(4):
        g, g2 = rng.standard_normal(N).astype(f), (0.3 * rng.standard_normal(N)).astype(f)
        if k == 0:
            g[zero] = 0
            g2[zero] = 0
        skip = k == 2
        scale = 0.625 if k == 1 else 1.0
        tick = R.tick_ref(step_ref_t, hp["lr"], hp["beta1"], hp["beta2"], hp["weight_decay"], decoupled, skip=skip)
        state = R.tick_emul(state, hp["lr"], hp["beta1"], hp["beta2"], hp["weight_decay"], decoupled, skip=skip, fault=fault)
        if tick is None:
            continue                # the kernel writes nothing: a planted tick_on_skip shows in the next step's words
        step_ref_t = tick["step"]
        ref = R.step_ref(p, g, m, v, tick, hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], decoupled, s=hp["grad_scale"] * scale, g2=g2,
                         omb1=hp["omb1"], omb2=hp["omb2"], ema=e if ema else None, coef=coef)
        got = R.step_emul(p, g, m, v, state, hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], decoupled, hp["grad_scale"], scale, g2,
                          e if ema else None, coef, fault=fault)
        for name, gt in zip(("p", "m", "v", "ema"), got):
            if gt is not None:
                ok = ok and R.within(gt, ref[name], ref["e_" + name])
        p, m, v = (ref[n].astype(f) for n in ("p", "m", "v"))
        if ema:
            e = ref["ema"].astype(f)
    return ok


@pytest.mark.parametrize("decoupled", [True, False])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fp32_emulation_is_inside_the_bound(decoupled, wd):
    assert _sequence(decoupled, wd)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_are_outside_the_bound(fault):
    """Bias correction dropped, decoupled decay applied as L2, eps inside the square root, t advanced on a skipped step."""
    assert _sequence(True, 1e-2, fault=fault) is False


def test_struct_sizes_match_the_header(tmp_path):
    from chap_amd import _lib
    pairs = {"chap_adam_tick_params": ctypes.sizeof(_lib.AdamTickParams), "chap_adam_params": ctypes.sizeof(_lib.AdamParams), "chap_adam_state": 16}
    c = tmp_path / "sz.c"
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in pairs)
    c.write_text('#include <stdio.h>\n#include "chap_hip_optim.h"\nint main(void){\n%sprintf("abi %%d\\n", CHAP_ABI_VERSION);\nreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    sizes = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for name, size in pairs.items():
        assert int(sizes[name]) == size, (name, sizes[name], size)
    assert int(sizes["abi"]) == _lib.ABI_VERSION == 9
    from chap_amd import ops
    assert ops.ADAM_STATE_WORDS * 4 == 16
    # a header of its own: chap_hip.h neither holds nor includes it
    assert "adam" not in open(os.path.join(ROOT, "include", "chap_hip.h")).read().lower()


def test_binding_table_is_outside_the_walked_tables():
    """tests/test_launch_access_cpu.py walks every attribute of _lib whose name starts with _SIGS; the two entry points are bound from a table
    that it does not walk, and _fn() still finds their argtypes."""
    from chap_amd import _lib
    names = {"chap_adam_tick", "chap_adam_step"}
    for attr in dir(_lib):
        if attr.startswith("_SIGS"):
            assert not names & set(getattr(_lib, attr)), attr
    assert set(_lib._OPTIM_SIGS) == names
    assert _lib._fn("chap_adam_step").argtypes[0]._type_ is _lib.AdamParams
    assert _lib._fn("chap_adam_tick").argtypes[0]._type_ is _lib.AdamTickParams


def test_train_entries_refuse_an_unknown_optimizer_before_writing(tmp_path):
    from chap_amd import train_ours_2D, train_ours_3D
    for T in (train_ours_2D, train_ours_3D):
        assert T.FLAG_DEFAULTS["optimizer"] == "sgd" and T.FLAG_DEFAULTS["betas"] == (0.9, 0.999) and T.FLAG_DEFAULTS["adam_eps"] == 1e-8
        snap = tmp_path / T.__name__
        with pytest.raises(ValueError, match="optimizer='lion'"):
            T.train({"optimizer": "lion"}, str(snap))
        assert not snap.exists()
