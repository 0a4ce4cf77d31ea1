"""chap_adam_tick and chap_adam_step (include/chap_hip_optim.h) on the GPU against the fp64 restatement and the bound of tests/adam_ref.py,
which were fixed before the first run.

Sizes: 1, 3 (tail only), 4, 7, 1027 and one grid-stride trip of the launcher's capped grid plus 13 (a second trip and a tail).  Every buffer is
followed by words of a NaN bit pattern that must survive; the state block's three float words are pre-filled with it.  t starts at 0, 1, 999
and at a count where beta^t underflows.  Moments are random with some v = 0, g = 0 elements.  At n = 1027 the cases are fully crossed:
decoupled, weight decay 0 / 1e-2, second bucket, grad_scale 1 / 0.5, zero_grad, EMA, and the guard absent / scale 1 / scale c / skip."""
import collections
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from tests import adam_ref as R

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 8
PAD_BITS = 0x7FC00ABC               # a quiet NaN no arithmetic produces
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
SCALE_C = 0.37
COEF = (0.99, R.fl32(1.0 - 0.99))


def grid_cap():
    """The block cap chap_adam_step hands chap_blocks, read from the launcher."""
    src = open(os.path.join(ROOT, "chap_amd", "csrc", "optim.hip")).read()
    caps = re.findall(r"chap_blocks\(n4, (\d+)\)", src)
    assert len(caps) == 1
    return int(caps[0])


BIG = grid_cap() * 256 * 4 + 13
SIZES = [1, 3, 4, 7, 1027, BIG]
UNDERFLOW_T = 2_000_000             # 0.999^t < 2^-1074: bc2 = 1 exactly; 0.9^t long before
Case = collections.namedtuple("Case", "n t0 decoupled wd grad2 gs zero_grad ema guard")
BASE = Case(n=1027, t0=1, decoupled=True, wd=1e-2, grad2=True, gs=0.5, zero_grad=True, ema=True, guard="c")


@functools.lru_cache(maxsize=None)
def inputs(n):
    rng = np.random.default_rng(4200 + n % 9973)
    f = np.float32
    p, g, g2, e = (rng.standard_normal(n).astype(f) for _ in range(4))
    m = (0.1 * rng.standard_normal(n)).astype(f)
    v = (0.01 * rng.random(n)).astype(f)
    zero = np.arange(n) % 11 == 2
    v[zero] = 0
    g[zero] = 0
    g2[zero] = 0                    # x = 0 (or wd * p), v = 0: den = eps
    if n >= 4:
        assert zero.any()
    return dict(p=p, g=g, g2=g2, m=m, v=v, ema=e)


def padded(values):
    """A device tensor of len(values) words whose storage goes on for PAD words of PAD_BITS."""
    n = len(values)
    full = torch.full((n + PAD,), PAD_BITS, dtype=torch.int32, device=DEV)
    view = full[:n].view(torch.float32)
    view.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    return full, view


def guard_state(mode):
    if mode is None:
        return None
    scale, skip = {"one": (1.0, 0), "c": (SCALE_C, 0), "skip": (0.0, 1)}[mode]
    st = torch.zeros(ops.guard_state_words(0), dtype=torch.int32, device=DEV)
    st[0] = int(np.float32(scale).view(np.int32))
    st[1] = skip
    return st


def state_block(t0):
    return torch.tensor([t0, PAD_BITS, PAD_BITS, PAD_BITS], dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=512)
def launch(c):
    """tick + step of one case; everything read back as numpy (floats also as their bits)."""
    x = inputs(c.n)
    bufs = {k: padded(x[k]) for k in ("p", "g", "m", "v")}
    if c.grad2:
        bufs["g2"] = padded(x["g2"])
    if c.ema:
        bufs["ema"] = padded(x["ema"])
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=DEV)
    coef = torch.tensor(COEF, dtype=torch.float32, device=DEV)
    gs = guard_state(c.guard)
    state = state_block(c.t0)
    ops.adam_tick(state, lr_dev, BETAS[0], BETAS[1], c.wd, c.decoupled, gs)
    ops.adam_step(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], state, BETAS[0], BETAS[1], EPS, c.wd, c.decoupled,
                  bufs["ema"][1] if c.ema else None, coef if c.ema else None, gs, c.gs, c.zero_grad, bufs["g2"][1] if c.grad2 else None)
    torch.cuda.synchronize()
    out = {k: full.cpu().numpy() for k, (full, _) in bufs.items()}        # int32 words, pad included
    out["state"] = state.cpu().numpy()
    return out


def f32(words, n):
    return words[:n].view(np.float32)


def reference(c):
    x = inputs(c.n)
    hp = R.kernel_hparams(LR, BETAS[0], BETAS[1], EPS, c.wd, c.gs)
    tick = R.tick_ref(c.t0, hp["lr"], hp["beta1"], hp["beta2"], hp["weight_decay"], c.decoupled)
    scale = {None: 1.0, "one": 1.0, "c": R.fl32(SCALE_C)}[c.guard]
    ref = R.step_ref(x["p"], x["g"], x["m"], x["v"], tick, hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], c.decoupled,
                     s=hp["grad_scale"] * scale, g2=x["g2"] if c.grad2 else None, omb1=hp["omb1"], omb2=hp["omb2"],
                     ema=x["ema"] if c.ema else None, coef=COEF)
    return tick, ref


def check_tick(c, words):
    tick, _ = reference(c)
    assert int(words[0]) == tick["step"] == c.t0 + 1, (c, int(words[0]))
    for k, name in enumerate(("step_size", "bc2_sqrt", "decay"), 1):
        got, want = float(words[k:k + 1].view(np.float32)[0]), np.float32(tick[name])
        print("    tick %s: %.9g, restatement %.17g" % (name, got, tick[name]))
        assert abs(got - float(want)) <= float(np.spacing(want)), (c, name, got, tick[name])
    return tick


def check_case(c):
    """One launched case against the restatement: values within the bound, pads intact, buckets zeroed or kept."""
    x, out = inputs(c.n), launch(c)
    n = c.n
    for k, words in out.items():
        if k != "state":
            assert np.all(words[n:] == PAD_BITS), (c, k, "wrote behind n")
    if c.guard == "skip":
        for k, src in (("p", "p"), ("m", "m"), ("v", "v"), ("ema", "ema")):
            if k in out:
                assert np.array_equal(out[k][:n], x[src].view(np.int32)), (c, k, "written on a skipped step")
        assert out["state"].tolist() == [c.t0, PAD_BITS, PAD_BITS, PAD_BITS], (c, "the state block was written on a skipped step")
    else:
        check_tick(c, out["state"])
        _, ref = reference(c)
        for k in ("p", "m", "v") + (("ema",) if c.ema else ()):
            got = f32(out[k], n)
            i, gv, rv, bv, ratio = R.worst(got, ref[k], ref["e_" + k])
            print("    %s: worst element %d: %.9g vs %.17g, |diff| / bound = %.3g" % (k, i, gv, rv, ratio))
            assert R.within(got, ref[k], ref["e_" + k]), (c, k, i, gv, rv, bv)
        assert not np.array_equal(out["p"][:n], x["p"].view(np.int32)), c
    for k in ("g",) + (("g2",) if c.grad2 else ()):
        if c.zero_grad:
            assert np.all(out[k][:n] == 0), (c, k, "not zeroed")           # +0.0 exactly
        else:
            assert np.array_equal(out[k][:n], x[k].view(np.int32)), (c, k, "zero_grad = 0 changed the bucket")


def check_bit_relations(c):
    """What must hold bit for bit between launches of the same inputs."""
    n, out = c.n, launch(c)
    same = lambda a, b, keys: all(np.array_equal(a[k][:n], b[k][:n]) for k in keys)
    pmv = ("p", "m", "v")
    if c.guard == "one":
        other = launch(c._replace(guard=None))
        assert same(out, other, pmv + (("ema",) if c.ema else ())) and np.array_equal(out["state"], other["state"]), (c, "scale 1 differs from no guard")
    if c.guard == "c":
        eff = float(np.float32(c.gs) * np.float32(SCALE_C))            # fl32(grad_scale * c)
        other = launch(c._replace(guard=None, gs=eff))
        assert same(out, other, pmv + (("ema",) if c.ema else ())), (c, "scale c differs from grad_scale = fl32(grad_scale * c)")
    if c.ema:
        assert same(out, launch(c._replace(ema=False)), pmv), (c, "param / m / v depend on the EMA instance")


@pytest.mark.parametrize("guard", [None, "one", "c", "skip"], ids=["noguard", "scale1", "scalec", "skip"])
def test_crossed_cases(guard):
    for decoupled, wd, grad2, gs, zero_grad, ema in itertools.product((True, False), (0.0, 1e-2), (False, True), (1.0, 0.5), (True, False), (False, True)):
        c = BASE._replace(decoupled=decoupled, wd=wd, grad2=grad2, gs=gs, zero_grad=zero_grad, ema=ema, guard=guard)
        check_case(c)
        check_bit_relations(c)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    """Tail only, body only, both, several blocks, a second grid-stride trip: each with and without the optional streams, on the update and
    on the skip path."""
    for grad2, ema, guard, zero_grad in ((True, True, "c", True), (False, False, None, True), (True, False, "skip", True), (False, True, "one", False)):
        c = BASE._replace(n=n, grad2=grad2, ema=ema, guard=guard, zero_grad=zero_grad)
        check_case(c)
        check_bit_relations(c)
    launch.cache_clear()


@pytest.mark.parametrize("t0", [0, 1, 999, UNDERFLOW_T])
@pytest.mark.parametrize("decoupled", [True, False])
def test_step_counts(t0, decoupled):
    c = BASE._replace(n=1027, t0=t0, decoupled=decoupled, guard=None)
    check_case(c)
    if t0 == UNDERFLOW_T:           # both corrections are exactly 1
        w = launch(c)["state"]
        assert float(w[2:3].view(np.float32)[0]) == 1.0 and float(w[1:2].view(np.float32)[0]) == float(np.float32(LR))


def test_tick_alone_counts_and_skips():
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=DEV)
    state = state_block(0)
    for t in (1, 2, 3):
        ops.adam_tick(state, lr_dev, BETAS[0], BETAS[1], 1e-2, True)
        assert int(state[0]) == t
    before = state.clone()
    ops.adam_tick(state, lr_dev, BETAS[0], BETAS[1], 1e-2, True, guard_state("skip"))
    assert torch.equal(state, before)
    ops.adam_tick(state, lr_dev, BETAS[0], BETAS[1], 1e-2, False, guard_state("c"))
    assert int(state[0]) == 4 and float(state[3:4].view(torch.float32)) == 1.0


# ------------------------------------------------------------------------------------------ argument checks: refused before any launch
def _step_params(n=64):
    t = {k: torch.zeros(n, device=DEV) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
    state = state_block(0)
    q = L.AdamParams()
    q.param, q.grad, q.exp_avg, q.exp_avg_sq = (t[k].data_ptr() for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
    q.state = state.data_ptr()
    q.beta1, q.beta2, q.eps, q.weight_decay, q.decoupled, q.grad_scale, q.zero_grad, q.n = 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 1, n
    return q, (t, state)


def _tick_params():
    state, lr = state_block(0), torch.tensor([LR], device=DEV)
    q = L.AdamTickParams()
    q.state, q.lr, q.beta1, q.beta2, q.weight_decay, q.decoupled = state.data_ptr(), lr.data_ptr(), 0.9, 0.999, 0.0, 1
    return q, (state, lr)


STEP_REFUSALS = [
    (dict(param=None), "chap_adam_step: null param, grad, exp_avg or exp_avg_sq"), (dict(grad=None), "chap_adam_step: null param"),
    (dict(exp_avg=None), "chap_adam_step: null param"), (dict(exp_avg_sq=None), "chap_adam_step: null param"),
    (dict(state=None), "chap_adam_step: null state"), (dict(n=0), "chap_adam_step: n=0"), (dict(n=-4), "chap_adam_step: n=-4"),
    (dict(ema="buf"), "chap_adam_step: null coef"), (dict(ema="buf", coef="odd"), "chap_adam_step: coef must be 4-byte aligned"),
    (dict(beta1=1.0), "chap_adam_step: betas="), (dict(beta1=-0.1), "chap_adam_step: betas="), (dict(beta2=1.0), "chap_adam_step: betas="),
    (dict(beta2=float("nan")), "chap_adam_step: betas="), (dict(eps=0.0), "chap_adam_step: eps=0"), (dict(eps=-1e-8), "chap_adam_step: eps="),
] + [({k: "misaligned"}, "chap_adam_step: buffers, state and guard must be 16-byte aligned")
     for k in ("param", "grad", "grad2", "exp_avg", "exp_avg_sq", "ema", "state", "guard")]

TICK_REFUSALS = [
    (dict(state=None), "chap_adam_tick: null state or lr"), (dict(lr=None), "chap_adam_tick: null state or lr"),
    (dict(state="misaligned"), "chap_adam_tick: state must be 16-byte aligned"), (dict(guard="misaligned"), "chap_adam_tick: lr must be 4-byte, guard 16-byte"),
    (dict(lr="odd"), "chap_adam_tick: lr must be 4-byte, guard 16-byte aligned"),
    (dict(beta1=1.0), "chap_adam_tick: betas="), (dict(beta2=-1.0), "chap_adam_tick: betas="),
]


def _refused(name, make, change, message):
    q, keep = make()
    spare = torch.zeros(80, device=DEV)
    for k, v in change.items():
        if v == "misaligned":
            v = spare.data_ptr() + 4
            if k == "ema":
                q.coef = spare.data_ptr()
        elif v == "buf":
            v = spare.data_ptr()
        elif v == "odd":
            v = spare.data_ptr() + 2
        setattr(q, k, v)
    with pytest.raises(L.ChapError, match=re.escape(message)):
        L.call(name, q, torch.cuda.current_stream().cuda_stream)
    return keep


def test_argument_checks():
    for change, message in STEP_REFUSALS:
        t, state = _refused("chap_adam_step", _step_params, change, message)
        torch.cuda.synchronize()
        assert all(float(v.abs().max()) == 0.0 for v in t.values()) and state.tolist() == [0, PAD_BITS, PAD_BITS, PAD_BITS], change
    for change, message in TICK_REFUSALS:
        state, _ = _refused("chap_adam_tick", _tick_params, change, message)
        torch.cuda.synchronize()
        assert state.tolist() == [0, PAD_BITS, PAD_BITS, PAD_BITS], change
    for name in ("chap_adam_step", "chap_adam_tick"):           # (L.call takes the struct by reference: the null struct goes in directly)
        assert L._fn(name)(None, None) != 0 and L.lib().chap_last_error().decode() == name + ": null argument"


def test_ops_refuse_wrong_tensors_and_misaligned_views():
    n = 64
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    state = state_block(0)
    off = torch.zeros(n + 1, device=DEV)[1:]
    with pytest.raises(L.ChapError, match="16-byte aligned"):
        ops.adam_step(p, off, m, v, state, 0.9, 0.999, 1e-8, 0.0, True)
    with pytest.raises(L.ChapError, match="16-byte aligned"):
        ops.adam_step(p, g, m, v, state, 0.9, 0.999, 1e-8, 0.0, True, grad2=off)
    with pytest.raises(ValueError, match="exp_avg_sq must be a contiguous fp32 tensor of 64 elements"):
        ops.adam_step(p, g, m, v[:32], state, 0.9, 0.999, 1e-8, 0.0, True)
    with pytest.raises(ValueError, match="grad must be"):
        ops.adam_step(p, g.double(), m, v, state, 0.9, 0.999, 1e-8, 0.0, True)
    with pytest.raises(ValueError, match="state must be a contiguous int32 tensor of 4 words"):
        ops.adam_step(p, g, m, v, state[:3], 0.9, 0.999, 1e-8, 0.0, True)
    with pytest.raises(ValueError, match="state must be"):
        ops.adam_tick(state.float(), torch.zeros(1, device=DEV), 0.9, 0.999, 0.0, True)
    with pytest.raises(ValueError, match="lr_dev must be an fp32 word"):
        ops.adam_tick(state, torch.zeros(1), 0.9, 0.999, 0.0, True)
    with pytest.raises(ValueError, match="guard_state must hold"):
        ops.adam_tick(state, torch.zeros(1, device=DEV), 0.9, 0.999, 0.0, True, torch.zeros(2, dtype=torch.int32, device=DEV))
    strided = torch.zeros(2 * ops.guard_state_words(0), dtype=torch.int32, device=DEV)[::2]       # enough words, but not where the kernel reads them
    with pytest.raises(ValueError, match="guard_state must hold 8 contiguous int32 words"):
        ops.adam_tick(state, torch.zeros(1, device=DEV), 0.9, 0.999, 0.0, True, strided)
    with pytest.raises(ValueError, match="guard_state must hold 8 contiguous int32 words"):
        ops.adam_step(p, g, m, v, state, 0.9, 0.999, 1e-8, 0.0, True, guard_state=strided)
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and state.tolist() == [0, PAD_BITS, PAD_BITS, PAD_BITS]
