"""Adam / AdamW (include/chap_hip_optim.h) restated for the tests (a helper module, not a conftest): the fp64 restatement of chap_adam_tick and
chap_adam_step, exactly the header's definitions; a numpy fp32 emulation of the kernels, operation by operation; and the per-element error
bound the kernel is held to.  Everything is numpy on the host.

The restatement takes its hyper-parameters as the doubles it is given.  The kernels see fp32 values: kernel_hparams() rounds them the way the
ctypes structs and the launcher do (beta, eps, weight_decay, grad_scale and lr to fp32, omb = fl32(1 - (double)fl32(beta))), and the GPU tests
feed the restatement those.  With omb1 / omb2 None the restatement forms 1 - beta in double, which is torch.optim's arithmetic.

The bound, fixed before any GPU run.  Error model of tests/kernel_ref.py: a value computed in fp32 from k roundings is within gamma(k) * (sum
of the absolute values of its summands) of the exact one, gamma(k) = 2^-20 for every k <= 4096 (16 unit roundoffs).  Roundings along the
longest chain, h -> x -> m, v -> sqrt -> / -> + eps -> / -> * step_size -> p:
    h = g + g2                      1
    s = grad_scale * scale          1
    x = h * s                       1
    x + wd * p  |  p * decay        2   (product, sum | the decay word's rounding in the tick, product)
    m = b1 m + omb1 x               3   (two products, one sum; contraction can only remove one)
    v = b2 v + (omb2 x) x           4
    sqrt(v)                         1
    / bc2_sqrt                      2   (the word's rounding in the tick, the division)
    + eps                           1
    m / den                         1
    * step_size                     2   (the word's rounding in the tick, the product)
    p - ...                         1
                                   20 to p, 23 to ema (two products, one sum) -- k = 23, G = gamma(23) = 2^-20.
No stage holds more than 4 of them, so G * (the stage's summands) covers every stage on its own, and the errors of a stage's inputs are carried
through it to first order with the exact derivative bounds (|sqrt a - sqrt b| <= min(|a - b| / sqrt a, sqrt |a - b|); the quotient with the
denominator at its lower end).  The three tick words are each one rounding of an fp64 value (counted above); their fp64 arithmetic, pow
included, is 2^-29 of a unit of G and not counted.
"""
import math

import numpy as np

from tests.kernel_ref import gamma

ROUNDINGS = 23
G = gamma(ROUNDINGS)

FAULTS = ("no_bias_correction", "decay_as_l2", "eps_in_sqrt", "tick_on_skip")


def fl32(v):
    """A double -> the nearest fp32, as a double."""
    return float(np.float32(v))


def kernel_hparams(lr, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """What the kernels compute with, as doubles: dict(lr, beta1, beta2, eps, weight_decay, grad_scale, omb1, omb2)."""
    b1, b2 = fl32(beta1), fl32(beta2)
    return dict(lr=fl32(lr), beta1=b1, beta2=b2, eps=fl32(eps), weight_decay=fl32(weight_decay), grad_scale=fl32(grad_scale),
                omb1=fl32(1.0 - b1), omb2=fl32(1.0 - b2))


# ------------------------------------------------------------------------------------------ fp64 restatement
def tick_ref(step, lr, beta1, beta2, weight_decay, decoupled, skip=False):
    """chap_adam_tick in fp64, unrounded: dict(step, step_size, bc2_sqrt, decay), or None when the guard skips (nothing is written)."""
    if skip:
        return None
    t = int(step) + 1
    bc1 = 1.0 - float(beta1) ** t
    bc2 = 1.0 - float(beta2) ** t
    return dict(step=t, step_size=lr / bc1, bc2_sqrt=math.sqrt(bc2), decay=(1.0 - lr * weight_decay) if decoupled else 1.0)


def step_ref(p, g, m, v, tick, beta1, beta2, eps, weight_decay, decoupled, s=1.0, g2=None, omb1=None, omb2=None, ema=None, coef=None):
    """chap_adam_step in fp64 with `tick` = tick_ref(...) and s = grad_scale * guard scale.  Returns dict(p, m, v[, ema]) and, under 'e_p', 'e_m',
    'e_v'[, 'e_ema'], the per-element bounds on |kernel - this| (module docstring)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    omb1 = (1.0 - beta1) if omb1 is None else omb1
    omb2 = (1.0 - beta2) if omb2 is None else omb2
    h, e_h = g, np.zeros_like(g)
    if g2 is not None:
        h = g + np.asarray(g2, dtype=np.float64)
        e_h = G * np.abs(h)
    x = h * s
    e_x = abs(s) * e_h + G * np.abs(x)
    if not decoupled:
        e_x = e_x + G * (np.abs(x) + np.abs(weight_decay * p))
        x = x + weight_decay * p
        pd, e_pd = p, np.zeros_like(p)
    else:
        pd = p * tick["decay"]
        e_pd = G * np.abs(pd)
    m2 = beta1 * m + omb1 * x
    e_m = omb1 * e_x + G * (np.abs(beta1 * m) + np.abs(omb1 * x))
    v2 = beta2 * v + (omb2 * x) * x
    e_v = omb2 * (2.0 * np.abs(x) * e_x + e_x * e_x) + G * (np.abs(beta2 * v) + omb2 * x * x)
    r = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_r = np.where(r > 0, np.minimum(e_v / np.where(r > 0, r, 1.0), np.sqrt(e_v)), np.sqrt(e_v)) + G * r
    rb = r / tick["bc2_sqrt"]
    den = rb + eps
    e_den = e_r / tick["bc2_sqrt"] + G * (rb + den)
    den_lo = den - e_den
    q = m2 / den
    with np.errstate(divide="ignore", invalid="ignore"):
        e_q = np.where(den_lo > 0, e_m / den_lo + np.abs(m2) * e_den / (den * den_lo), np.inf) + G * np.abs(q)
    u = tick["step_size"] * q
    e_u = abs(tick["step_size"]) * e_q + G * np.abs(u)
    p2 = pd - u
    e_p = e_pd + e_u + G * (np.abs(pd) + np.abs(u))
    out = dict(p=p2, m=m2, v=v2, e_p=e_p, e_m=e_m, e_v=e_v)
    if ema is not None:
        a, b = float(coef[0]), float(coef[1])
        e = np.asarray(ema, dtype=np.float64)
        out["ema"] = a * e + b * p2
        out["e_ema"] = abs(b) * e_p + G * (np.abs(a * e) + np.abs(b * p2))
    return out


def within(got, ref, bound):
    """Every element of |got - ref| <= bound (non-finite `got` never is)."""
    got = np.asarray(got, dtype=np.float64)
    return bool(np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound))


def worst(got, ref, bound):
    """(index, got, ref, bound) of the element with the largest |got - ref| / bound, for a failure message."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, np.abs(got - ref) / np.where(bound > 0, bound, 1.0), np.where(got == ref, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    i = int(np.argmax(ratio))
    return i, float(got.flat[i]), float(ref.flat[i]), float(np.asarray(bound).flat[i]), float(ratio.flat[i])


# ------------------------------------------------------------------------------------------ fp32 emulation of the kernels, operation by operation
def tick_emul(state, lr, beta1, beta2, weight_decay, decoupled, skip=False, fault=None):
    """adam_tick_kernel: state = (step, step_size, bc2_sqrt, decay) with the three words np.float32.  lr, betas, weight_decay: the kernel's fp32 values."""
    if skip and fault != "tick_on_skip":
        return state
    t = int(state[0]) + 1
    lr, b1, b2, wd = (float(np.float32(a)) for a in (lr, beta1, beta2, weight_decay))
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    if fault == "no_bias_correction":
        bc1 = bc2 = 1.0
    return (t, np.float32(lr / bc1), np.float32(math.sqrt(bc2)), np.float32(1.0 - lr * wd) if decoupled else np.float32(1.0))


def step_emul(p, g, m, v, state, beta1, beta2, eps, weight_decay, decoupled, grad_scale=1.0, scale=None, g2=None, ema=None, coef=None, fault=None):
    """adam_kernel without contraction: every operation rounded to fp32.  Returns (p, m, v, ema or None) as float32 arrays."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2, eps, wd = f(beta1), f(beta2), f(eps), f(weight_decay)
    omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
    _, step_size, bc2_sqrt, decay = state
    s = f(grad_scale) if scale is None else f(grad_scale) * f(scale)
    h = g if g2 is None else g + np.asarray(g2, dtype=f)
    x = h * s
    if not decoupled or fault == "decay_as_l2":
        x = x + wd * p
    else:
        p = p * decay
    m = b1 * m + omb1 * x
    v = b2 * v + (omb2 * x) * x
    if fault == "eps_in_sqrt":
        den = np.sqrt(v / (bc2_sqrt * bc2_sqrt) + eps)
    else:
        den = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / den)
    e = None
    if ema is not None:
        e = f(coef[0]) * np.asarray(ema, dtype=f) + f(coef[1]) * p
    assert all(a.dtype == f for a in (p, m, v))
    return p, m, v, e


def clip_coef(h, grad_scale, max_norm):
    """The guard's coefficient (include/chap_hip_guard.h) of the gradient h * grad_scale, in fp64 and rounded once to fp32."""
    norm = math.sqrt(float(np.sum(np.asarray(h, dtype=np.float64) ** 2))) * grad_scale
    return fl32(min(1.0, max_norm / (norm + 1e-6))) if max_norm > 0 else 1.0
