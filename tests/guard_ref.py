"""fp64 restatement of the gradient guard (include/chap_hip_guard.h), for tests/test_guard_*.py.  NOT a test module.

    h     = fl32(g + g2)                      the fp32 sum the optimizer kernel forms
    total = sum h^2                           math.fsum: correctly rounded
    norm  = sqrt(total) * grad_scale          fp64
    skip  = (total is inf or NaN) and skip_nonfinite
    coef  = 0 if skip else (min(1, max_norm / (norm + 1e-6)) if max_norm > 0 else 1)       clip_grad_norm_'s expression; rounded once to fp32

The kernel adds the squares (each exact in fp64) in another order than fsum: a sum of n non-negative terms is within n * 2^-53 of the exact one
whatever the order, the square root and the product with grad_scale add one rounding (2^-53) each; the bound below grants 2^-52 for each."""
import math

import numpy as np
import torch


def fl32(v):
    return float(np.float32(v))


def h_of(g, g2=None):
    """g + g2 as fp32 tensors on the CPU (IEEE addition: the same bits as the device's v_add_f32)."""
    g = g.detach().cpu().float()
    return g if g2 is None else g + g2.detach().cpu().float()


def total_of(h):
    if not bool(torch.isfinite(h).all()):
        return float("nan") if bool(torch.isnan(h).any()) else float("inf")
    return math.fsum((h.double() * h.double()).reshape(-1).tolist())      # the fp64 square of an fp32 value is exact


def guard_ref(g, g2=None, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True):
    """-> dict(norm64, norm, coef64, coef, skip, nonfinite, bound): norm64 / coef64 the fp64 values, norm / coef them rounded to fp32, bound the
    relative error granted to the kernel's fp64 norm."""
    h = h_of(g, g2)
    total = total_of(h)
    nonfinite = not math.isfinite(total)
    gs, mx = fl32(grad_scale), fl32(max_norm)
    norm = (math.sqrt(total) if total == total and total >= 0 else float("nan")) * gs
    skip = bool(nonfinite and skip_nonfinite)
    if skip:
        coef = 0.0
    elif mx > 0:
        q = mx / (norm + 1e-6)
        coef = min(1.0, q)                          # Python's min(1.0, nan) is 1.0, as C's fmin(1, NaN)
    else:
        coef = 1.0
    n = h.numel()
    return dict(norm64=norm, norm=fl32(norm), coef64=coef, coef=fl32(coef), skip=int(skip), nonfinite=nonfinite,
                bound=n * 2.0 ** -53 + 2 * 2.0 ** -52)


def ulp32(x):
    """Spacing of the fp32 numbers at |x|."""
    return float(np.spacing(np.float32(abs(x))))


def within_one_ulp(got, want):
    """fp32 `got` within one fp32 ulp of the fp32 value `want` (the kernel rounds an fp64 value that differs from the reference's in its last bits)."""
    if not math.isfinite(want):
        return (got != got and want != want) or got == want
    return abs(float(got) - float(want)) <= ulp32(want)


def clip_like_torch(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on copies of `grads` (CPU tensors): (total_norm, clipped copies)."""
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return float(total), [p.grad for p in ps]
