"""fp64 restatement of the mean-teacher average that chap_sgd_ema_step computes beside the SGD update (a helper module, not a test module),
written from its definition:

    alpha(s) = min(1 - 1 / (s + 1), decay)        in double; s = the number of updates applied before this one
    a = fp32(alpha), b = fp32(1 - alpha)          each rounded on its own
    ema' = a * ema + b * p'                       p' = the parameter the same launch has just written

Error model, that of tests/kernel_ref.py (U32 = 2^-24, one rounding per fp32 operation on its absolute terms): the kernel forms two products
and an add -- or, contracted, one product and a fused multiply-add -- from the fp32 values a, b, ema and p': at most three roundings, each at
most U32 times |a ema| + |b p'|:

    |ema'_kernel - ema'_fp64| <= 3 U32 (|a ema| + |b p'|)              per element, ema and p' being the values the kernel read

With a = 0, b = 1 (the first update) the products are exact and so is the sum: ema' == p' as a value, element for element.
Fixed before the first GPU run of the kernel; not fitted to observed errors."""
import torch

from tests.kernel_ref import U32, _c, _fp32_scalar


def alpha_of(step, decay):
    return min(1.0 - 1.0 / (step + 1), decay)


def coefficients(step, decay):
    """(a, b) as fp32 values held in Python floats."""
    al = alpha_of(step, decay)
    return _fp32_scalar(al), _fp32_scalar(1.0 - al)


def ema_ref(ema, p_new, a, b):
    """One update: (ema', bound).  ema, p_new: the fp32 tensors the kernel read / wrote; a, b: the fp32 coefficients."""
    a, b = _fp32_scalar(a), _fp32_scalar(b)
    t0, t1 = a * _c(ema), b * _c(p_new)
    return t0 + t1, 3 * U32 * (t0.abs() + t1.abs())


def ema_recurrence(ema0, params, coefs):
    """The fp64 recurrence e_k = a_k e_{k-1} + b_k p_k over recorded parameters p_1..p_K (fp32 tensors), from ema0, never rounded; coefs: [(a_k, b_k)].
    A kernel-side value within B_{k-1} of e_{k-1} gives one within  B_k = |a_k| B_{k-1} + 3 U32 (|a_k| (|e_{k-1}| + B_{k-1}) + |b_k p_k|)  of e_k.
    Returns [(e_k, B_k)]."""
    e, bnd = _c(ema0), torch.zeros_like(_c(ema0))
    out = []
    for p, (a, b) in zip(params, coefs):
        a, b = _fp32_scalar(a), _fp32_scalar(b)
        t1 = b * _c(p, e)
        bnd = abs(a) * bnd + 3 * U32 * (abs(a) * (e.abs() + bnd) + t1.abs())
        e = a * e + t1
        out.append((e, bnd))
    return out
