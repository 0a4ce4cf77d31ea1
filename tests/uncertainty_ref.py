"""fp64 restatements of chap_teacher_uncertainty and chap_teacher_consistency_masked (include/chap_hip_uncertainty.h) with per-element error
bounds, an fp32 emulation of each kernel's arithmetic, and the inputs the CPU and GPU tests share (a helper module, not a conftest).

    pbar = 1/(2T) sum_k sum_h softmax(t[k][h]),  H = - sum_c pbar_c log(pbar_c + 1e-6),  m = H < thr,  count = sum m
    q = 0.5 (softmax(t[0][0]) + softmax(t[0][1])),  p_h = softmax(s_h),  e_h = p_h - q,  den = C count + 1e-16
    loss = sum_h sum m e_h^2 / den,   g_h,k = m G p_k (e_k - sum_c p_c e_c),  G = gscale * gscale_dev * 2 / den

The bounds, from the building blocks of tests/teacher_ref.py and tests/kernel_ref.py (U32 = 2^-24, gamma(n) for an n-term fp32 chain), written
down before the first GPU run of either kernel and not changed after it -- nothing below was fitted to what the kernels give:
  softmax      e_p = (ew(C) + |z - m| U32) p, teacher_ref's
  S            the sum of the 2T probabilities: d_S = sum e_p + gamma(2T) S
  pbar         S * fl(1 / 2T): d_pbar = d_S / 2T + 2 U32 pbar                     (the reciprocal's rounding and the product's)
  a            pbar + 1e-6f: d_a = d_pbar + U32 1e-6 + U32 a                       (the fp32 constant against 1e-6, the add)
  L = log a    d_L = d_a / (a - d_a) + 4 U32 |L|                                   (the argument's relative error; logf within two ulps)
  t = pbar L   d_t = d_pbar |L| + pbar d_L + U32 |t|
  H            d_H = sum_c d_t + gamma(C) sum_c |t_c|
  mask         exact wherever |H - thr| > d_H with thr the fp32 value the kernel compares against; a pixel inside that band is
               "undecided" and left out of the comparison.  At most UNDECIDED_CAP of a case's pixels may be undecided: a condition on the
               inputs, checked on the reference alone, not a tolerance.  count == mask.sum() exactly and sure <= count <= sure + undecided.
  masked term  teacher_ref's chain with den in place of N C P.  den = fl(fl(C) fl(count)) + 1e-16f: three roundings where N C P had one, so
               the loss carries 8 U32 |loss| (its 6, and 2 more) and the gradient 8 U32 |g|; everything else -- d_q, d_e, the sum's
               gamma(N C P) chain, d_dot, the accumulate's single rounding -- is teacher_ref's, term by term.  Where m = 0: the prior's bits
               (accumulate) or +0, compared exactly.
Every term is relative to a quantity of the element itself: there is no absolute floor in any comparison."""
import math

import torch

from tests import kernel_ref as kr
from tests import teacher_ref as tr

CLASSES = tr.CLASSES
SCALAR, QUADS, TWO_TRIPS, TWO_TRIPS_CLASSES = tr.SCALAR, tr.QUADS, tr.TWO_TRIPS, tr.TWO_TRIPS_CLASSES
PASSES = (1, 2, 3, 8)
FRACTIONS = (0.75, 0.9)             # thresholds as fractions of ln C; 1.0 is the method's own tie (DESIGN.md "Teacher uncertainty") and is not tested
UNDECIDED_CAP = 1e-3
EPS = 1e-6
# The generator's base seed.  The cap is a condition on the inputs and one combination needs a look: 0.75 ln 4 = 1.5 ln 2 is itself the entropy of
# a (1/2, 1/4, 1/4) mixture of saturated predictions, which four one-hot predictions (C = 4, T = 2) form with probability 9/16.  On the saturated
# (odd) samples a fraction of a percent of the pixels then lies within 1e-5 of the threshold -- the method's own tie, as ln 2 is for C = 2 at the
# end of the ramp (DESIGN.md "Teacher uncertainty").  7000, 7100 and 7200 leave 2 to 5 such pixels of about 1300 in the band at C = 4, T = 2;
# 7300 is the first base, counted on the reference alone and before any kernel ran, at which every case of both small shapes meets the cap.
BASE_SEED = 7300
ew = tr.ew


def threshold(frac, C):
    """The fp32 word the kernel compares against, as a Python float."""
    return kr._fp32_scalar(frac * math.log(C))


def inputs(C, shape, T, seed=0):
    """Student logits s[2] and teacher logits t[T][2] of one case.  Samples with even n are 1.5 randn (soft predictions: entropies on both
    sides of the thresholds), odd n are 10 randn clamped to +-30 (saturated).  Planted: teacher_ref's +-30 extremes and exact ties in every
    tensor; pixels where all 2T predictions are equal and saturated (H ~ 0); pixels where the predictions contradict each other one-hot,
    alternately class 0 and class C - 1 (H ~ ln 2); pixels with exactly uniform logits (H ~ ln C)."""
    N, sp = shape
    g = torch.Generator().manual_seed(BASE_SEED + 64 * seed + 8 * C + T)

    def mk():
        x = torch.randn(N, C, *sp, generator=g)
        x[0::2] *= 1.5
        x[1::2] = (10 * x[1::2]).clamp_(-30, 30)
        return x
    s = [mk(), mk()]
    t = [[mk(), mk()] for _ in range(T)]
    P = s[0][0, 0].numel()
    flat = lambda x: x.reshape(N, C, P)
    for k, x in enumerate(s + [h for pair in t for h in pair]):
        f = flat(x)
        f[k % N, 0, (5 + 3 * k)::37] = 30.0
        f[k % N, C - 1, (5 + 3 * k)::37] = -30.0
        f[(k + 1) % N, 0, (11 + k)::41] = f[(k + 1) % N, C - 1, (11 + k)::41]        # ties
    for j, x in enumerate(h for pair in t for h in pair):
        f = flat(x)
        f[0, :, 3::31] = -30.0
        f[0, 1 % C, 3::31] = 30.0                               # all agree, saturated
        f[0, :, 7::43] = -30.0
        f[0, 0 if j % 2 == 0 else C - 1, 7::43] = 30.0          # one-hot contradiction, half and half
        f[N - 1, :, 13::47] = 0.0                               # uniform
    flat(s[0])[0, :, 2::29] = flat(t[0][0])[0, :, 2::29]        # the student agrees with the target's first head
    return dict(N=N, C=C, T=T, sp=sp, P=P, s=s, t=t)


def _softmax(z, C):
    return tr._softmax(z, C)


def uncertainty_ref(passes, thr):
    """-> dict(H, H_b [N][...] fp64, mask (H < thr) bool, undecided bool, sure int, n_undecided int).  `thr`: the fp32 value (threshold())."""
    U = kr.U32
    T = len(passes)
    C = passes[0][0].shape[1]
    S, d_S = 0.0, 0.0
    for pair in passes:
        for z in pair:
            p, e_p = _softmax(z, C)
            S, d_S = S + p, d_S + e_p
    d_S = d_S + kr.gamma(2 * T) * S
    pbar = S / (2 * T)
    d_pbar = d_S / (2 * T) + 2 * U * pbar
    a = pbar + EPS
    d_a = d_pbar + U * EPS + U * a
    L = torch.log(a)
    d_L = d_a / (a - d_a) + 4 * U * L.abs()
    t = pbar * L
    d_t = d_pbar * L.abs() + pbar * d_L + U * t.abs()
    H = -t.sum(1)
    H_b = d_t.sum(1) + kr.gamma(C) * t.abs().sum(1)
    und = (H - thr).abs() <= H_b
    mask = H < thr
    return dict(H=H, H_b=H_b, mask=mask, undecided=und, sure=int((mask & ~und).sum()), n_undecided=int(und.sum()))


def check_mask(name, got_mask, got_count, r):
    """The mask exactly outside the band, the count exactly its sum and inside [sure, sure + undecided].  -> the undecided share."""
    got = got_mask.cpu().reshape(r["mask"].shape)
    assert bool(((got == 0) | (got == 1)).all()), name
    dec = ~r["undecided"]
    bad = (got.bool() != r["mask"]) & dec
    assert not bool(bad.any()), "%s: %d decided pixels differ, first at %s" % (name, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))
    count = int(got_count)
    assert count == int(got.sum()), (name, count, int(got.sum()))
    assert r["sure"] <= count <= r["sure"] + r["n_undecided"], (name, r["sure"], count, r["n_undecided"])
    share = r["n_undecided"] / r["mask"].numel()
    assert share <= UNDECIDED_CAP, (name, share)
    return share


def masked_ref(logits, teacher, mask, count, gscale=1.0, gscale_dev=None, prior=(None, None)):
    """-> dict(loss [1], loss_b [1], g [2], g_b [2]) in fp64, teacher_ref's chain with den = C count + 1e-16.  Where the mask is 0, g is the
    prior (or 0) and its bound 0: compared exactly."""
    U = kr.U32
    N, C = logits[0].shape[:2]
    total = logits[0].numel()
    count = int(count)
    den = C * count + 1e-16
    G = kr._fp32_scalar(gscale) * (1.0 if gscale_dev is None else float(gscale_dev)) * 2.0 / den
    m = mask.reshape((N, 1) + tuple(logits[0].shape[2:])).bool()
    (p1, b1), (p2, b2) = _softmax(teacher[0], C), _softmax(teacher[1], C)
    q = 0.5 * (p1 + p2)
    d_q = 0.5 * (b1 + b2) + U * q
    loss, loss_b, gs, gbs = 0.0, 0.0, [], []
    zero = torch.zeros((), dtype=torch.float64)
    for h in range(2):
        p, e_p = _softmax(logits[h], C)
        e = p - q
        d_e = e_p + d_q + U * e.abs()
        sq = torch.where(m, e * e, zero).sum()
        loss = loss + sq / den
        loss_b = loss_b + (torch.where(m, 2 * e.abs() * d_e + d_e * d_e + U * e * e, zero).sum() + (kr.gamma(total) + U) * sq) / den
        dot = (p * e).sum(1, keepdim=True)
        d_dot = (e_p * e.abs() + p * d_e).sum(1, keepdim=True) + (C + 1) * U * (p * e).abs().sum(1, keepdim=True)
        r = e - dot
        g = torch.where(m, G * p * r, zero)
        g_b = torch.where(m, abs(G) * (e_p * r.abs() + p * (d_e + d_dot + U * r.abs())) + 8 * U * g.abs(), zero)
        if prior[h] is not None:
            g = prior[h].double() + g
            g_b = g_b + torch.where(m, U * g.abs(), zero)
        gs.append(g)
        gbs.append(g_b)
    loss_b = loss_b + 8 * U * abs(float(loss))
    as1 = lambda v: torch.as_tensor(float(v), dtype=torch.float64).reshape(1)
    return dict(loss=as1(loss), loss_b=as1(loss_b), g=gs, g_b=gbs)


UNCERTAINTY_FAULTS = ("mean_entropy", "div_T", "no_eps", "one_head")
MASKED_FAULTS = ("den_np", "no_C", "mask_loss_only")


def _sm32(z):
    z = z.to(torch.float32)
    ex = torch.exp(z - z.amax(1, keepdim=True))
    return ex * (1.0 / ex.sum(1, keepdim=True))


def emulate_uncertainty_f32(passes, thr, fault=None):
    """The kernel's arithmetic in fp32 torch ops (torch's exp / log in place of expf / logf) -> (H fp32, mask uint8, count int).  `fault`:
      mean_entropy  the mean of the 2T predictions' entropies instead of the entropy of their mean     div_T   the divisor T where 2T belongs
      no_eps        log(pbar) without the 1e-6                                                          one_head  only each pass's first head"""
    f = torch.float32
    T = len(passes)
    heads = [pair[0] for pair in passes] if fault == "one_head" else [z for pair in passes for z in pair]
    div = T if fault in ("div_T", "one_head") else 2 * T
    inv = torch.tensor(1.0, dtype=f) / torch.tensor(float(div), dtype=f)
    eps = torch.tensor(0.0 if fault == "no_eps" else EPS, dtype=f)

    def ent(pb):
        s = torch.zeros_like(pb[:, 0])
        for c in range(pb.shape[1]):
            s = s + pb[:, c] * torch.log(pb[:, c] + eps)
        return -s
    if fault == "mean_entropy":
        H = sum(ent(_sm32(z)) for z in heads) * inv
    else:
        S = torch.zeros_like(heads[0], dtype=f)
        for z in heads:
            S = S + _sm32(z)
        H = ent(S * inv)
    mask = (H < torch.tensor(thr, dtype=f)).to(torch.uint8)
    return H, mask, int(mask.sum())


def emulate_masked_f32(logits, teacher, mask, count, gscale=1.0, gscale_dev=None, prior=(None, None), fault=None):
    """-> (loss [1] fp32, [g1, g2] fp32).  `fault`:
      den_np          N P where the count belongs        no_C   count where C count belongs        mask_loss_only  the gradient not masked"""
    f = torch.float32
    N, C = logits[0].shape[:2]
    cnt = logits[0].numel() // C if fault == "den_np" else int(count)
    Cf = 1.0 if fault == "no_C" else float(C)
    den = torch.tensor(Cf, dtype=f) * torch.tensor(float(cnt), dtype=f) + torch.tensor(1e-16, dtype=f)
    m = mask.reshape((N, 1) + tuple(logits[0].shape[2:])).bool()
    q = 0.5 * (_sm32(teacher[0]) + _sm32(teacher[1]))
    gs = torch.tensor(gscale, dtype=f) * torch.tensor(1.0 if gscale_dev is None else float(gscale_dev), dtype=f) * (torch.tensor(2.0, dtype=f) / den)
    tot, out = torch.zeros((), dtype=torch.float64), []
    for h in range(2):
        p = _sm32(logits[h])
        e = p - q
        tot = tot + torch.where(m, e * e, torch.zeros((), dtype=f)).sum(dtype=torch.float64).float().double()
        g = gs * p * (e - (p * e).sum(1, keepdim=True))
        if fault != "mask_loss_only":
            g = torch.where(m, g, torch.zeros((), dtype=f))
        if prior[h] is None:
            out.append(g)
        else:
            pr = prior[h].to(f)
            out.append(pr + g if fault == "mask_loss_only" else torch.where(m, pr + g, pr))
    return (tot.float() / den).reshape(1), out
