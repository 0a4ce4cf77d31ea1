"""fp64 restatements of the library's ops and ONE per-element error model, for the kernel tests (a helper module, not a conftest).

Tensors are CPU NC(D)HW (channel first), as the tests build them.  A restatement returns the fp64 value of what the kernel computes
from the operands the kernel multiplies -- the lazy transform rounded where the kernel rounds it, the weights rounded to the MFMA
operand type -- together with the sums of absolute terms the bound needs.  `bound` turns those into a per-element bound on
|kernel - reference|; `check` compares and names the worst element.

Constants, fixed before any GPU run and never fitted to observed errors:
  U32 = 2^-24, U_BF16 = 2^-8   unit roundoff (round to nearest) of an fp32 / bf16 value (24 / 8 significant bits).
  gamma(n) = 2^-20 * max(1, sqrt(n / 4096))
      fp32 accumulation of an n-term chain, relative to sum |term|.  The one measured figure, gfx950's fp32-input MFMA (a k-ordered
      fp32 fma chain), is 0.75-1.5e-7 * sum |a*b| from fp64 at K <= 1024 and 3.5e-7 at K = 4096; 2^-20 = 9.5e-7 covers it with a
      margin of 2.7.  Longer chains grow like sqrt(n) (independent roundings).
Chain lengths (the n of gamma) of the kernels:
  conv          K = taps * input channels + 1 (the bias add): the MFMA K loop of conv_kernel.h / conv_wp.h / conv_kpar.h (kpar splits
                it into chunks joined in LDS: shorter chains, not longer).
  statistics    a block's per-lane running sum over its tiles, a 16-lane row sum, four waves: at most the launch's pixel count.  The
                slot totals are summed in fp64 (stats_totals / bn_finalize): exact here.
  dW, db        a block's pixel loop over its share of the grid, then the slab reduction over the splits: at most the pixel count.
  act_bwd sums  a thread's grid-stride loop, the shuffle / LDS reduction, an fp64 total over the blocks: at most the pixel count.
"""
import itertools
import math

import torch
import torch.nn.functional as F

PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DECONV_FWD, PACK_DECONV_DGRAD, PACK_DOWN_DGRAD = range(5)      # = chap_amd._lib (chap_hip.h)

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def unit(dtype):
    return U32 if dtype == torch.float32 else U_BF16


def gamma(n):
    return 2.0 ** -20 * max(1.0, math.sqrt(n / 4096.0))


def f32(v):
    """fp64 -> nearest fp32 (one rounding), kept as fp64."""
    return v.float().double()


def _c(t, like=None):
    """fp64 copy, on the device of `like` (default: where it is).  The restatements run where their inputs are: CPU for the per-kernel
    tests, the GPU for the full-size launches of tests/test_step_launches_gpu.py."""
    t = t.detach().double()
    return t if like is None else t.to(like.device)


def _bcast(v, like, per_sample=False):
    """[C] (or [N, C]) -> broadcastable against an NC(D)HW tensor."""
    sh = ([like.shape[0]] if per_sample else [1]) + [-1] + [1] * (like.dim() - 2)
    return _c(v, like).reshape(sh)


def _fp32_scalar(s):
    return float(torch.tensor(float(s), dtype=torch.float32))


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def lazy_f32(x, scale=None, shift=None, act=False, slope=0.0, keep=None, keep_scale=1.0, chan_mul=None):
    """The fp32 value a kernel computes from a stored raw tensor x [N, C, *sp] (values representable in the storage type) through the
    lazy transform  v = chan_mul * keep*keep_scale * leaky(fmaf(x, scale, shift))  (common.h src_load8 / src_load1).  Each fp32 step
    is computed exactly in fp64 (a product of two fp32 values is exact) and rounded once to fp32.  The affine is an fmaf: its exact
    product plus shift is rounded in fp64 and then to fp32 -- a double rounding, at most one fp32 ulp off the kernel's fmaf.
    Returns (v, dv): dv bounds |v - the kernel's v|: two fp32 ulps (<= 4 U32 |v|: the fmaf's, and one more rounding carried through
    the later products), 0 where no affine was applied (the later products are then rounded exactly as the kernel rounds them)."""
    v = _c(x)
    affine = scale is not None
    if affine:
        v = f32(v * _bcast(scale, x) + _bcast(shift, x))
    if act:
        v = torch.where(v > 0, v, f32(v * _fp32_scalar(slope)))
    if keep is not None:
        v = torch.where(_c(keep, v) != 0, f32(v * _fp32_scalar(keep_scale)), torch.zeros_like(v))
    if chan_mul is not None:
        v = f32(v * _bcast(chan_mul, x, per_sample=True))
    dv = 4 * U32 * v.abs() if affine else torch.zeros_like(v)
    return v, dv


def add_f32(parts):
    """add-combined sources (the V-Net skip add): the fp32 sum of the transformed values.  parts: [(v, dv), ...] -> (v, dv)."""
    v = f32(sum(p[0] for p in parts))
    dv = sum(p[1] for p in parts)
    dv = torch.where(dv > 0, dv + 2 * U32 * v.abs(), dv)       # an input off by dv can move the sum's rounding by one more ulp
    return v, dv


def mfma_operand(v, dv, dtype):
    """fp32 value v (+ its uncertainty dv) -> the MFMA operand (bf16 RNE for bf16 kernels, the fp32 value itself for fp32 ones) and
    `flip`: the largest change of that operand a kernel-side value within dv of v can cause.  For bf16 it is nonzero only for values
    within dv of a bf16 rounding boundary (one bf16 ulp there); for fp32 it is dv itself."""
    if dtype == torch.float32:
        return v, dv
    a = v.float().bfloat16().double()
    d = dv * 1.001
    up = (v + d).float().bfloat16().double()
    dn = (v - d).float().bfloat16().double()
    return a, torch.maximum((up - a).abs(), (dn - a).abs())


def operand(x, dtype, **lazy):
    """lazy_f32 followed by mfma_operand: (a, flip)."""
    v, dv = lazy_f32(x, **lazy)
    return mfma_operand(v, dv, dtype)


def weight_operand(w, dtype):
    """fp32 master weight -> the packed operand (chap_pack_weights: bf16 RNE, or fp32 as is)."""
    return _c(w) if dtype == torch.float32 else w.detach().cpu().float().bfloat16().double()


# ---- convolution ------------------------------------------------------------------------------------------------------------------
def _window(t, n, stride, dims):
    return (slice(None), slice(None)) + tuple(slice(t[i], t[i] + stride * (n[i] - 1) + 1, stride) for i in range(dims))


def conv_taps(a, w, *, stride, pad):
    """y[n, o, p] = sum_{t, c} a[n, c, p*stride + t - pad] * w[o, c, t], fp64, tap by tap (shifted windows and an einsum)."""
    dims = a.dim() - 2
    k = w.shape[-1]
    ap = F.pad(a, [pad] * (2 * dims)) if pad else a
    osp = [(s - k) // stride + 1 for s in ap.shape[2:]]
    y = None
    for t in itertools.product(range(k), repeat=dims):
        term = torch.einsum("nc...,oc->no...", ap[_window(t, osp, stride, dims)], w[(slice(None), slice(None)) + t])
        y = term if y is None else y + term
    return y


def deconv_taps(a, w):
    """k2 s2 transposed conv: y[n, o, 2p + t] = sum_c a[n, c, p] * w[c, o, t], fp64."""
    dims = a.dim() - 2
    y = a.new_zeros(a.shape[0], w.shape[1], *[2 * s for s in a.shape[2:]])
    for t in itertools.product(range(2), repeat=dims):
        sl = (slice(None), slice(None)) + tuple(slice(t[i], None, 2) for i in range(dims))
        y[sl] = torch.einsum("nc...,co->no...", a, w[(slice(None), slice(None)) + t])
    return y


def conv_linear(kind, a, w):
    """The linear map of chap_conv_fwd for packed-weight `kind` (w in checkpoint layout):
      CONV_FWD      conv, k3 pad 1 / k1 / k2 s2                                w [cout, cin, k..]
      CONV_DGRAD    input gradient of the k3 / k1 conv (flipped, transposed taps) w [cout, cin, k..], a = gradient (cout channels)
      DECONV_FWD    transposed conv k2 s2 (1x1 conv + depth-to-space)           w [cin, cout, 2..]
      DECONV_DGRAD  its input gradient: conv k2 s2                              w [cin, cout, 2..], a = gradient (cout channels)
      DOWN_DGRAD    input gradient of the k2 s2 down conv (1x1 + depth-to-space) w [cout, cin, 2..], a = gradient (cout channels)"""
    k = w.shape[-1]
    if kind == PACK_CONV_FWD:
        return conv_taps(a, w, stride=2 if k == 2 else 1, pad=1 if k == 3 else 0)
    if kind == PACK_CONV_DGRAD:
        return conv_taps(a, w.transpose(0, 1).flip(list(range(2, w.dim()))), stride=1, pad=(k - 1) // 2)
    if kind == PACK_DECONV_FWD:
        return deconv_taps(a, w)
    if kind == PACK_DECONV_DGRAD:
        return conv_taps(a, w, stride=2, pad=0)
    if kind == PACK_DOWN_DGRAD:
        return deconv_taps(a, w)
    raise ValueError(kind)


def conv_ref(kind, a, w, bias=None, *, flip=None):
    """chap_conv_fwd in fp64 from its operands a (MFMA operand values, NC(D)HW; concatenated sources: torch.cat on dim 1) and w
    (weight_operand).  Returns dict(y, sabs, fterm, chain): sabs = the same map on |a|, |w| plus |bias| (sum of |term| per element),
    fterm = the map on flip, |w| (the operand-boundary term), chain = terms per element."""
    y = conv_linear(kind, a, w)
    sabs = conv_linear(kind, a.abs(), w.abs())
    fterm = conv_linear(kind, flip, w.abs()) if flip is not None and bool((flip != 0).any()) else torch.zeros_like(y)
    if bias is not None:
        y = y + _bcast(bias, y)
        sabs = sabs + _bcast(bias, y).abs()
    taps = 1 if kind in (PACK_DECONV_FWD, PACK_DOWN_DGRAD) else w.shape[-1] ** (a.dim() - 2)
    return dict(y=y, sabs=sabs, fterm=fterm, chain=a.shape[1] * taps + 1)


def conv_bound(r, store):
    """bound of a conv output; store = the stored type (None: the fp32 accumulator itself)."""
    return bound(r["y"], sabs=r["sabs"], chain=r["chain"], flip=r["fterm"], store=store)


def stats_ref(r, c=None):
    """BatchNorm statistics of a conv: (sum(v - c), sum((v - c)^2)) per channel (dim 1) over all other dims, with bounds.  The conv
    epilogues sum the fp32 accumulator plus bias BEFORE the store (conv_kernel.h / conv_wp.h: d = v - c; ssum += d; ssq += d*d), so
    each element carries the accumulator's bound e (no store term), propagated through the total:
      sum(v - c):      sum e  + (gamma(pixels) + U32) * sum |v - c|                (the chain; the subtraction's rounding)
      sum((v - c)^2):  sum (2|v - c| e + e^2)  + (gamma(pixels) + 3 U32) * sum (v - c)^2   (the chain; subtraction, square)"""
    y = r["y"]
    e = bound(y, sabs=r["sabs"], chain=r["chain"], flip=r["fterm"])
    red = [0] + list(range(2, y.dim()))
    d = y - (_bcast(c, y) if c is not None else 0.0)
    g = gamma(y[:, 0].numel())
    s1, s2 = d.sum(red), (d * d).sum(red)
    b1 = e.sum(red) + (g + U32) * d.abs().sum(red)
    b2 = (2 * d.abs() * e + e * e).sum(red) + (g + 3 * U32) * (d * d).sum(red)
    return (s1, b1), (s2, b2)


# ---- weight gradient --------------------------------------------------------------------------------------------------------------
def wgrad_ref(A, B, *, ksize, stride, flipA=None, flipB=None):
    """chap_wgrad in fp64: dW[t, kc, kn] = sum_p A[n, kc, p*stride + t - pad] * B[n, kn, p] over the grid of B (pad 1 for k3, else 0).
    A = the conv input's MFMA operand at input resolution, B = the output gradient (a transposed conv passes its fine gradient as A
    and its coarse lazy input as B; flipB: that operand's boundary term).  Returns dict(dw [taps, Ca, Cb], sabs, fterm, db, db_sabs, chain = pixels of the grid)."""
    dims = A.dim() - 2
    pad = [1 if ksize == 3 else 0] * (2 * dims)
    Ap = F.pad(A, pad)
    Fp = F.pad(flipA, pad) if flipA is not None else None
    osp = B.shape[2:]
    Bb = B.abs()
    dw, sabs, fterm = [], [], []
    for t in itertools.product(range(ksize), repeat=dims):
        win = _window(t, osp, stride, dims)
        dw.append(torch.einsum("nc...,nk...->ck", Ap[win], B))
        sabs.append(torch.einsum("nc...,nk...->ck", Ap[win].abs(), Bb))
        fterm.append(torch.einsum("nc...,nk...->ck", Fp[win], Bb) if Fp is not None else torch.zeros_like(dw[-1]))
        if flipB is not None:
            fterm[-1] = fterm[-1] + torch.einsum("nc...,nk...->ck", Ap[win].abs(), flipB)
    red = [0] + list(range(2, B.dim()))
    return dict(dw=torch.stack(dw), sabs=torch.stack(sabs), fterm=torch.stack(fterm), db=B.sum(red), db_sabs=Bb.sum(red),
                chain=B[:, 0].numel())


def wgrad_bound(r, prior=None, which="dw"):
    """dW ([taps, Ca, Cb]) or db accumulated (+=) into fp32 `prior` (None = zero): the pixel chain, the operand-boundary term, and
    the rounding of the accumulate (U32 * |prior + total|)."""
    if which == "dw":
        b, tot = bound(r["dw"], sabs=r["sabs"], chain=r["chain"], flip=r["fterm"]), r["dw"]
    else:
        b, tot = bound(r["db"], sabs=r["db_sabs"], chain=r["chain"]), r["db"]
    if prior is not None:
        tot = tot + _c(prior, tot)
    return b + U32 * tot.abs()


def to_layout(t, strides, shape):
    """[taps, kc, kn] -> the dW tensor of `shape` the kernel writes through (s_tap, s_kc, s_kn)."""
    out = torch.zeros(shape, dtype=t.dtype, device=t.device)
    out.as_strided(t.shape, strides).copy_(t)
    return out


# ---- BatchNorm / activation backward ----------------------------------------------------------------------------------------------
def act_bwd_ref(raw, grads, *, scale=None, shift=None, act=False, slope=0.0, keep=None, keep_scale=1.0, chan_mul=None,
                g_pool=None, pool_idx=None, bn_mode=0, mean=None, invstd=None, gamma_=None, count=None):
    """chap_act_bwd_reduce + _apply in fp64 (pointwise.hip act_bwd_kernel, actbwd_math.h).  raw [N, C, *sp]; grads: NC(D)HW tensors
    whose sum is the incoming gradient; g_pool / pool_idx [N, C, H/2, W/2]: a pooled gradient routed to the position
    ((y & 1) << 1 | (x & 1)) its index names in the 2x2 window.
      dz = gsum * (z > 0 ? 1 : slope) * keep*keep_scale * chan_mul,  z = raw*scale + shift (the kernel's fmaf keeps the exact sign)
      bn 0, 2: g = dz*scale (the lazy affine's own derivative; dz without one);   bn 1: g = gamma*invstd*(dz - S0/cnt - xhat*S1/cnt)
      S0 = sum dz, S1 = sum dz*xhat, xhat = (raw - mean)*invstd   (given mean: dbeta += S0, dgamma += S1)
    Returns dict(g, g_bound (without the store), S0, S1, b0, b1)."""
    r = _c(raw)
    red = [0] + list(range(2, r.dim()))
    gsum = sum(_c(g, r) for g in grads) if grads else torch.zeros_like(r)
    gabs = sum(_c(g, r).abs() for g in grads) if grads else torch.zeros_like(r)
    nterms = len(grads)
    if g_pool is not None:
        H, W = r.shape[-2:]
        ar = lambda k: torch.arange(k, device=r.device)
        me = ((ar(H).view(H, 1) & 1) << 1) | (ar(W).view(1, W) & 1)
        up = lambda t: t.repeat_interleave(2, -2).repeat_interleave(2, -1)
        routed = torch.where(up(pool_idx.to(r.device).long()) == me, up(_c(g_pool, r)), torch.zeros_like(r))
        gsum, gabs, nterms = gsum + routed, gabs + routed.abs(), nterms + 1
    fac = torch.ones_like(r)
    if act:
        z = r * _bcast(scale, r) + _bcast(shift, r) if scale is not None else r
        fac = torch.where(z > 0, fac, torch.full_like(fac, _fp32_scalar(slope)))
    if keep is not None:
        fac = fac * torch.where(_c(keep, r) != 0, _fp32_scalar(keep_scale), 0.0)
    if chan_mul is not None:
        fac = fac * _bcast(chan_mul, r, per_sample=True)
    dz = gsum * fac
    # dz: (nterms - 1) fp32 adds of the gradients, then up to three products (slope, keep scale, channel multiplier)
    e_dz = (nterms + 3) * U32 * gabs * fac.abs()
    out = dict(S0=None, S1=None, b0=None, b1=None)
    if mean is not None:
        mu, istd = _bcast(mean, r), _bcast(invstd, r)
        xhat = (r - mu) * istd
        # kernel: xh = raw*istd + fl(-mean*istd): three roundings on terms of size |raw*istd| and |mean*istd|
        e_x = 3 * U32 * (r.abs() + mu.abs()) * istd.abs()
        g = gamma(r[:, 0].numel())
        out.update(S0=dz.sum(red), S1=(dz * xhat).sum(red),
                   b0=e_dz.sum(red) + g * dz.abs().sum(red),
                   b1=(e_dz * xhat.abs() + dz.abs() * e_x).sum(red) + (g + U32) * (dz * xhat).abs().sum(red))
    if bn_mode != 1 and scale is None:
        gout, e = dz, e_dz
    elif bn_mode != 1:                                     # act_bwd_kernel: k0 = scale whenever the source has one and bn != 1
        sc = _bcast(scale, r)
        gout = dz * sc
        e = sc.abs() * e_dz + U32 * gout.abs()
    else:
        cnt = float(count)
        k0 = _bcast(gamma_, r) * istd
        k1, k2 = _bcast(out["S0"], r) / cnt, _bcast(out["S1"], r) / cnt
        cB, cC = -istd * k0 * k2, mu * istd * k0 * k2 - k0 * k1
        gout = k0 * (dz - k1 - xhat * k2)
        # kernel: g = fma(dz, k0, fma(raw, cB, cC)), cC = fma(mean*istd*k0, k2, -k0*k1); k0, k1, k2, cB and cC's two parts carry <= 4
        # fp32 roundings each and the fmas one each: 8 U32 on every term before it cancels (|cC| can be far smaller than its parts when
        # |mean| >> std) -- plus dz's error and the totals' bounds carried through k1, k2
        bb0, bb1 = _bcast(out["b0"], r), _bcast(out["b1"], r)
        cC_parts = (mu * istd * k0 * k2).abs() + (k0 * k1).abs()
        e = (8 * U32 * ((dz * k0).abs() + (r * cB).abs() + cC_parts) + k0.abs() * e_dz
             + k0.abs() * (bb0 + (r.abs() + mu.abs()) * istd.abs() * bb1) / cnt)
    out.update(g=gout, g_bound=e)
    return out


def param_grad_bound(S, b, prior=None):
    """dbeta / dgamma += a total: the total's bound, its rounding from the fp64 block total to fp32, the accumulate's rounding."""
    tot = S + (_c(prior, S) if prior is not None else 0.0)
    return b + U32 * S.abs() + U32 * tot.abs()


# ---- the error model --------------------------------------------------------------------------------------------------------------
def bound(ref, *, sabs=None, chain=1, flip=None, extra=None, store=None):
    """Per-element bound on |kernel - ref|, the sum of:
      accumulation  gamma(chain) * sabs   fp32 summation of the element's own terms (sabs = sum |term|, from the reference)
      epilogue      U32 * sabs            one more fp32 rounding on the way out (the bias add)
      operand       flip                  operands whose value may differ from the kernel's (bf16 values within one fp32 ulp of a
                                          rounding boundary, fp32 values a double rounding off the fmaf): their possible change
                                          times |the other factor|, summed over the element's terms
      extra         the caller's          a result's own propagated bound (act_bwd)
      store         unit(store) * (|ref| + the terms above)   rounding of the stored value (bf16 2^-8, fp32 2^-24; None = not stored)"""
    b = torch.zeros_like(ref)
    if sabs is not None:
        b = b + (gamma(chain) + U32) * sabs
    if flip is not None:
        b = b + flip
    if extra is not None:
        b = b + extra
    if store is not None:
        b = b + unit(store) * (ref.abs() + b)
    return b


def check(name, got, ref, bnd, dims="ncdhw"):
    """Fails with the worst element (its index named by `dims`), value, reference, bound and ratio; returns the worst |err| / bound."""
    ref = _c(ref)
    got, bnd = _c(got, ref), _c(bnd, ref)
    assert got.shape == ref.shape == bnd.shape, (name, tuple(got.shape), tuple(ref.shape), tuple(bnd.shape))
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
    flat = int(torch.argmax(ratio.reshape(-1)))
    worst = float(ratio.reshape(-1)[flat])
    if not worst <= 1.0:
        idx = []
        for s in reversed(ref.shape):
            idx.append(flat % s)
            flat //= s
        idx = tuple(reversed(idx))
        names = dims[:len(idx)] if len(dims) >= len(idx) else "?" * len(idx)
        raise AssertionError("%s: worst element (%s) = %s: got %.9g ref %.9g bound %.3g ratio %.3g" % (
            name, ",".join(names), idx, float(got[idx]), float(ref[idx]), float(bnd[idx]), worst))
    return worst
