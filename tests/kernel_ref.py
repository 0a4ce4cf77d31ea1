"""fp64 restatements of the library's ops and ONE per-element error model, for the kernel tests (a helper module, not a conftest).

Tensors are CPU NC(D)HW (channel first), as the tests build them.  A restatement returns the fp64 value of what the kernel computes
from the operands the kernel multiplies -- the lazy transform rounded where the kernel rounds it, the weights rounded to the MFMA
operand type -- together with the sums of absolute terms the bound needs.  `bound` turns those into a per-element bound on
|kernel - reference|; `check` compares and names the worst element.  The second half restates the plumbing kernels (losses, VAT / BCP
helpers, the counter-based RNG, the perturbation mask, SGD, GradSim) in the same way; what is an integer, a mask or a copy is exact.
The third part does the same for the evaluation kernels (ensemble_argmax, the sliding-window accumulate / finalize), the channel-drop kernels,
bn_finalize / bn_eval_affine, the channel sums and the layout converters.

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
  losses        mix_loss / kl / dice-distance accumulators: a thread's grid-stride loop, the wave shuffle, four waves, one partial row per block,
                the rows summed in fp64 (sum_partial_rows): at most the launch's pixel count N * P (kl: its 2 * C * N * P terms).
  l2_normalize  the sum of squares of a sample: a thread's loop, the wave / block reduction, an fp64 total over the slices: at most P.
  grad_sim      accumulated in fp64: no chain term.  perturb, sgd_step, the RNG, boxes, masks: elementwise, no chain.
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
def wgrad_ref(A, B, *, ksize, stride, flipA=None, flipB=None, Bv=None, dBv=None):
    """chap_wgrad in fp64: dW[t, kc, kn] = sum_p A[n, kc, p*stride + t - pad] * B[n, kn, p] over the grid of B (pad 1 for k3, else 0).
    A = the conv input's MFMA operand at input resolution, B = the output gradient (a transposed conv passes its fine gradient as A
    and its coarse lazy input as B; flipB: that operand's boundary term).  Returns dict(dw [taps, Ca, Cb], sabs, fterm, db, db_sabs, db_flip, chain = pixels of the grid).
    Bv, dBv: the fp32 value of a LAZY B and its uncertainty (lazy_f32's pair), for the bias gradient.  The kernel (wgrad_kernel.h, the commit of a
    B tile) sums db from the transformed fp32 value v and packs v to the operand type afterwards; a plain B is summed as stored.  So db of a lazy B is
    sum v, not the sum of the operands: in bf16 the two differ by up to U_BF16 |v| per pixel (independent roundings: about U_BF16 |v| sqrt(pixels) / 3 in
    all, far above the fp32 chain's gamma(pixels) sum |v|), and in either type the kernel's v may be dBv off the restated one.  Without Bv, db = sum B."""
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
    Bd = B if Bv is None else Bv
    return dict(dw=torch.stack(dw), sabs=torch.stack(sabs), fterm=torch.stack(fterm), db=Bd.sum(red), db_sabs=Bd.abs().sum(red),
                db_flip=dBv.sum(red) if dBv is not None else torch.zeros_like(Bd.sum(red)), chain=B[:, 0].numel())


def wgrad_bound(r, prior=None, which="dw"):
    """dW ([taps, Ca, Cb]) or db accumulated (+=) into fp32 `prior` (None = zero): the pixel chain, the operand-boundary term, and
    the rounding of the accumulate (U32 * |prior + total|)."""
    if which == "dw":
        b, tot = bound(r["dw"], sabs=r["sabs"], chain=r["chain"], flip=r["fterm"]), r["dw"]
    else:
        b, tot = bound(r["db"], sabs=r["db_sabs"], chain=r["chain"], flip=r.get("db_flip")), r["db"]
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


# ==== plumbing kernels: losses, VAT helpers, RNG, boxes, diff mask, SGD, GradSim =====================================================
# Elementwise budget of a SHORT fp32 chain (at most eight roundings: an expf / logf / divide counted as one each, the ROCm installed
# here ships no ulp table for them): EW = 8 U32 on the sum of the chain's |terms|, the figure act_bwd_ref uses.  A value that is a
# product of several such chains (the loss gradients: softmax factor x coefficient x softmax factor) gets EW per factor.
EW = 8 * U32
SEED_DEV_MIX = 0xD1342543DE82EF95                          # aux.hip: seed + *seed_dev * this (mod 2^64)


def softmax_ref(logits):
    """softmax_px (loss.hip) over dim 1 of fp64 logits [N, C, ...]: p_c = expf(z_c - m) / sum, lse = m + logf(sum).
    Returns dict(p, lse, e_p, e_lse, zm):
      e_p   = (EW + |z_c - m| U32) p_c   the chain expf, (C - 1) adds, reciprocal, product (<= 8 roundings for C <= 4) plus the rounding
                                        of the exponent's argument z_c - m, which expf turns into a relative error of the same size
      e_lse = EW (|m| + 1)              sum in [1, C] carries <= C + 1 roundings, logf's slope 1/sum <= 1 makes them absolute; logf's own
                                        rounding on log(sum) <= 1.4; the add's on |lse| <= |m| + 1.4
      zm    = max_c |z_c - m| per pixel."""
    z = logits
    m = z.amax(1, keepdim=True)
    ex = torch.exp(z - m)
    s = ex.sum(1, keepdim=True)
    p = ex / s
    lse = (m + torch.log(s)).squeeze(1)
    d = (z - m).abs()
    return dict(p=p, lse=lse, e_p=(EW + d * U32) * p, e_lse=EW * (m.abs().squeeze(1) + 1.0), zm=d.amax(1))


def _onehot(t, C, like):
    """[N, ...] integer labels -> fp64 [N, C, ...] (all zero for a label outside [0, C))."""
    return torch.stack([(t == c) for c in range(C)], 1).to(like.dtype)


def _dice_partials(I, Z, Y, bI, bZ, bY, s):
    """r = (2 I + s) / (Z + Y + s) with |dr| from the accumulators' bounds."""
    num, den = 2 * I + s, Z + Y + s
    r = num / den
    return num, den, r, 2 * bI / den + r * (bZ + bY) / den


def mix_loss_ref(logits, target_a, target_b=None, mask=None, w_a=1.0, w_b=0.5, smooth=1e-10, k_dice=0.0, k_ce=0.0, gscale=1.0,
                 gscale_dev=None, prior=None):
    """chap_mix_loss_fwd / _bwd in fp64.  logits [N, C, *sp]; targets, mask [N, *sp] (mask None: ones; target_b None: target_a).
    Per part k (a: weight mask, b: weight 1 - mask) the accumulators ce = sum mk (lse - z_t), I_c = sum mk p_c t_c, Z_c = sum mk p_c^2,
    Y_c = sum mk t_c, msum = sum mk over all N * P pixels, then
      dice_k = w_k / C sum_c [1 - (2 I_c + s) / (Z_c + Y_c + s)],  ce_k = w_k ce / (msum + 1e-16),  loss_k = kd dice_k + kc ce_k
      dlogits = gs (kc dz + kd p (dp - dot)),  dz_c = sum_k w_k mk / (msum_k + 1e-16) (p_c - t_kc),
      dp_c = sum_k w_k / C mk (-2 t_kc / den_kc + num_kc 2 p_c / den_kc^2),  dot = sum_c dp_c p_c         (mix_loss_bwd_kernel).
    Returns dict(acc [2, 2 + 3C] (layout of row 0 of the workspace), acc_b, loss [3], loss_b, dlogits, dlogits_b).  Bounds:
      accumulators  gamma(N * P) sum |term| + sum (elementwise error of the term) + U32 |total| (the fp64 total stored as fp32)
      loss          EW on the |terms| of each short chain (a Dice part, a CE part, the k_dice / k_ce combination), plus the accumulators'
                    bounds through the partial derivatives
      dlogits       (3 EW + 2 zm U32) * sum of the ABSOLUTE terms of kc dz + kd p (dp - dot) (each term is a product of at most three short
                    chains -- softmax, coefficient, softmax -- and both differences cancel), plus the accumulators' bounds through the
                    partial derivatives, plus U32 |prior + g| when accumulating onto `prior`."""
    z = _c(logits)
    N, C = z.shape[:2]
    total = z[:, 0].numel()
    sm = softmax_ref(z)
    p, lse = sm["p"], sm["lse"]
    s, tiny = _fp32_scalar(smooth), _fp32_scalar(1e-16)
    dflt = k_dice == 0.0 and k_ce == 0.0
    kd, kc = (0.5, 0.5) if dflt else (_fp32_scalar(k_dice), _fp32_scalar(k_ce))
    m = torch.ones_like(lse) if mask is None else _c(mask, z)
    mks = (m, 1.0 - m)
    ts = [_onehot(target_a.to(z.device), C, z), _onehot((target_a if target_b is None else target_b).to(z.device), C, z)]
    ws = (_fp32_scalar(w_a), _fp32_scalar(w_b))
    red = [0] + list(range(2, z.dim()))
    g = gamma(total)
    acc, acc_b, parts, parts_b, per = [], [], [], [], []
    for k in range(2):
        mk, t = mks[k], ts[k]
        mk1 = mk.unsqueeze(1)
        cepx = lse - (t * z).sum(1)
        ce = (cepx * mk).sum()
        b_ce = ((sm["e_lse"] + U32 * cepx.abs()) * mk).sum() + g * (cepx.abs() * mk).sum()
        I, Z, Y = (p * t * mk1).sum(red), (p * p * mk1).sum(red), (t * mk1).sum(red)
        bI = (sm["e_p"] * t * mk1).sum(red) + g * I
        bZ = ((2 * p * sm["e_p"] + U32 * p * p) * mk1).sum(red) + g * Z
        bY = g * Y
        msum = mk.sum()
        bM = g * msum
        row = torch.cat([ce.reshape(1), I, Z, Y, msum.reshape(1)])
        rb = torch.cat([b_ce.reshape(1), bI, bZ, bY, bM.reshape(1)]) + U32 * row.abs()
        b_ce, bI, bZ, bY, bM = rb[0], rb[1:1 + C], rb[1 + C:1 + 2 * C], rb[1 + 2 * C:1 + 3 * C], rb[1 + 3 * C]
        acc.append(row), acc_b.append(rb)
        num, den, r, dr = _dice_partials(I, Z, Y, bI, bZ, bY, s)
        w = ws[k]
        dice = w / C * (1.0 - r).sum()
        e_dice = EW * w / C * (1.0 + r).sum() + w / C * dr.sum()
        cek = w * ce / (msum + tiny)
        e_cek = EW * cek.abs() + w * b_ce / (msum + tiny) + cek.abs() * bM / (msum + tiny)
        parts.append(kd * dice + kc * cek)
        parts_b.append(kd * e_dice + kc * e_cek + EW * ((kd * dice).abs() + (kc * cek).abs()))
        per.append(dict(mk=mk, mk1=mk1, t=t, w=w, num=num, den=den, msum=msum, bI=bI, bZ=bZ, bY=bY, bM=bM))
    loss = torch.stack([parts[0], parts[1], parts[0] + parts[1]])
    loss_b = torch.stack([parts_b[0], parts_b[1], parts_b[0] + parts_b[1] + U32 * (parts[0] + parts[1]).abs()])
    # gradient
    gs = _fp32_scalar(gscale) * (1.0 if gscale_dev is None else float(gscale_dev))
    dz, dz_abs, dz_d = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    dp, dp_abs, dp_d = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    sh = [1, C] + [1] * (z.dim() - 2)
    for q in per:
        kce = q["w"] * q["mk1"] / (q["msum"] + tiny)
        dz = dz + kce * (p - q["t"])
        dz_abs = dz_abs + kce * (p + q["t"])
        dz_d = dz_d + kce / (q["msum"] + tiny) * q["bM"] * (p - q["t"]).abs()
        num, den = q["num"].reshape(sh), q["den"].reshape(sh)
        dnum, dden = 2 * q["bI"].reshape(sh), (q["bZ"] + q["bY"]).reshape(sh)
        co = q["w"] / C * q["mk1"]
        dp = dp + co * (-2 * q["t"] / den + num * 2 * p / den ** 2)
        dp_abs = dp_abs + co * (2 * q["t"] / den + num * 2 * p / den ** 2)
        dp_d = dp_d + co * (2 * q["t"] / den ** 2 * dden + 2 * p / den ** 2 * dnum + 4 * num * p / den ** 3 * dden)
    dot = (dp * p).sum(1, keepdim=True)
    gz = gs * (kc * dz + kd * p * (dp - dot))
    A = abs(gs) * (kc * dz_abs + kd * p * (dp_abs + (dp_abs * p).sum(1, keepdim=True)))
    prop = abs(gs) * (kc * dz_d + kd * p * (dp_d + (dp_d * p).sum(1, keepdim=True)))
    gb = (3 * EW + 2 * sm["zm"].unsqueeze(1) * U32) * A + prop
    if prior is not None:
        gz = gz + _c(prior, z)
        gb = gb + U32 * gz.abs()
    return dict(acc=torch.stack(acc), acc_b=torch.stack(acc_b), loss=loss, loss_b=loss_b, dlogits=gz, dlogits_b=gb, p=p)


def pseudo_ref(logits1, logits2):
    """chap_pseudo_block in fp64: soft1/2 with bound e_p, arg1/2 (first maximum), knowledge = (lse1 - z1[arg2]) + (lse2 - z2[arg1]) with
    bound e_lse1 + e_lse2 + U32 (|lse1 - z1[arg2]| + |lse2 - z2[arg1]| + |knowledge|), and `near` [N, *sp]: pixels whose two largest
    probabilities of either head differ, in fp64, by less than those probabilities' bounds (and by more than 0: an exact tie of the
    logits is an exact tie of the kernel's probabilities, the first index wins there) -- the argmax is undecided there."""
    out = {}
    near = None
    sms = [softmax_ref(_c(l)) for l in (logits1, logits2)]
    for i, sm in enumerate(sms):
        top = sm["p"].topk(2, dim=1)
        gap = top.values[:, 0] - top.values[:, 1]
        thr = sm["e_p"].gather(1, top.indices).sum(1)
        nr = (gap > 0) & (gap < thr)
        near = nr if near is None else near | nr
        out["soft%d" % (i + 1)], out["soft%d_b" % (i + 1)] = sm["p"], sm["e_p"]
        out["arg%d" % (i + 1)] = sm["p"].argmax(1)
    z1, z2 = _c(logits1), _c(logits2)
    k1 = sms[0]["lse"] - z1.gather(1, out["arg2"].unsqueeze(1)).squeeze(1)
    k2 = sms[1]["lse"] - z2.gather(1, out["arg1"].unsqueeze(1)).squeeze(1)
    out["knowledge"] = k1 + k2
    out["knowledge_b"] = sms[0]["e_lse"] + sms[1]["e_lse"] + U32 * (k1.abs() + k2.abs() + (k1 + k2).abs())
    out["near"] = near
    return out


NEAR_TIE_CAP = 1e-4                                        # at most 0.01 % of a case's pixels may be left out as near ties


def kl_ref(logits, targets, mode="kl", gscale=1.0, gscale_dev=None, prior=0.0):
    """chap_kl_fwd_bwd in fp64 (two heads; logits / targets: pairs of [N, C, *sp]).  Returns dict(loss, loss_b, g [2], g_b [2]); loss
    includes the prior value the kernel adds onto.
      kl    loss += 1/total sum_{h, pixel, c: t > 0} t (log t - (z - lse)),  g_h = gs/total (p - t)
            term error: EW t (|log t| + |z - lse|) + t e_lse; chain gamma(2 C total); the total times fl(1/total): 3 U32; the += : U32
            g: EW gs/total (p + t) + gs/total zm U32 p
      dice  I, Z, Y = sum p t, sum p^2, sum t^2 per head and class; loss += sum_h sum_c (1 - (2I + s)/(Z + Y + s)) / C
            g_h = gs p (dp - dot), dp_c = (-2 t / den + num 2 p / den^2) / C: bounds as in mix_loss_ref."""
    gs = _fp32_scalar(gscale) * (1.0 if gscale_dev is None else float(gscale_dev))
    zs, ts = [_c(l) for l in logits], [_c(t) for t in targets]
    N, C = zs[0].shape[:2]
    total = zs[0][:, 0].numel()
    red = [0] + list(range(2, zs[0].dim()))
    sh = [1, C] + [1] * (zs[0].dim() - 2)
    gout, gb = [], []
    if mode == "kl":
        val, vb, vabs = 0.0, 0.0, 0.0
        for z, t in zip(zs, ts):
            sm = softmax_ref(z)
            lt = torch.log(t.clamp_min(1e-300))
            zl = z - sm["lse"].unsqueeze(1)
            pos = (t > 0).to(z.dtype)
            term = pos * t * (lt - zl)
            val = val + term.sum()
            vabs = vabs + term.abs().sum()
            vb = vb + (pos * t * (EW * (lt.abs() + zl.abs()) + sm["e_lse"].unsqueeze(1))).sum()
            gout.append(gs / total * (sm["p"] - t))
            gb.append(abs(gs) / total * (EW * (sm["p"] + t) + sm["zm"].unsqueeze(1) * U32 * sm["p"]))
        v = val / total
        b = (vb + (gamma(2 * C * total) + U32) * vabs) / total + 3 * U32 * abs(v)
    else:
        s = _fp32_scalar(1e-10)
        g = gamma(total)
        v, b = 0.0, 0.0
        for z, t in zip(zs, ts):
            sm = softmax_ref(z)
            p = sm["p"]
            I, Z, Y = (p * t).sum(red), (p * p).sum(red), (t * t).sum(red)
            bI = (sm["e_p"] * t).sum(red) + (g + U32) * (p * t).abs().sum(red) + U32 * I.abs()
            bZ = (2 * p * sm["e_p"] + U32 * p * p).sum(red) + (g + U32) * Z
            bY = (g + 2 * U32) * Y
            num, den, r, dr = _dice_partials(I, Z, Y, bI, bZ, bY, s)
            v = v + (1.0 - r).sum() / C
            b = b + (EW * (1.0 + r).sum() + dr.sum()) / C
            num, den, dnum, dden = num.reshape(sh), den.reshape(sh), 2 * bI.reshape(sh), (bZ + bY).reshape(sh)
            dp = (-2 * t / den + num * 2 * p / den ** 2) / C
            dp_abs = (2 * t.abs() / den + num.abs() * 2 * p / den ** 2) / C
            dp_d = (2 * t.abs() / den ** 2 * dden + 2 * p / den ** 2 * dnum + 4 * num.abs() * p / den ** 3 * dden) / C
            dot = (dp * p).sum(1, keepdim=True)
            gout.append(gs * p * (dp - dot))
            A = abs(gs) * p * (dp_abs + (dp_abs * p).sum(1, keepdim=True))
            gb.append((3 * EW + 2 * sm["zm"].unsqueeze(1) * U32) * A + abs(gs) * p * (dp_d + (dp_d * p).sum(1, keepdim=True)))
        b = b + EW * abs(float(v))
    loss = v + float(prior)
    return dict(loss=torch.as_tensor(loss, dtype=torch.float64).reshape(1), loss_b=torch.as_tensor(b + U32 * abs(float(loss)), dtype=torch.float64).reshape(1),
                g=gout, g_b=gb)


def l2_normalize_ref(x, eps=1e-8):
    """chap_l2_normalize: out[n] = x[n] / (sqrt(sum x[n]^2) + eps).  The sum of squares is a P-term fp32 chain (relative gamma(P) on a sum
    of non-negative terms, halved by the root), then root, add, reciprocal, product: (gamma(P) + EW) |out|.  An all-zero sample: exact 0."""
    v = _c(x)
    flat = v.reshape(v.shape[0], -1)
    nrm = flat.pow(2).sum(1).sqrt().reshape([-1] + [1] * (v.dim() - 1))
    out = v / (nrm + _fp32_scalar(eps))
    return out, (gamma(flat.shape[1]) + EW) * out.abs()


def perturb_ref(x, d, alpha, mask=None, sign=False):
    """chap_perturb: out = x + (alpha * mask) * (sign ? sgn(d) : d), sgn(+-0) = 0.  Two products and an add (possibly fused): one rounding
    per operation on the absolute terms, 3 U32 (|x| + |alpha mask d|)."""
    xv, dv = _c(x), _c(d)
    if sign:
        dv = torch.sign(dv)
    t = _fp32_scalar(alpha) * (1.0 if mask is None else _c(mask, xv)) * dv
    return xv + t, 3 * U32 * (xv.abs() + t.abs())


def sgd_ref(param, grad, mom, lr, momentum, weight_decay, grad_scale=1.0, grad2=None):
    """chap_sgd_step: g = grad (+ grad2); gg = g * grad_scale + wd * p; m' = mu * m + gg; p' = p - lr * m'.  Contraction may fuse a product
    into its add, so each operation is allowed one fp32 rounding on its absolute terms:
      e_g = U32 |g| (with grad2)   e_gg = gs e_g + 2 U32 (|g gs| + |wd p|)   e_m = e_gg + 2 U32 (|mu m| + |gg|)   e_p = lr e_m + 2 U32 (|p| + |lr m'|)
    Returns (p', e_p, m', e_m)."""
    p, g, m = _c(param), _c(grad), _c(mom)
    lr, mu, wd, gs = (_fp32_scalar(v) for v in (lr, momentum, weight_decay, grad_scale))
    e_g = torch.zeros_like(g)
    if grad2 is not None:
        g = g + _c(grad2, g)
        e_g = U32 * g.abs()
    gg = g * gs + wd * p
    e_gg = abs(gs) * e_g + 2 * U32 * ((g * gs).abs() + (wd * p).abs())
    m2 = mu * m + gg
    e_m = e_gg + 2 * U32 * ((mu * m).abs() + gg.abs())
    p2 = p - lr * m2
    e_p = abs(lr) * e_m + 2 * U32 * (p.abs() + (lr * m2).abs())
    return p2, e_p, m2, e_m


def grad_sim_ref(gl, gu, score, ema=0.0):
    """chap_grad_sim: score = ema score + (1 - ema) cos(gl[c], gu[c]) per row; the cosine is accumulated in fp64 and rounded once to fp32,
    1 - ema once, then two products and an add: 4 U32 (|ema score| + |(1 - ema) sim|).  A zero row: sim = 0 exactly."""
    a, b = _c(gl).reshape(gl.shape[0], -1), _c(gu).reshape(gu.shape[0], -1)
    sim = (a * b).sum(1) / (a.pow(2).sum(1).sqrt() * b.pow(2).sum(1).sqrt() + 1e-12)
    e = _fp32_scalar(ema)
    t0, t1 = e * _c(score, a), (1.0 - e) * sim
    return t0 + t1, 4 * U32 * (t0.abs() + t1.abs())


# ---- counter-based RNG (aux.hip u01): exact integers ------------------------------------------------------------------------------
def u01_np(seed, idx, seed_dev=None):
    """u01(seed, i) of aux.hip in numpy uint64 arithmetic (wraps mod 2^64 as the kernel's does): the 24-bit integer z >> 40; the kernel's
    float is that integer times 2^-24, exact.  seed_dev: the device word mixed into the seed (None: absent)."""
    import numpy as np
    M64 = (1 << 64) - 1
    sd = (int(seed) + (0 if seed_dev is None else int(seed_dev) * SEED_DEV_MIX)) & M64
    with np.errstate(over="ignore"):
        z = np.uint64(sd) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(idx).astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.int64)


def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def _lsr(z, s):
    return (z >> s) & ((1 << (64 - s)) - 1)


def u01_int(seed, n, seed_dev=None, device="cpu"):
    """u01_np for indices 0..n-1 in torch int64 (two's-complement wrap = the uint64 arithmetic; logical shifts masked), on `device`: the
    full-size masks of a training step are restated on the GPU.  tests/test_kernel_ref_cpu.py asserts it equals u01_np."""
    sd = _s64(int(seed) + (0 if seed_dev is None else int(seed_dev) * SEED_DEV_MIX))
    i = torch.arange(1, n + 1, dtype=torch.int64, device=device)
    z = i * _s64(0x9E3779B97F4A7C15) + sd
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return _lsr(z, 40)


def keep_mask_ref(seed, n, p, seed_dev=None, device="cpu"):
    """keep[i] = u01(seed, i) >= p (uint8), the comparison in fp32 as the kernel's: bit-exact."""
    u = u01_int(seed, n, seed_dev, device).float() * (1.0 / 16777216.0)
    return (u >= torch.tensor(p, dtype=torch.float32)).to(torch.uint8)


def chan_mask_ref(seed, n, p, seed_dev=None, device="cpu"):
    """mul[i] = u >= p ? 1 / (1 - p) : 0 in fp32 (IEEE divide, subtract): bit-exact."""
    pf = torch.tensor(p, dtype=torch.float32, device=device)
    keep = u01_int(seed, n, seed_dev, device).float() * (1.0 / 16777216.0) >= pf
    return torch.where(keep, 1.0 / (1.0 - pf), torch.zeros((), device=device))


def rand_uniform_ref(seed, n, lo, hi, seed_dev=None, device="cpu"):
    """lo + fl(hi - lo) * u in fp64, and the bound: the multiply-add may be fused or not; unfused, the product's rounding is U32 |d u| even
    where the sum cancels, so "one fp32 ulp" is taken at the larger of the operands and the result: 2^-23 max(|lo|, |d u|, |value|)."""
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    d = float(hi32 - lo32)
    du = d * (u01_int(seed, n, seed_dev, device).double() / 16777216.0)
    v = float(lo32) + du
    return v, 2.0 ** -23 * torch.maximum(torch.maximum(du.abs(), v.abs()), torch.full_like(v, abs(float(lo32))))


# ---- BCP boxes ------------------------------------------------------------------------------------------------------------------
def box_inside(shape, box):
    """bool [*shape] (shape = (H, W) with box (y0, x0, bh, bw), or (D, H, W) with (z0, y0, x0, bd, bh, bw)): inside the box."""
    nd = len(shape)
    ins = torch.zeros(shape, dtype=torch.bool)
    ins[tuple(slice(max(int(box[i]), 0), max(int(box[i]) + int(box[nd + i]), 0)) for i in range(nd))] = True
    return ins


def box_mix_ref(a, b, box):
    """out = inside ? b : a; a, b [N, (1,) *shape]."""
    shape = a.shape[-(len(box) // 2):]
    return torch.where(box_inside(shape, box).to(a.device), b, a)


def box_mask_ref(n, shape, box):
    """int64 [N, *shape]: 0 inside the box, 1 outside."""
    return (~box_inside(shape, box)).long().unsqueeze(0).repeat(n, *([1] * len(shape)))


# ---- diff mask ------------------------------------------------------------------------------------------------------------------
def diff_mask_k(topk, M):
    """the definition's count (oracle.train_step.create_mask_v1): max(int(topk * M), 1) in double."""
    return max(int(topk * M), 1)


def exact_knowledge(N, H, W, scale, gen, ties=None):
    """knowledge >= 0 [N, H, W] of multiples of 2^-10 whose scale x scale cell sums are T * 2^-10 with T = 2^14 + a permutation of
    0..M-1 per sample: every partial sum is a multiple of 2^-10 below 2^7 (17 significant bits), so the pooled mean is exact in fp32 in any
    summation order and the pooled values of a sample are distinct.  ties = (k, count): `count` further cells of each sample are given
    the k-th largest value."""
    PH, PW = H // scale, W // scale
    M, q = PH * PW, scale * scale
    assert M <= 2 ** 16 and q == 16
    T = torch.stack([torch.randperm(M, generator=gen) for _ in range(N)]) + 2 ** 14
    if ties is not None:
        k, count = ties
        for n in range(N):
            order = T[n].argsort(descending=True)
            T[n, order[k:k + count]] = int(T[n, order[k - 1]])
    px = torch.randint(0, 1024, (N, M, q), generator=gen)
    px[:, :, 0] = T - px[:, :, 1:].sum(2)
    assert int(px.min()) >= 0
    kn = px.reshape(N, PH, PW, scale, scale).permute(0, 1, 3, 2, 4).reshape(N, H, W)
    return kn.double().mul(2.0 ** -10).float()


def diff_mask_ref(p1, p2, knowledge, scale, k):
    """(p1 != p2) OR the cells whose pooled value is >= the k-th largest of their sample (all ties at that value included), fp64 pooling."""
    if knowledge.dim() == 4:
        n, d, h, w = knowledge.shape
        return diff_mask_ref(p1.reshape(n, d * h, w), p2.reshape(n, d * h, w), knowledge.reshape(n, d * h, w), scale, k).reshape(n, d, h, w)
    n = knowledge.shape[0]
    pooled = F.avg_pool2d(_c(knowledge).unsqueeze(1), scale).squeeze(1).clamp_min(0)
    thr = pooled.reshape(n, -1).topk(k, dim=1).values[:, -1]
    sel = (pooled >= thr.view(n, 1, 1)).repeat_interleave(scale, 1).repeat_interleave(scale, 2)
    return (sel | (p1 != p2)).float()


# ---- test inputs shared by tests/test_plumbing_kernels_gpu.py and tests/test_kernel_ref_cpu.py -----------------------------------
LOSS_SHAPES = {"2d_ragged": (3, 4, (37, 50)),              # P % 4 = 2: the scalar KL path, a ragged last wave
               "3d_c2": (2, 2, (9, 13, 20)),               # the C = 2 instances, P % 4 = 0: the quads path
               "2d_two_trips": (3, 4, (211, 209)),         # 132 297 pixels > 512 * 256: a second grid-stride trip for some threads only
               "3d_c2_offset": (2, 2, (8, 12, 20))}        # P % 4 = 0, logits one float into their buffer: the scalar path again


def loss_inputs(name):
    """CPU inputs of a loss case (tests/test_kernel_ref_cpu.py asserts their near-tie share)."""
    N, C, sp = LOSS_SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    l1, l2 = torch.randn(N, C, *sp, generator=g) * 2, torch.randn(N, C, *sp, generator=g) * 2
    # planted exact ties of the largest logit: two classes (40 pixels per head), three classes (C = 4: 24 pixels): the first index wins
    P = l1[0, 0].numel()
    for lg, off in ((l1, 0), (l2, 7)):
        flat = lg.reshape(N, C, P)
        for j in range(40):
            n, px = j % N, (off + 997 * j) % P
            top = flat[n, :, px].max() + 1.0
            flat[n, C - 1, px] = top
            flat[n, (j % (C - 1)), px] = top
        if C == 4:
            for j in range(24):
                n, px = j % N, (off + 3 + 1013 * j) % P
                top = flat[n, :, px].max() + 0.5
                flat[n, 1:, px] = top
    ta, tb = torch.randint(0, C, (N, *sp), generator=g), torch.randint(0, C, (N, *sp), generator=g)
    mask = (torch.rand(N, *sp, generator=g) > 0.4).long()
    t1 = torch.softmax(torch.randn(N, C, *sp, generator=g), 1)
    t2 = torch.softmax(torch.randn(N, C, *sp, generator=g), 1)
    t2.reshape(N, C, P)[:, 0, ::5] = 0.0                   # targets with exact zeros: the t > 0 guard of the KL term
    t2 = t2 / t2.sum(1, keepdim=True)                      # ... still summing to 1 over the classes, as the kernel's KL gradient p - t assumes
    return dict(N=N, C=C, sp=sp, l1=l1, l2=l2, ta=ta, tb=tb, mask=mask, t1=t1, t2=t2)


def spiral(H, W, cut=None):
    """a one-pixel-wide rectangular spiral walked inwards from the top-left corner, one blank pixel between its arms: ONE component under
    8-connectivity, with a long union-find chain.  cut = fraction of the path at which one pixel of a straight stretch is cleared: two
    components (the arms are two pixels apart, nothing else links them)."""
    im = torch.zeros(H, W, dtype=torch.int64)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W
    y, x, dy, dx = 0, 0, 0, 1
    im[0, 0] = 1
    path = [(0, 0)]
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and im[ny, nx] == 0 and (not inside(fy, fx) or im[fy, fx] == 0):
                break
            dy, dx = dx, -dy                               # turn right
        else:
            break
        y, x = ny, nx
        im[y, x] = 1
        path.append((y, x))
    if cut is not None:
        i = int(cut * len(path))
        while not (path[i - 1][0] == path[i + 1][0] or path[i - 1][1] == path[i + 1][1]):
            i += 1
        im[path[i]] = 0
    return im


def serpentine(H, W):
    """rows 0, 2, 4, .. full (runs of W pixels), joined alternately at the right and the left end: one component."""
    im = torch.zeros(H, W, dtype=torch.int64)
    im[0::2] = 1
    for j, y in enumerate(range(1, H - 1, 2)):
        im[y, W - 1 if j % 2 == 0 else 0] = 1
    return im


# ==== evaluation, channel-drop, BatchNorm-finalize and layout kernels ================================================================
# Chains (every bound below was written before the first GPU run):
#   softmax_c (loss.hip)   __expf(x) compiles to v_exp_f32(fl(x * fl(log2 e))) (clang's __clang_hip_math.h): the subtract, the float constant and
#                          the product each put a relative d U32 (d = |z - m|) on the exponential; then the exp, C - 1 adds, one reciprocal, one
#                          product.  v_exp_f32 returns 0 for a result below the smallest normal number.
#   bn_finalize            fp32 slot values summed in fp64 (relative 2^-53 per add: the term `ulp64`), then the fp32 roundings counted below.
#   channel sums           a thread's pixel loop, the shuffle / LDS reduction: an fp32 chain of at most the pixels one result sums.
#   channel_drop           one block: fp32 chains over nchunk and over C, then the short elementwise chain of the probability.
# A term whose fp64 value is below EXP_UNDERFLOW may be 0 in the kernel.  v_exp_f32 has no denormal results: it returns 0 once its ROUNDED argument
# fl(x * fl(log2 e)) is below -126, and that argument is off by up to 3 d U32 log2 e = 2^-22.6 d from the true one (d <= 88 here: 2^-16): the true term is then
# below 2^(-126 + 2^-16).  2^-126 itself, the figure of a kernel with an exact argument, would leave such a term unbounded; the next power of two, 2^-125, is
# taken -- the only place where this bound is wider than "the reference's term is below 2^-126".
EXP_UNDERFLOW = 2.0 ** -125


def infer_softmax_ref(logits):
    """softmax_c over dim 1 of fp64 logits [N, C, ...], C <= 8.  Returns dict(p, e_p):
      e_p = (max(EW, (C + 2) U32) + 3 d U32) p + (2^-125 where exp(z - m) < 2^-125: EXP_UNDERFLOW above says why not 2^-126)."""
    z = logits
    C = z.shape[1]
    m = z.amax(1, keepdim=True)
    d = (z - m).abs()
    ex = torch.exp(z - m)
    s = ex.sum(1, keepdim=True)
    p = ex / s
    e = (max(EW, (C + 2) * U32) + 3 * d * U32) * p
    return dict(p=p, e_p=e + torch.where(ex < EXP_UNDERFLOW, EXP_UNDERFLOW, 0.0))


def label_ref(p, e_p):
    """(first maximal index over dim 1, near): near = the two largest values differ by more than 0 (an exact tie of the reference is an exact
    tie of the kernel for these kernels' inputs: the first index wins) and by no more than the sum of their bounds."""
    if p.shape[1] == 1:
        z = torch.zeros(p[:, 0].shape, dtype=torch.int64, device=p.device)
        return z, z.bool()
    top = p.topk(2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    thr = e_p.gather(1, top.indices).sum(1)
    return p.argmax(1), (gap > 0) & (gap <= thr)


def ensemble_ref(a, b, mode):
    """chap_ensemble_argmax: a, b fp32 logits [N, C, *sp] (the unused head may be None).  Returns dict(p, e_p, label, near).
      model1 / model2   softmax_c of one head
      logit_ensemble    softmax_c of fl(a + b) / 2: the add rounds once, the halving is exact.  The reference rounds the sum to fp32 as the kernel does (an
                        fp32 add is correctly rounded, so fl of the fp64 sum IS the kernel's value) instead of carrying U32 |a + b| / 2 through the softmax
                        as a term 2 * that on e_p: tighter, at the price that the reference shares the kernel's first operation -- a wrong add (a
                        head read twice, a missing halving) still shows, as an error of the size of the logits
      prob_ensemble     fl(p1 + p2) / 2: (e_p1 + e_p2) / 2 + U32 p"""
    if mode == "model1":
        r = infer_softmax_ref(_c(a))
    elif mode == "model2":
        r = infer_softmax_ref(_c(b))
    elif mode == "logit_ensemble":
        r = infer_softmax_ref(f32(_c(a) + _c(b)) / 2.0)
    elif mode == "prob_ensemble":
        r1, r2 = infer_softmax_ref(_c(a)), infer_softmax_ref(_c(b))
        p = (r1["p"] + r2["p"]) / 2.0
        r = dict(p=p, e_p=(r1["e_p"] + r2["e_p"]) / 2.0 + U32 * p)
    else:
        raise ValueError(mode)
    r["label"], r["near"] = label_ref(r["p"], r["e_p"])
    return r


def window_accumulate_ref(logits, origins, score0, cnt0):
    """chap_window_accumulate: logits [K, C, pw, ph, pd], origins [(x, y, z)] * K, score0 [C, W, H, D] and cnt0 [W, H, D] (what the buffers held).
    Per voxel the covering patches in patch order k: value = prior + sum_k p_k, one fp32 add per patch.
    Returns dict(score, score_b, cnt, covered): score_b = sum_k e_p,k + n_cover U32 (|prior| + sum_k p_k); 0 where no patch covers (the voxel
    must be left as it was); cnt exact."""
    lg = _c(logits)
    prior = _c(score0, lg)
    K, C, pw, ph, pd = lg.shape
    sm = infer_softmax_ref(lg)
    sp, se, n = torch.zeros_like(prior), torch.zeros_like(prior), torch.zeros_like(prior[0])
    for k, (x, y, z) in enumerate(origins):
        sl = (slice(x, x + pw), slice(y, y + ph), slice(z, z + pd))
        sp[(slice(None),) + sl] += sm["p"][k]
        se[(slice(None),) + sl] += sm["e_p"][k]
        n[sl] += 1
    return dict(score=prior + sp, score_b=se + n * U32 * (prior.abs() + sp), cnt=_c(cnt0, lg) + n, covered=n > 0)


def window_finalize_ref(score, cnt, e_score=None):
    """chap_window_finalize: v = fl(score / cnt) with bound e_score / cnt + U32 |v|; label = the first maximal index (near as label_ref).  Where cnt == 0
    the quotient is not finite (0 / 0 = NaN): `empty` names those voxels, their value and bound are set to 0 here and the caller asserts them apart."""
    s, c = _c(score), _c(cnt, score).unsqueeze(0)
    empty = (c == 0).squeeze(0)
    cs = torch.where(c == 0, torch.ones_like(c), c)
    v = torch.where(c == 0, torch.zeros_like(s), s / cs)
    b = (torch.zeros_like(s) if e_score is None else _c(e_score, s)) / cs + U32 * v.abs()
    b = torch.where(c == 0, torch.zeros_like(b), b)
    label, near = label_ref(v.unsqueeze(0), b.unsqueeze(0))
    return dict(score=v, score_b=b, label=label[0], near=near[0] & ~empty, empty=empty)


def bn_finalize_ref(slots, nslots, C, Clog, count, shift, gamma_, beta, rm, rv, momentum, eps):
    """chap_bn_finalize.  slots: fp32 [>= nslots, 2 (S | Q), Clog]; rows >= nslots are not read.  S, Q = the fp64 totals over the slots in use and over the
    Clog / C sub-lattice rows; n = the fp32 count.
      ms = S / n;  var = max(Q / n - ms^2, 0)                                   fp64
      mean = fl(shift + ms)   invstd = fl(1 / sqrt(var + eps))                  one fp32 rounding each
      scale = fl(gamma invstd)                                                  one more
      shift' = beta - mean scale                                                product and subtract, fused or not: U32 (|mean scale| + |shift'|)
      running_mean' = fl(fl(fl(1 - mom) rm) + fl(mom mean))                     fl(1 - mom) is the kernel's own value (a correctly rounded subtract);
      running_var'  = the same with unb = fl(var n / (n - 1)) (n > 1; else var)  two products and an add, fused or not: U32 (|a| + |b| + |sum|)
    Every bound also carries `ulp64`, the fp64 summation error of the totals (2^-53 per add on sum |slot value|), through the partial derivatives -- it matters
    only where var cancels.  Returns dict name -> (value, bound); running statistics only when momentum > 0 and rm is given."""
    sl = _c(slots)[:nslots]
    n = float(torch.tensor(float(count), dtype=torch.float32))
    nsub = Clog // C
    fold = lambda t: t.reshape(nsub, C).sum(0)
    S, Q = fold(sl[:, 0].sum(0)), fold(sl[:, 1].sum(0))
    terms = nslots * nsub + 4
    dS, dQ = 2.0 ** -53 * terms * fold(sl[:, 0].abs().sum(0)), 2.0 ** -53 * terms * fold(sl[:, 1].abs().sum(0))
    ms = S / n
    raw = Q / n - ms * ms
    var = raw.clamp_min(0.0)
    dvar = dQ / n + 2 * ms.abs() * dS / n + 2.0 ** -52 * (Q.abs() / n + ms * ms)
    eps = _fp32_scalar(eps)
    sft = _c(shift, sl) if shift is not None else torch.zeros_like(S)
    gam, bet = _c(gamma_, sl), _c(beta, sl)
    mean = sft + ms
    e_mean = U32 * mean.abs() + dS / n
    invstd = 1.0 / torch.sqrt(var + eps)
    e_inv = U32 * invstd + 0.5 * invstd * dvar / (var + eps)
    scale = gam * invstd
    e_scale = gam.abs() * e_inv + U32 * scale.abs()
    sh = bet - mean * scale
    e_sh = scale.abs() * e_mean + mean.abs() * e_scale + U32 * ((mean * scale).abs() + sh.abs())
    out = dict(mean=(mean, e_mean), invstd=(invstd, e_inv), scale=(scale, e_scale), shift=(sh, e_sh))
    mom = _fp32_scalar(momentum)
    if mom > 0 and rm is not None:
        om = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(mom, dtype=torch.float32))
        unb = var * n / (n - 1.0) if n > 1.0 else var
        e_unb = U32 * unb + dvar * (n / (n - 1.0) if n > 1.0 else 1.0)
        for name, old, new, e_new in (("running_mean", _c(rm, sl), mean, e_mean), ("running_var", _c(rv, sl), unb, e_unb)):
            a, b = om * old, mom * new
            out[name] = (a + b, mom * e_new + U32 * (a.abs() + b.abs() + (a + b).abs()))
    return out


def bn_eval_ref(gamma_, beta, rm, rv, eps):
    """chap_bn_eval_affine: scale = gamma rsqrtf(rv + eps), shift = beta - rm scale.
      scale   the add (U32 on rv + eps: U32 / 2 on the root), rsqrtf (v_rsq_f32: an approximation good to one ulp = 2 U32, not a correctly rounded result), the
              product: 4 U32 |scale|
      shift   fused: one rounding, U32 |shift|; not fused: U32 |rm scale| + U32 |shift|: the larger (second) form is the bound; plus |rm| e_scale.
    Returns ((scale, e_scale), (shift, e_shift))."""
    g, b, m, v = (_c(t) for t in (gamma_, beta, rm, rv))
    scale = g / torch.sqrt(v + _fp32_scalar(eps))
    e_scale = 4 * U32 * scale.abs()
    shift = b - m * scale
    return (scale, e_scale), (shift, m.abs() * e_scale + U32 * ((m * scale).abs() + shift.abs()))


def _chan_red(t):
    return [0] + list(range(2, t.dim()))


def channel_sum_ref(lazy, prior=None):
    """chap_channel_sum: out[c] += sum over all pixels of a lazy activation.  lazy = (v, dv) of lazy_f32, [N, C, *sp].  The chain is the N * P pixels a result
    sums (a thread's loop, the shuffles, the LDS rows; the block rows are totalled in fp64): gamma(N P) sum |v| + sum dv, then param_grad_bound for the
    fp32 total and its += .  Returns (prior + S, bound)."""
    v, dv = lazy
    red = _chan_red(v)
    S = v.sum(red)
    b = gamma(v[:, 0].numel()) * v.abs().sum(red) + dv.sum(red)
    return S + (_c(prior, S) if prior is not None else 0.0), param_grad_bound(S, b, prior)


def sample_channel_sum_ref(lazy):
    """chap_sample_channel_sum: per-sample sums [N, C] of a lazy activation, delivered as partial rows whose SUM is the contract (how the pixels are
    dealt to the rows is not).  A row is an fp32 chain over its pixels, the caller adds the rows in fp64: gamma(P) sum |v| + sum dv.
    Returns dict(sum, sum_b, mean, mean_b): mean = sum / P, what channel_drop consumes."""
    v, dv = lazy
    red = list(range(2, v.dim()))
    P = v[0, 0].numel()
    S = v.sum(red)
    b = gamma(P) * v.abs().sum(red) + dv.sum(red)
    return dict(sum=S, sum_b=b, mean=S / P, mean_b=b / P)


def channel_drop_ref(u1, u2, B, mode, *, pool_partial=None, npix=1, grad_sim=None, comp=False, branch=0, prob_kind="sigmoid"):
    """chap_channel_drop in fp64.  u1, u2 [U, C] uniforms; mode 'dropout2d' | 'comp_binomial' | 'scores'; pool_partial fp32 [U, nchunk, C].
    scores with an all-zero grad_sim is dropout2d.  The chain of the probabilities (kernel order):
      a = sum_k partial_k                 fp32 chain of nchunk: gamma(nchunk) sum |partial|
      s = gs * (a * fl(1 / npix))         two products: |gs / npix| e_a + 2 U32 |s|
      mean = sum_c s / C                  chain of C, a divide: (gamma(C) sum |s| + sum e_s) / C + U32 |mean|
      q = sum_c (s - mean)^2              d = s - mean: e_d = e_s + e_mean + U32 |d|;  e_q = sum (2 |d| e_d + e_d^2) + (gamma(C) + U32) q
      sigma = sqrtf(q / (C - 1))          divide, root: e_var = e_q / (C - 1) + U32 var;  e_sigma = e_var / (2 sigma) + U32 sigma
      sigmoid: z = d / (sigma + 1e-8);  pr = 1 / (1 + expf(2 z))        the add, the divide, expf, the add, the divide: one U32 each, propagated
      gauss:   z = d / (2 sigma + 1e-8); pr = 0.5 (1 + erff(z / sqrt 2)) the same with erff (|erf'| <= 2 / sqrt pi exp(-x^2)) and the rounded constant
    masks: m = (u < q), q = 1 - pr (one more rounding) or pr: decided where |u - q| > e_q, `near` elsewhere.  mul = fl(m U C / count): exact count, the
    product exact (integers), one divide: U32 |mul|.  An empty mask: 0 / 0, every element of it NaN.  Rows [0, B) are 1.
    Returns dict(mode, probs, probs_b, mul1, mul1_b, mul2, mul2_b, near1, near2, nan1, nan2); mul / bounds [B + U, C]."""
    u1, u2 = _c(u1), _c(u2, u1)
    U, C = u1.shape
    ones = torch.ones(B, C, dtype=torch.float64, device=u1.device)
    full = lambda m: torch.cat((ones, m))
    zb = torch.zeros(B + U, C, dtype=torch.float64, device=u1.device)
    none = torch.zeros(U, C, dtype=torch.bool, device=u1.device)
    if mode == "scores" and not bool((_c(grad_sim) != 0).any()):
        mode = "dropout2d"
    if mode != "scores":
        m1 = torch.where(u1 < 0.5, 2.0, 0.0)
        m2 = 2.0 - m1 if mode == "comp_binomial" else torch.where(u2 < 0.5, 2.0, 0.0)
        return dict(mode=mode, probs=None, probs_b=None, mul1=full(m1), mul1_b=zb, mul2=full(m2), mul2_b=zb, near1=none, near2=none, nan1=False, nan2=False)
    part, gs = _c(pool_partial, u1), _c(grad_sim, u1).reshape(1, C)
    nchunk = part.shape[1]
    inv = _fp32_scalar(1.0 / npix)
    a = part.sum(1)
    e_a = gamma(nchunk) * part.abs().sum(1)
    s = gs * (a * inv)
    e_s = gs.abs() * inv * e_a + 2 * U32 * s.abs()
    mean = s.mean(1, keepdim=True)
    e_mean = (gamma(C) * s.abs().sum(1, keepdim=True) + e_s.sum(1, keepdim=True)) / C + U32 * mean.abs()
    d = s - mean
    e_d = e_s + e_mean + U32 * d.abs()
    q = (d * d).sum(1, keepdim=True)
    e_q = (2 * d.abs() * e_d + e_d * e_d).sum(1, keepdim=True) + (gamma(C) + U32) * q
    var = q / (C - 1)
    e_var = e_q / (C - 1) + U32 * var
    sigma = var.sqrt()
    e_sigma = e_var / (2 * sigma).clamp_min(1e-300) + U32 * sigma
    tiny = _fp32_scalar(1e-8)
    if prob_kind == "gauss":
        den = sigma * 2.0 + tiny
        e_den = 2 * e_sigma + U32 * den
    else:
        den = sigma + tiny
        e_den = e_sigma + U32 * den
    z = d / den
    e_z = e_d / den + z.abs() * e_den / den + U32 * z.abs()
    if prob_kind == "gauss":
        k = _fp32_scalar(0.70710678118654752)
        x = z * k
        e_x = k * e_z + 2 * U32 * x.abs()
        er = torch.erf(x)
        e_er = 2 / math.sqrt(math.pi) * torch.exp(-x * x) * e_x + e_x * e_x + U32 * er.abs()
        pr = (0.5 * (1.0 + er)).clamp(0.0, 1.0)
        e_pr = 0.5 * (e_er + U32 * (1.0 + er).abs())
    else:
        t = torch.exp(2.0 * z)
        e_t = t * (2 * e_z + 4 * e_z * e_z + U32)
        w = 1.0 + t
        e_w = e_t + U32 * w
        pr = 1.0 / w
        e_pr = e_w / (w * w) + U32 * pr
    pk, e_pk = 1.0 - pr, e_pr + U32 * (1.0 - pr).abs()
    q1, e1 = (pr, e_pr) if (comp and branch == 1) else (pk, e_pk)
    q2, e2 = (pr, e_pr) if (comp and branch == 0) else (pk, e_pk)
    out = dict(mode=mode, probs=pr, probs_b=e_pr, q1=q1, q1_b=e1, q2=q2, q2_b=e2)
    for i, (u, qq, ee) in enumerate(((u1, q1, e1), (u2, q2, e2)), 1):
        m = (u < qq).double()
        cnt = float(m.sum())
        mul = m * (U * C) / cnt if cnt > 0 else torch.zeros_like(m)
        out["mul%d" % i], out["mul%d_b" % i] = full(mul), torch.cat((torch.zeros_like(ones), U32 * mul.abs()))
        out["near%d" % i], out["nan%d" % i] = (u - qq).abs() <= ee, cnt == 0
    return out


def channel_drop_check(tag, r, B, mul1, mul2, probs=None):
    """compares a launch of chap_channel_drop (mul1, mul2 [B + U, C]; probs [U, C] or None) with channel_drop_ref's `r`; returns the worst err / bound.
    An element whose comparison u < q fp64 cannot decide (`near`; at most NEAR_TIE_CAP of a mask) may take either value: the count is then the kernel's own."""
    worst = 0.0
    if probs is not None and r["mode"] == "scores":
        worst = check(tag + " probs", probs, r["probs"], r["probs_b"], "uc")
    for i, got in ((1, mul1), (2, mul2)):
        got = _c(got, r["mul%d" % i])
        assert bool((got[:B] == 1).all()), (tag, "rows [0, B)")
        if r["nan%d" % i]:
            assert bool(torch.isnan(got[B:]).all()), (tag, "an empty mask is 0 / 0 everywhere")
            continue
        near = r["near%d" % i]
        assert float(near.double().mean()) <= NEAR_TIE_CAP, (tag, "near ties", int(near.sum()))
        ref, bnd = r["mul%d" % i], r["mul%d_b" % i]
        if bool(near.any()):
            m = torch.where(near, got[B:] != 0, ref[B:] != 0).double()
            ref = torch.cat((ref[:B], m * m.numel() / m.sum()))
            bnd = torch.cat((bnd[:B], U32 * ref[B:]))
        worst = max(worst, check("%s mul%d" % (tag, i), got, ref, bnd, "nc"))
    return worst


def fold_ref(g, coff, C, mul, B, U, dtype):
    """chap_fold_perturbed: g [B + U, ..., ld] (values representable in `dtype`), channels [coff, coff + C).  out[n] = g[n] for n < B - U: a copy, exact;
    out[B - U + u] = fmaf(g[B + u], mul[B + u], g[B - U + u]) (v + w without mul): one fp32 rounding, then the store.  Returns (out [B, ..., C], bound)."""
    gg = _c(g)[..., coff:coff + C]
    out = gg[:B].clone()
    e = torch.zeros_like(out)
    if U > 0:
        w = gg[B:]
        if mul is not None:
            w = w * _c(mul, gg)[B:].reshape([U] + [1] * (gg.dim() - 2) + [C])
        out[B - U:] = out[B - U:] + w
        e[B - U:] = bound(out[B - U:], extra=U32 * out[B - U:].abs(), store=dtype)
    return out, e


def planar_to_cl_ref(x, out0, out_coff=0, cpad=0):
    """chap_planar_to_cl: fp32 x [N, C, *sp] -> channels [out_coff, out_coff + max(C, cpad)) of out0 [N, ..., ld] (what the buffer held; its dtype is the
    output's): x rounded to that dtype to nearest even, zeros in [C, cpad), every other element untouched.  Exact: returns the expected tensor."""
    N, C = x.shape[:2]
    out = out0.clone()
    cl = x.reshape(N, C, -1).transpose(1, 2).reshape(*out0.shape[:-1], C)
    out[..., out_coff:out_coff + C] = cl.to(out0.dtype)
    if cpad > C:
        out[..., out_coff + C:out_coff + cpad] = 0
    return out


# chap_cl_to_planar has no restatement of its own: its output IS lazy_f32's (v, dv) -- v within dv, dv = 0 (exact) without an affine -- as [N, C, *sp].


# ---- inputs shared by tests/test_eval_plumbing_kernels_gpu.py and tests/test_kernel_ref_cpu.py ------------------------------------------
ENSEMBLE_SCALES = {"model1": (1.0, 8.0, 30.0), "model2": (1.0, 8.0, 30.0), "logit_ensemble": (1.0, 8.0, 30.0), "prob_ensemble": (1.0, 3.0)}


ENSEMBLE_TWO_TRIPS = (3, (419, 419))                        # N, spatial size of the second-grid-stride-trip case (C = 2)


def ensemble_inputs(C, scales, N=5, sp=(37, 41), seed=3):
    """randn logits of two heads times a per-sample scale (cycled over the samples); pixel (0, 0) of sample 0: an exact tie of all classes."""
    g = torch.Generator().manual_seed(seed)
    sc = torch.tensor([scales[i % len(scales)] for i in range(N)]).view(N, 1, *([1] * len(sp)))
    a, b = torch.randn(N, C, *sp, generator=g) * sc, torch.randn(N, C, *sp, generator=g) * sc
    a[(0, slice(None)) + (0,) * len(sp)] = 1.0
    b[(0, slice(None)) + (0,) * len(sp)] = 1.0
    return a, b


WINDOW_CASE = dict(vol=(20, 18, 14), patch=(12, 10, 8), calls=(((8, 8, 6), (0, 0, 0), (4, 3, 2)), ((8, 0, 6), (0, 8, 0), (8, 8, 6))))


def window_inputs(C, vol, patch, calls, seed=5, scale=4.0):
    """per call the patch logits (randn * scale); a nonzero prior score / cnt (cnt a small integer), both 0 in the corner block [:2, -2:, -2:] so that an
    uncovered voxel with nothing in it (0 / 0) exists when no patch reaches that corner."""
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn(len(o), C, *patch, generator=g) * scale for o in calls]
    score0 = torch.rand(C, *vol, generator=g)
    cnt0 = torch.randint(1, 4, vol, generator=g).float()
    score0[:, :2, -2:, -2:] = 0
    cnt0[:2, -2:, -2:] = 0
    return logits, score0, cnt0


DROP_SHAPES = ((1, 2), (3, 16), (5, 24), (12, 256), (64, 256))


def channel_drop_inputs(U, C, nchunk=3, npix=35, seed=0, prob_kind="sigmoid", comp=False, branch=0):
    """pool_partial [U, nchunk, C] (positive, as sums of activations), grad_sim [C], uniforms u1, u2 [U, C]: drawn, then every u within 4x the bound of its q
    (channel_drop_ref) is moved to the far side of that band, away from q.  Returns dict(..., moved = their count)."""
    g = torch.Generator().manual_seed(1000 * U + C + seed)
    part = torch.rand(U, nchunk, C, generator=g) * npix / nchunk
    gs = torch.randn(C, generator=g)
    u1, u2 = torch.rand(U, C, generator=g), torch.rand(U, C, generator=g)
    r = channel_drop_ref(u1, u2, 0, "scores", pool_partial=part, npix=npix, grad_sim=gs, comp=comp, branch=branch, prob_kind=prob_kind)
    moved = 0
    for u, key in ((u1, "q1"), (u2, "q2")):
        q, e = r[key], 4 * r[key + "_b"]
        close = (u.double() - q).abs() <= e
        moved += int(close.sum())
        away = torch.where(u.double() >= q, q + 2 * e + 1e-6, q - 2 * e - 1e-6).clamp(0.0, 1.0).float()
        u[close] = away[close]
    return dict(part=part, gs=gs, u1=u1, u2=u2, npix=npix, moved=moved)
