"""Thin tensor-level wrappers over the C ABI (one Python function per entry point).

Activations are torch tensors shaped [N, D, H, W, C] (channel-last; D == 1 for 2D nets) of dtype
float32 or bfloat16.  torch is used for memory, streams and dtype bookkeeping only: every kernel
launched here is hand-written HIP from libchap_hip.so, enqueued on torch's current stream.
"""
import torch

from . import _lib as L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dt(t):
    if t.dtype == torch.float32:
        return L.F32
    if t.dtype == torch.bfloat16:
        return L.BF16
    raise TypeError("unsupported activation dtype %s" % t.dtype)


def _p(t):
    return None if t is None else t.data_ptr()


class Lazy:
    """A stored raw tensor + the transform consumers apply while loading it
    (a = keep * keep_scale * chan_mul * leaky(scale*raw + shift))."""

    __slots__ = ("raw", "C", "coff", "scale", "shift", "act", "slope", "keep", "keep_scale", "chan_mul")

    def __init__(self, raw, scale=None, shift=None, act=False, slope=0.0, keep=None, keep_scale=1.0,
                 chan_mul=None, C=None, coff=0):
        self.raw, self.scale, self.shift = raw, scale, shift
        self.act, self.slope = bool(act), float(slope)
        self.keep, self.keep_scale, self.chan_mul = keep, float(keep_scale), chan_mul
        self.C = raw.shape[-1] if C is None else C
        self.coff = coff

    @property
    def ld(self):
        return self.raw.shape[-1]

    def fill(self, s):
        s.ptr, s.scale, s.shift = _p(self.raw), _p(self.scale), _p(self.shift)
        s.keep, s.chan_mul = _p(self.keep), _p(self.chan_mul)
        s.C, s.ld, s.coff = self.C, self.ld, self.coff
        s.act, s.slope, s.keep_scale = int(self.act), self.slope, self.keep_scale
        return s

    def src(self):
        return self.fill(L.Src())


def pack_weights(w, kind, dtype, cin, cout, taps):
    """w: fp32 parameter in checkpoint layout -> packed tensor (uint8 storage) in `dtype`."""
    p = L.PackParams()
    p.w, p.kind, p.Cin, p.Cout, p.taps = w.data_ptr(), kind, cin, cout, taps
    p.dtype = L.F32 if dtype == torch.float32 else L.BF16
    nbytes = L.size_of("chap_pack_size", p)
    out = L.hold_empty(nbytes, dtype=torch.uint8, device=w.device)
    p.out = out.data_ptr()
    L.call("chap_pack_weights", p, _stream())
    return out


def conv_fwd(srcs, wpacked, bias, cout, out, *, grid, in_dims, ksize, stride, dims, combine=0,
             out_ld=None, out_coff=0, out_mode=0, out_cn=0, out_planar=False, out_f32=False,
             stats=None, stats_shift=None, out2=None):
    """stats: fp32 buffer from `stats_buffer(cout)` (per-block partial slots of the shifted moments, chap_hip.h);
    stats_shift: fp32 [real channels] or None.  out2: a second output tensor taking the channels [out.shape[-1], cout) (chap_conv_params.out2)."""
    p = L.ConvParams()
    for i, s in enumerate(srcs):
        s.fill(p.src[i])
    p.nsrc, p.combine = len(srcs), combine
    p.N, p.D, p.H, p.W = grid
    p.ID, p.IH, p.IW = in_dims
    p.ksize, p.stride, p.dims = ksize, stride, dims
    p.wpacked, p.bias, p.out = wpacked.data_ptr(), _p(bias), out.data_ptr()
    p.Cout = cout
    p.out_ld = out.shape[-1] if out_ld is None else out_ld
    p.out_coff, p.out_mode, p.out_Cn = out_coff, out_mode, out_cn
    p.out_planar, p.out_f32 = int(out_planar), int(out_f32)
    p.stats, p.stats_shift = _p(stats), _p(stats_shift)
    p.dtype = dt(srcs[0].raw)
    if out2 is not None:
        assert out2.shape == out.shape and out2.dtype == out.dtype and cout == 2 * out.shape[-1]
        p.out2, p.out2_from = out2.data_ptr(), out.shape[-1]
    L.call("chap_conv_fwd", p, _stream())


def stats_size(clog):
    """floats of a BatchNorm-statistics buffer for a conv with `clog` logical output channels."""
    return L.STATS_HDR + L.STATS_MAX_SLOTS * 2 * clog


def stats_buffer(clog, device):
    return L.hold_empty(stats_size(clog), dtype=torch.float32, device=device)


def stats_totals(stats, clog, creal=None):
    """Host-side view of a statistics buffer (tests / debugging): fp64 [2, creal] = (sum(v - c), sum((v - c)^2)) over all
    slots in use, the sub-lattice rows of a transposed conv (clog = nsub * creal) folded.  Synchronises."""
    n = int(stats[:1].view(torch.int32).item())
    t = stats[L.STATS_HDR:L.STATS_HDR + n * 2 * clog].view(n, 2, clog).double().sum(0)
    creal = clog if creal is None else creal
    return t.view(2, clog // creal, creal).sum(1)


def stats_from_moments(s, q):
    """A one-slot statistics buffer holding the given per-channel moments (tests of chap_bn_finalize)."""
    c = s.numel()
    buf = torch.zeros(stats_size(c), dtype=torch.float32, device=s.device)
    buf[:1].view(torch.int32).fill_(1)
    buf[L.STATS_HDR:L.STATS_HDR + c] = s
    buf[L.STATS_HDR + c:L.STATS_HDR + 2 * c] = q
    return buf


def conv_c1_fwd(x, w, bias, out, *, dims, stats=None, stats_shift=None):
    """x: fp32 [N, D, H, W] (C == 1)."""
    p = L.ConvC1Params()
    p.x, p.w, p.bias, p.out = x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr()
    p.stats, p.stats_shift = _p(stats), _p(stats_shift)
    p.N, p.D, p.H, p.W = x.shape
    p.dims, p.Cout, p.dtype = dims, out.shape[-1], dt(out)
    L.call("chap_conv_c1_fwd", p, _stream())


def conv_c1_bwd(g, w, x, *, dims, dx=None, dw=None, db=None):
    p = L.ConvC1BwdParams()
    p.g, p.w, p.x = g.data_ptr(), w.data_ptr(), _p(x)
    p.dx, p.dw, p.db = _p(dx), _p(dw), _p(db)
    p.N, p.D, p.H, p.W = g.shape[:4]
    p.dims, p.Cout, p.dtype = dims, g.shape[-1], dt(g)
    ws = None
    if dw is not None or db is not None:
        ws = L.hold_empty(L.size_of("chap_conv_c1_bwd_ws", p), dtype=torch.uint8, device=g.device)
        p.ws = ws.data_ptr()
    L.call("chap_conv_c1_bwd", p, _stream())


def wgrad(a_srcs, b, dw, strides, *, grid, in_dims, ksize, stride, dims, combine=0, db=None, kc_valid=0, kn_valid=0):
    p = L.WgradParams()
    for i, s in enumerate(a_srcs):
        s.fill(p.a[i])
    p.na, p.combine = len(a_srcs), combine
    b.fill(p.b)
    p.N, p.D, p.H, p.W = grid
    p.ID, p.IH, p.IW = in_dims
    p.ksize, p.stride, p.dims = ksize, stride, dims
    p.dw = dw.data_ptr()
    p.s_tap, p.s_kc, p.s_kn = strides
    p.db = _p(db)
    p.kc_valid, p.kn_valid = kc_valid, kn_valid
    p.dtype = dt(b.raw)
    nbytes = L.size_of("chap_wgrad_ws", p)
    ws = L.hold_empty(max(nbytes, 16), dtype=torch.uint8, device=dw.device)
    p.ws, p.ws_bytes = ws.data_ptr(), nbytes
    L.call("chap_wgrad", p, _stream())


def bn_finalize(stats, gamma, beta, running_mean, running_var, nbt, count, eps, momentum,
                scale, shift, mean=None, invstd=None, stats_shift=None, clog=None):
    """stats: the conv's partial-slot buffer; clog: its logical channel count (C * sub-positions for a transposed conv);
    stats_shift: the shift the conv was given (read before running_mean is updated)."""
    p = L.BnFinalizeParams()
    p.stats, p.stats_shift, p.gamma, p.beta = stats.data_ptr(), _p(stats_shift), gamma.data_ptr(), beta.data_ptr()
    p.Clog = gamma.numel() if clog is None else clog
    p.running_mean, p.running_var, p.num_batches_tracked = _p(running_mean), _p(running_var), _p(nbt)
    p.scale, p.shift, p.mean, p.invstd = scale.data_ptr(), shift.data_ptr(), _p(mean), _p(invstd)
    p.C, p.count, p.eps, p.momentum = gamma.numel(), float(count), eps, momentum
    L.call("chap_bn_finalize", p, _stream())


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, scale, shift):
    p = L.BnEvalParams()
    p.gamma, p.beta, p.running_mean, p.running_var = gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr()
    p.scale, p.shift, p.C, p.eps = scale.data_ptr(), shift.data_ptr(), gamma.numel(), eps
    L.call("chap_bn_eval_affine", p, _stream())


def act_pool2(lazy, out, idx=None, dims=2):
    p = L.PoolParams()
    lazy.fill(p.r)
    p.out, p.idx = out.data_ptr(), _p(idx)
    p.N, p.H, p.W = lazy.raw.shape[0], lazy.raw.shape[2], lazy.raw.shape[3]
    p.D = lazy.raw.shape[1] if dims == 3 else 1
    p.dtype = dt(lazy.raw)
    L.call("chap_act_pool2", p, _stream())


def upsample2x(lazy, out, *, dims, out_coff=0, half_pixel=False):
    p = L.UpsampleParams()
    p.half_pixel = int(half_pixel)
    lazy.fill(p.r)
    p.out, p.out_ld, p.out_coff = out.data_ptr(), out.shape[-1], out_coff
    p.N, p.D, p.H, p.W = lazy.raw.shape[:4]
    p.dims, p.dtype = dims, dt(lazy.raw)
    L.call("chap_upsample2x", p, _stream())


def upsample2x_bwd(g, g_coff, C, out, *, dims):
    p = L.UpsampleBwdParams()
    p.g, p.g_ld, p.g_coff, p.out = g.data_ptr(), g.shape[-1], g_coff, out.data_ptr()
    p.N, p.D, p.H, p.W = out.shape[:4]
    p.C, p.dims, p.dtype = C, dims, dt(g)
    L.call("chap_upsample2x_bwd", p, _stream())


def _act_bwd_params(lazy, grads, g_pool, pool_idx, mean, invstd, gamma, sums, gout, dgamma, dbeta, count):
    p = L.ActBwdParams()
    for i, (g, coff) in enumerate(grads):
        p.g[i], p.g_ld[i], p.g_coff[i] = g.data_ptr(), g.shape[-1], coff
    p.ng = len(grads)
    p.g_pool, p.pool_idx = _p(g_pool), _p(pool_idx)
    lazy.fill(p.r)
    p.mean, p.invstd, p.gamma, p.sums = _p(mean), _p(invstd), _p(gamma), _p(sums)
    p.gout, p.dgamma, p.dbeta = _p(gout), _p(dgamma), _p(dbeta)
    p.N, p.D, p.H, p.W = lazy.raw.shape[:4]
    p.bn, p.count, p.dtype = int(mean is not None), float(count), dt(lazy.raw)
    return p


def act_bwd(lazy, grads, gout, *, g_pool=None, pool_idx=None, mean=None, invstd=None, gamma=None,
            dgamma=None, dbeta=None, count=1.0, bn_mode=None, sums=None):
    """grads: list of (tensor, channel offset).
    bn_mode 1 (default when mean is given): training-mode BN backward fused in;
    bn_mode 2: fixed affine (eval-mode BN), dgamma/dbeta from the same reduction when requested."""
    if bn_mode is None:
        bn_mode = 1 if mean is not None else 0
    need_reduce = bn_mode == 1 or (bn_mode == 2 and (dgamma is not None or dbeta is not None))
    if need_reduce and sums is None:
        sums = L.hold_empty(act_bwd_sums_size(lazy.C), dtype=torch.float32, device=gout.device)
    p = _act_bwd_params(lazy, grads, g_pool, pool_idx, mean, invstd, gamma, sums, gout, dgamma, dbeta, count)
    p.bn = bn_mode
    if need_reduce:
        L.call("chap_act_bwd_reduce", p, _stream())
    L.call("chap_act_bwd_apply", p, _stream())
    return sums


def act_bwd_sums_size(c):
    """floats of the BN-backward workspace: row 0 = totals, rows 1.. = per-block partials (chap_hip.h)."""
    return (1 + L.ACT_BWD_SLOTS) * 2 * c


def residual_fwd(r, srcs, out, xin=None):
    """chap_residual_fwd: out = relu(a(r) + t) with t = the block input: the sum of the lazy sources `srcs` (one or two), or xin
    (fp32 [N, D*H*W], the one-channel image broadcast over the channels) when there are none.  r: the last stage's Lazy (act off)."""
    p = L.ResidualParams()
    r.fill(p.r)
    for i, s in enumerate(srcs):
        s.fill(p.src[i])
    p.nsrc, p.xin, p.out = len(srcs), _p(xin), out.data_ptr()
    p.N, p.D, p.H, p.W = r.raw.shape[:4]
    p.dtype = dt(r.raw)
    L.call("chap_residual_fwd", p, _stream())


def residual_bwd(grads, out, gout, chan_mul=None, dxin=None):
    """chap_residual_bwd: gout = (sum of up to three grads) * chan_mul * [out > 0]; grads: list of (tensor, channel offset);
    dxin (fp32 [N, D*H*W] or None) receives the channel sum of the unrounded value."""
    p = L.ResidualBwdParams()
    if len(grads) > 3:
        raise ValueError("residual_bwd: %d gradient contributions (1..3; fold the oldest with grad_sum)" % len(grads))
    for i, (g, coff) in enumerate(grads):
        p.g[i], p.g_ld[i], p.g_coff[i] = g.data_ptr(), g.shape[-1], coff
    p.ng = len(grads)
    p.out, p.chan_mul, p.gout, p.dxin = out.data_ptr(), _p(chan_mul), gout.data_ptr(), _p(dxin)
    p.N, p.D, p.H, p.W, p.C = out.shape
    p.dtype = dt(out)
    L.call("chap_residual_bwd", p, _stream())


def grad_sum(grads, out):
    """chap_grad_sum: out [..., C] = ((g0 + g1) + g2) + g3 of two to four (tensor, channel offset) contributions, fp32 adds."""
    p = L.GradSumParams()
    if len(grads) > 4:
        raise ValueError("grad_sum: %d tensors (2..4)" % len(grads))
    for i, (g, coff) in enumerate(grads):
        p.g[i], p.g_ld[i], p.g_coff[i] = g.data_ptr(), g.shape[-1], coff
    p.ng, p.out, p.npix, p.C, p.dtype = len(grads), out.data_ptr(), out[..., 0].numel(), out.shape[-1], dt(out)
    L.call("chap_grad_sum", p, _stream())


def channel_sum(lazy, out):
    p = L.ChanSumParams()
    lazy.fill(p.r)
    ws = L.hold_empty(L.CHANSUM_SLOTS * lazy.C, dtype=torch.float32, device=out.device)
    p.ws = ws.data_ptr()
    p.out, p.npix, p.pix_per_sample, p.dtype = out.data_ptr(), lazy.raw[..., 0].numel(), lazy.raw[0, ..., 0].numel(), dt(lazy.raw)
    L.call("chap_channel_sum", p, _stream())


def planar_to_cl(x, out, out_coff=0, cpad=0):
    """fp32 [N, C, *spatial] -> out [N, D, H, W, ld] (dtype of out); channels [C, cpad) zero-filled."""
    p = L.PlanarToClParams()
    N, Cc = x.shape[0], x.shape[1]
    p.in_, p.out, p.N, p.C, p.P = x.data_ptr(), out.data_ptr(), N, Cc, x[0, 0].numel()
    p.out_ld, p.out_coff, p.Cpad, p.dtype = out.shape[-1], out_coff, cpad, dt(out)
    L.call("chap_planar_to_cl", p, _stream())


def cl_to_planar(lazy, out):
    p = L.ClToPlanarParams()
    lazy.fill(p.r)
    p.out, p.N, p.P, p.dtype = out.data_ptr(), lazy.raw.shape[0], lazy.raw[0, ..., 0].numel(), dt(lazy.raw)
    L.call("chap_cl_to_planar", p, _stream())


# ------------------------------------------------------------------------------------------
# losses / training-loop helpers (fp32 planar logits [N, C, *spatial])
def mix_loss_fwd(logits, target_a, target_b, mask, w_a, w_b, smooth=1e-10, k_dice=0.0, k_ce=0.0):
    """Returns (loss[3] = (loss_a, loss_b, total), acc) -- acc is needed by mix_loss_bwd.
    target_b / mask may be None (mask of ones); (k_dice, k_ce) = (0, 0) selects mix_loss's 0.5 / 0.5."""
    N, Cc = logits.shape[0], logits.shape[1]
    p = L.MixLossParams()
    acc = L.hold_empty((1 + L.LOSS_SLOTS) * 2 * (2 + 3 * Cc), dtype=torch.float32, device=logits.device)     # row 0 = totals (read by mix_loss_bwd)
    loss = L.hold_empty(3, dtype=torch.float32, device=logits.device)
    p.logits, p.target_a, p.target_b, p.mask = logits.data_ptr(), target_a.data_ptr(), _p(target_b), _p(mask)
    p.w_a, p.w_b, p.acc, p.loss = w_a, w_b, acc.data_ptr(), loss.data_ptr()
    p.N, p.C, p.P, p.smooth, p.k_dice, p.k_ce = N, Cc, logits[0, 0].numel(), smooth, k_dice, k_ce
    L.call("chap_mix_loss_fwd", p, _stream())
    return loss, acc


def mix_loss_bwd(logits, target_a, target_b, mask, w_a, w_b, acc, dlogits, gscale=1.0, accumulate=False, smooth=1e-10, k_dice=0.0, k_ce=0.0,
                 gscale_dev=None):
    N, Cc = logits.shape[0], logits.shape[1]
    p = L.MixLossParams()
    p.logits, p.target_a, p.target_b, p.mask = logits.data_ptr(), target_a.data_ptr(), _p(target_b), _p(mask)
    p.w_a, p.w_b, p.acc, p.dlogits = w_a, w_b, acc.data_ptr(), dlogits.data_ptr()
    p.gscale, p.accumulate, p.gscale_dev = gscale, int(accumulate), _p(gscale_dev)
    p.N, p.C, p.P, p.smooth, p.k_dice, p.k_ce = N, Cc, logits[0, 0].numel(), smooth, k_dice, k_ce
    L.call("chap_mix_loss_bwd", p, _stream())


LOSS_CLASSES = range(2, 9)              # class counts the loss, pseudo-label and VAT-distance kernels are built for (csrc/loss.hip)
MIX_LOSS_MULTI_CLASSES = (2, 4)         # ... and the batched multi-term launch: the two benchmarked counts


def _fill_mix_loss(p, logits, target_a, target_b, mask, w_a, w_b, acc, smooth, k_dice, k_ce):
    p.logits, p.target_a, p.target_b, p.mask = logits.data_ptr(), target_a.data_ptr(), _p(target_b), _p(mask)
    p.w_a, p.w_b, p.acc = w_a, w_b, acc.data_ptr()
    p.N, p.C, p.P, p.smooth, p.k_dice, p.k_ce = logits.shape[0], logits.shape[1], logits[0, 0].numel(), smooth, k_dice, k_ce


def mix_loss_multi_fwd(terms):
    """Up to four mix_loss_fwd calls as one launch per kernel.  terms: dicts of mix_loss_fwd's arguments (logits, target_a, target_b, mask,
    w_a, w_b and optionally smooth, k_dice, k_ce); the class count and the spatial size are common.  Returns [(loss[3], acc)] in the
    order of the terms, bit for bit what the single-term calls return."""
    m = L.MixLossMultiParams()
    m.nterms = len(terms)
    if not 1 <= len(terms) <= 4:
        raise ValueError("mix_loss_multi_fwd: %d terms (1..4)" % len(terms))
    res = []
    for p, t in zip(m.term, terms):
        lg = t["logits"]
        acc = L.hold_empty((1 + L.LOSS_SLOTS) * 2 * (2 + 3 * lg.shape[1]), dtype=torch.float32, device=lg.device)
        loss = L.hold_empty(3, dtype=torch.float32, device=lg.device)
        _fill_mix_loss(p, lg, t["target_a"], t.get("target_b"), t.get("mask"), t["w_a"], t["w_b"], acc, t.get("smooth", 1e-10), t.get("k_dice", 0.0), t.get("k_ce", 0.0))
        p.loss = loss.data_ptr()
        res.append((loss, acc))
    L.call("chap_mix_loss_multi_fwd", m, _stream())
    return res


def mix_loss_multi_bwd(terms):
    """Up to four mix_loss_bwd calls as one launch.  terms: dicts of mix_loss_bwd's arguments (logits, target_a, target_b, mask, w_a, w_b,
    acc, dlogits and optionally gscale, accumulate, smooth, k_dice, k_ce, gscale_dev)."""
    m = L.MixLossMultiParams()
    m.nterms = len(terms)
    if not 1 <= len(terms) <= 4:
        raise ValueError("mix_loss_multi_bwd: %d terms (1..4)" % len(terms))
    for p, t in zip(m.term, terms):
        _fill_mix_loss(p, t["logits"], t["target_a"], t.get("target_b"), t.get("mask"), t["w_a"], t["w_b"], t["acc"], t.get("smooth", 1e-10),
                       t.get("k_dice", 0.0), t.get("k_ce", 0.0))
        p.dlogits, p.gscale, p.accumulate, p.gscale_dev = t["dlogits"].data_ptr(), t.get("gscale", 1.0), int(t.get("accumulate", False)), _p(t.get("gscale_dev"))
    L.call("chap_mix_loss_multi_bwd", m, _stream())


def pseudo_block(logits1, logits2, want_soft=True):
    N, Cc = logits1.shape[0], logits1.shape[1]
    sp = logits1.shape[2:]
    dev = logits1.device
    soft1 = L.hold_empty_like(logits1) if want_soft else None
    soft2 = L.hold_empty_like(logits2) if want_soft else None
    arg = L.hold_empty((2 * N,) + tuple(sp), dtype=torch.int64, device=dev)       # both heads' arg-max maps, stacked: one largest_cc call takes the pair (_stacked_pair)
    arg1, arg2 = arg[:N], arg[N:]
    know = L.hold_empty((N,) + tuple(sp), dtype=torch.float32, device=dev)
    p = L.PseudoParams()
    p.logits1, p.logits2, p.soft1, p.soft2 = logits1.data_ptr(), logits2.data_ptr(), _p(soft1), _p(soft2)
    p.arg1, p.arg2, p.knowledge = arg1.data_ptr(), arg2.data_ptr(), know.data_ptr()
    p.N, p.C, p.P = N, Cc, logits1[0, 0].numel()
    L.call("chap_pseudo_block", p, _stream())
    return soft1, soft2, arg1, arg2, know


DIST_MODES = {"kl": 0, "dice": 1}


def kl_fwd_bwd(logits, targets, loss, dlogits=(None, None), gscale=1.0, gscale_dev=None, mode="kl"):
    """loss (1-elem fp32 tensor) += the VAT distance between softmax(logits) and targets, summed over the two heads:
    'kl' = mean_{n,p} KL(target || softmax(logits)), 'dice' = mean_c soft Dice (chap_hip.h, chap_kl_params)."""
    p = L.KlParams()
    p.mode = DIST_MODES[mode]
    Cc = logits[0].shape[1]
    if loss is not None or p.mode == 1:
        ws = L.hold_empty((1 + L.LOSS_SLOTS) * 2 * (3 * Cc + 1), dtype=torch.float32, device=logits[0].device)
        p.ws = ws.data_ptr()
    for h in range(2):
        p.logits[h], p.target[h], p.dlogits[h] = logits[h].data_ptr(), targets[h].data_ptr(), _p(dlogits[h])
    p.loss, p.gscale, p.gscale_dev = _p(loss), gscale, _p(gscale_dev)
    p.N, p.C, p.P = logits[0].shape[0], logits[0].shape[1], logits[0][0, 0].numel()
    L.call("chap_kl_fwd_bwd", p, _stream())


def teacher_consistency_ws_words():
    return (1 + L.LOSS_SLOTS) * 2


def teacher_consistency(logits, teacher, loss, dlogits=(None, None), gscale=1.0, gscale_dev=None, accumulate=False, ws=None):
    """loss (1-elem fp32 tensor) = sum over the student's two heads of mean_{n,c,p} (softmax(logits[h]) - q)^2 with q the mean of the teacher's
    two softmax outputs; dlogits[h] (or None) = gscale * (*gscale_dev) * d loss / d logits[h], added to what it holds with `accumulate`
    (include/chap_hip_teacher.h).  `ws`: [1 + LOSS_SLOTS][2] fp32 per-block partials, allocated here when not given."""
    p = L.TeacherConsistencyParams()
    shape = logits[0].shape
    for t in (logits[0], logits[1], teacher[0], teacher[1], dlogits[0], dlogits[1]):
        if t is not None and (t.shape != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("chap_amd teacher_consistency: every tensor must be contiguous fp32 of shape %s, got %s %s" % (tuple(shape), t.dtype, tuple(t.shape)))
    if ws is None:
        ws = L.hold_empty(teacher_consistency_ws_words(), dtype=torch.float32, device=logits[0].device)
    elif ws.numel() < teacher_consistency_ws_words() or ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("chap_amd teacher_consistency: ws must hold %d contiguous fp32 words" % teacher_consistency_ws_words())
    for h in range(2):
        p.logits[h], p.teacher[h], p.dlogits[h] = logits[h].data_ptr(), teacher[h].data_ptr(), _p(dlogits[h])
    p.loss, p.ws, p.gscale, p.gscale_dev, p.accumulate = loss.data_ptr(), ws.data_ptr(), gscale, _p(gscale_dev), int(bool(accumulate))
    p.N, p.C, p.P = shape[0], shape[1], logits[0][0, 0].numel() if shape[0] > 0 else 0
    L.call("chap_teacher_consistency", p, _stream())


def teacher_uncertainty_ws_words():
    return 1 + L.LOSS_SLOTS


def teacher_uncertainty(passes, threshold=0.0, threshold_dev=None, want_entropy=False, ws=None):
    """`passes`: T = 1..8 pairs (head 1, head 2) of teacher logits [N][C][...].  -> (mask uint8 [N][...], count int64 [1][, entropy fp32 [N][...]]):
    mask = entropy of the mean of the 2T softmax outputs < threshold (`threshold_dev`, a 1-elem fp32 tensor, replaces the host value), count
    its exact sum (include/chap_hip_uncertainty.h).  `ws`: [1 + LOSS_SLOTS] int64 per-block partials, allocated here when not given."""
    p = L.TeacherUncertaintyParams()
    T = len(passes)
    if not 1 <= T <= L.UNCERTAINTY_MAX_T:
        raise ValueError("chap_amd teacher_uncertainty: %d passes, need 1..%d" % (T, L.UNCERTAINTY_MAX_T))
    shape = passes[0][0].shape
    for k, pair in enumerate(passes):
        if len(pair) != 2:
            raise ValueError("chap_amd teacher_uncertainty: pass %d has %d heads, need 2" % (k, len(pair)))
        for h, t in enumerate(pair):
            if t.shape != shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("chap_amd teacher_uncertainty: every tensor must be contiguous fp32 of shape %s, got %s %s" % (tuple(shape), t.dtype, tuple(t.shape)))
            p.teacher[k][h] = t.data_ptr()
    if threshold_dev is not None and (threshold_dev.dtype != torch.float32 or threshold_dev.numel() != 1):
        raise ValueError("chap_amd teacher_uncertainty: threshold_dev must be one fp32 word")
    dev = passes[0][0].device
    if ws is None:
        ws = L.hold_empty(teacher_uncertainty_ws_words(), dtype=torch.int64, device=dev)
    elif ws.numel() < teacher_uncertainty_ws_words() or ws.dtype != torch.int64 or not ws.is_contiguous():
        raise ValueError("chap_amd teacher_uncertainty: ws must hold %d contiguous int64 words" % teacher_uncertainty_ws_words())
    sp = (shape[0],) + tuple(shape[2:])
    mask = torch.empty(sp, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    entropy = torch.empty(sp, dtype=torch.float32, device=dev) if want_entropy else None
    p.mask, p.entropy, p.count, p.ws = mask.data_ptr(), _p(entropy), count.data_ptr(), ws.data_ptr()
    p.threshold, p.threshold_dev, p.T = float(threshold), _p(threshold_dev), T
    p.N, p.C, p.P = shape[0], shape[1], passes[0][0][0, 0].numel() if shape[0] > 0 else 0
    L.call("chap_teacher_uncertainty", p, _stream())
    return (mask, count, entropy) if want_entropy else (mask, count)


def teacher_consistency_masked(logits, teacher, mask, count, loss, dlogits=(None, None), gscale=1.0, gscale_dev=None, accumulate=False, ws=None):
    """teacher_consistency counted over the pixels with mask = 1 only and normalised by C * count (`count`: a 1-elem int64 device tensor, the
    number of ones in `mask`): loss = sum_h sum m e_h^2 / (C count + 1e-16); where mask = 0 the gradient is exactly 0 -- with `accumulate` the
    element keeps what it holds (include/chap_hip_uncertainty.h).  `ws`: [1 + LOSS_SLOTS][2] fp32, allocated here when not given."""
    p = L.TeacherConsistencyMaskedParams()
    shape = logits[0].shape
    for t in (logits[0], logits[1], teacher[0], teacher[1], dlogits[0], dlogits[1]):
        if t is not None and (t.shape != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("chap_amd teacher_consistency_masked: every tensor must be contiguous fp32 of shape %s, got %s %s" % (tuple(shape), t.dtype, tuple(t.shape)))
    if mask.dtype != torch.uint8 or not mask.is_contiguous() or tuple(mask.shape) != (shape[0],) + tuple(shape[2:]):
        raise ValueError("chap_amd teacher_consistency_masked: mask must be contiguous uint8 of shape %s, got %s %s" % ((shape[0],) + tuple(shape[2:]), mask.dtype, tuple(mask.shape)))
    if count.dtype != torch.int64 or count.numel() != 1:
        raise ValueError("chap_amd teacher_consistency_masked: count must be one int64 word")
    if ws is None:
        ws = L.hold_empty(teacher_consistency_ws_words(), dtype=torch.float32, device=logits[0].device)
    elif ws.numel() < teacher_consistency_ws_words() or ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("chap_amd teacher_consistency_masked: ws must hold %d contiguous fp32 words" % teacher_consistency_ws_words())
    for h in range(2):
        p.logits[h], p.teacher[h], p.dlogits[h] = logits[h].data_ptr(), teacher[h].data_ptr(), _p(dlogits[h])
    p.mask, p.count = mask.data_ptr(), count.data_ptr()
    p.loss, p.ws, p.gscale, p.gscale_dev, p.accumulate = loss.data_ptr(), ws.data_ptr(), gscale, _p(gscale_dev), int(bool(accumulate))
    p.N, p.C, p.P = shape[0], shape[1], logits[0][0, 0].numel() if shape[0] > 0 else 0
    L.call("chap_teacher_consistency_masked", p, _stream())


def l2_normalize(x, out, eps=1e-8):
    p = L.L2NormParams()
    ws = L.hold_empty(x.shape[0] * L.L2NORM_SLOTS, dtype=torch.float32, device=x.device)
    p.in_, p.out, p.N, p.P, p.eps, p.ws = x.data_ptr(), out.data_ptr(), x.shape[0], x[0].numel(), eps, ws.data_ptr()
    L.call("chap_l2_normalize", p, _stream())


def perturb(x, d, out, alpha, mask=None, sign=False):
    p = L.AxpyParams()
    p.x, p.d, p.mask, p.out = x.data_ptr(), d.data_ptr(), _p(mask), out.data_ptr()
    p.alpha, p.sign, p.n = alpha, int(sign), x.numel()
    L.call("chap_perturb", p, _stream())


def rand_uniform(out, seed, lo=0.0, hi=1.0, seed_dev=None):
    p = L.RandParams()
    p.out, p.seed, p.seed_dev, p.n, p.lo, p.hi = out.data_ptr(), seed, _p(seed_dev), out.numel(), lo, hi
    L.call("chap_rand_uniform", p, _stream())


def keep_mask(keep, seed, prob, seed_dev=None):
    p = L.KeepMaskParams()
    p.keep, p.seed, p.seed_dev, p.n, p.p = keep.data_ptr(), seed, _p(seed_dev), keep.numel(), prob
    L.call("chap_keep_mask", p, _stream())


def chan_mask(mul, seed, prob, seed_dev=None):
    p = L.ChanMaskParams()
    p.mul, p.seed, p.seed_dev, p.n, p.p = mul.data_ptr(), seed, _p(seed_dev), mul.numel(), prob
    L.call("chap_chan_mask", p, _stream())


DROP_MODES = {"dropout2d": 0, "comp_binomial": 1, "scores": 2}


def sample_channel_sum(lazy, nchunk=32):
    """Per-sample spatial sums of a lazy activation [N, ..., C] as partial sums fp32 [N, nchunk, C] (fixed order)."""
    p = L.SampleChanSumParams()
    lazy.fill(p.r)
    N = lazy.raw.shape[0]
    partial = L.hold_empty(N, nchunk, lazy.C, dtype=torch.float32, device=lazy.raw.device)
    p.partial, p.N, p.nchunk, p.pix_per_sample, p.dtype = partial.data_ptr(), N, nchunk, lazy.raw[0, ..., 0].numel(), dt(lazy.raw)
    L.call("chap_sample_channel_sum", p, _stream())
    return partial


def channel_drop(mul1, mul2, u1, u2, B, mode, *, pool_partial=None, npix=1, grad_sim=None, comp=False, branch=0,
                 prob_kind="sigmoid", probs_out=None):
    """FilterDropout.perform_dropout's two channel masks of one level, as the chan_mul rows of the (B + U) decoder
    batch: mul1/mul2 fp32 [B + U, C]; u1/u2 fp32 [U, C] uniforms."""
    p = L.ChannelDropParams()
    U, Cc = u1.shape
    assert tuple(mul1.shape) == (B + U, Cc) and tuple(mul2.shape) == (B + U, Cc) and tuple(u2.shape) == (U, Cc)
    p.pool_partial, p.grad_sim, p.u1, p.u2 = _p(pool_partial), _p(grad_sim), u1.data_ptr(), u2.data_ptr()
    p.mul1, p.mul2, p.probs_out = mul1.data_ptr(), mul2.data_ptr(), _p(probs_out)
    p.inv_npix, p.nchunk = 1.0 / npix, (pool_partial.shape[1] if pool_partial is not None else 0)
    p.B, p.U, p.C, p.mode, p.comp, p.branch = B, U, Cc, DROP_MODES[mode], int(bool(comp)), int(branch)
    p.prob_kind = {"sigmoid": 0, "gauss": 1}[prob_kind]
    L.call("chap_channel_drop", p, _stream())


def fold_perturbed(g, coff, Cc, mul, B, U):
    """Adjoint of cat((feat, mul * feat[B-U:])): g [B + U, ..., ld] (channels [coff, coff + Cc)) -> [B, ..., Cc]."""
    p = L.FoldParams()
    out = L.hold_empty((B,) + tuple(g.shape[1:-1]) + (Cc,), dtype=g.dtype, device=g.device)
    p.g, p.mul, p.out = g.data_ptr(), _p(mul), out.data_ptr()
    p.B, p.U, p.C, p.ld, p.coff = B, U, Cc, g.shape[-1], coff
    p.pix_per_sample, p.dtype = g[0, ..., 0].numel(), dt(g)
    L.call("chap_fold_perturbed", p, _stream())
    return out


def box_mix(a, b, out, box):
    """out = inside box ? b : a ; a/b/out [N, (1,) H, W] float32 or int64; box: device int32[4]."""
    p = L.BoxMixParams()
    p.a, p.b, p.out, p.box = a.data_ptr(), b.data_ptr(), out.data_ptr(), box.data_ptr()
    p.N, p.H, p.W, p.is_i64 = a.shape[0], a.shape[-2], a.shape[-1], int(a.dtype == torch.int64)
    p.D = a.shape[-3] if box.numel() == 6 else 1
    L.call("chap_box_mix", p, _stream())


def bcp_mix(a0, b0, out0, a1, b1, out1, mask, box):
    """box_mask(mask, box), box_mix(a0, b0, out0, box) and box_mix(a1, b1, out1, box) (fp32 images) as one launch."""
    p = L.BcpMixParams()
    for h, (a, b, o) in enumerate(((a0, b0, out0), (a1, b1, out1))):
        assert a.dtype == b.dtype == o.dtype == torch.float32 and a.shape == b.shape == o.shape and a.shape[-2:] == mask.shape[-2:]
        p.a[h], p.b[h], p.out[h], p.N[h] = a.data_ptr(), b.data_ptr(), o.data_ptr(), a.shape[0]
    p.mask, p.box, p.Nm, p.H, p.W = mask.data_ptr(), box.data_ptr(), mask.shape[0], mask.shape[-2], mask.shape[-1]
    p.D = mask.shape[-3] if box.numel() == 6 else 1
    L.call("chap_bcp_mix", p, _stream())


def _stacked_pair(a, b):
    """The [2N, ...] tensor that a and b are the two halves of (as pseudo_block returns its arg-max maps), or None."""
    base = a._base
    if base is None or b._base is not base or not base.is_contiguous() or base.shape[0] != 2 * a.shape[0] or base.shape[1:] != a.shape[1:]:
        return None
    n = a.numel() * a.element_size()
    return base if (a.shape == b.shape and a.data_ptr() == base.data_ptr() and b.data_ptr() == base.data_ptr() + n) else None


def box_mask(mask, box):
    p = L.BoxMaskParams()
    p.mask, p.box, p.N, p.H, p.W = mask.data_ptr(), box.data_ptr(), mask.shape[0], mask.shape[-2], mask.shape[-1]
    p.D = mask.shape[-3] if box.numel() == 6 else 1
    L.call("chap_box_mask", p, _stream())


def largest_cc(labels, num_classes):
    """labels int64 [N, H, W] (8-connectivity) or [N, D, H, W] (26-connectivity) -> same shape, keeping the
    largest connected component per (sample, class > 0)."""
    out = L.hold_empty_like(labels)
    p = L.LccParams()
    p.labels, p.out = labels.data_ptr(), out.data_ptr()
    p.N, p.H, p.W, p.num_classes = labels.shape[0], labels.shape[-2], labels.shape[-1], num_classes
    p.D = labels.shape[1] if labels.dim() == 4 else 1
    ws = L.hold_empty(L.size_of("chap_lcc_ws", p), dtype=torch.uint8, device=labels.device)
    p.ws = ws.data_ptr()
    L.call("chap_largest_cc", p, _stream())
    return out


def diff_mask(p1, p2, knowledge, scale, topk):
    """[N, H, W] maps (3D volumes are passed as [N, D*H, W]: in-plane scale x scale patches).  The count of selected cells is the
    definition's k = max(int(topk * M), 1), in Python's double arithmetic as oracle.train_step.create_mask_v1 computes it."""
    if knowledge.dim() == 4:
        n, d, h, w = knowledge.shape
        return diff_mask(p1.reshape(n, d * h, w), p2.reshape(n, d * h, w), knowledge.reshape(n, d * h, w), scale, topk).reshape(n, d, h, w)
    N, H, W = knowledge.shape
    out = L.hold_empty(N, H, W, dtype=torch.float32, device=knowledge.device)
    ws = L.hold_empty(N * (H // scale) * (W // scale) + N, dtype=torch.float32, device=knowledge.device)
    p = L.DiffMaskParams()
    p.p1, p.p2, p.knowledge, p.out, p.pooled_ws = p1.data_ptr(), p2.data_ptr(), knowledge.data_ptr(), out.data_ptr(), ws.data_ptr()
    p.N, p.H, p.W, p.scale, p.k = N, H, W, scale, max(int(topk * ((H // scale) * (W // scale))), 1)
    L.call("chap_diff_mask", p, _stream())
    return out


def grad_sim(gl, gu, score, ema=0.0):
    """score[c] = ema * score[c] + (1 - ema) * cos(gl[c, :], gu[c, :]) for the rows (output channels) of a conv kernel's two
    gradients gl, gu [Cout, Cin, k, k] (contiguous fp32 views)."""
    p = L.GradSimParams()
    p.gl, p.gu, p.score = gl.data_ptr(), gu.data_ptr(), score.data_ptr()
    p.C, p.K, p.ema = gl.shape[0], gl[0].numel(), ema
    L.call("chap_grad_sim", p, _stream())


def sgd_step(param, grad, mom, lr_dev, momentum, weight_decay, grad_scale=1.0, zero_grad=True, grad2=None):
    p = L.SgdParams()
    p.param, p.grad, p.grad2, p.mom, p.lr = param.data_ptr(), grad.data_ptr(), _p(grad2), mom.data_ptr(), lr_dev.data_ptr()
    p.momentum, p.weight_decay, p.grad_scale, p.n, p.zero_grad = momentum, weight_decay, grad_scale, param.numel(), int(zero_grad)
    L.call("chap_sgd_step", p, _stream())


def sgd_ema_step(param, grad, mom, lr_dev, momentum, weight_decay, ema, coef_dev, grad_scale=1.0, zero_grad=True, grad2=None):
    """sgd_step and, in the same pass, ema = coef_dev[0] * ema + coef_dev[1] * (the parameter just written): the mean-teacher average
    (update_ema_variables, train_ours_2D.py:50-54).  param / mom / grad / grad2 get bit for bit what sgd_step writes."""
    q = L.SgdEmaParams()
    p = q.sgd
    p.param, p.grad, p.grad2, p.mom, p.lr = param.data_ptr(), grad.data_ptr(), _p(grad2), mom.data_ptr(), lr_dev.data_ptr()
    p.momentum, p.weight_decay, p.grad_scale, p.n, p.zero_grad = momentum, weight_decay, grad_scale, param.numel(), int(zero_grad)
    q.ema, q.coef = _p(ema), _p(coef_dev)
    L.call("chap_sgd_ema_step", q, _stream())


# ------------------------------------------------------------------------------------------
# gradient guard (include/chap_hip_guard.h; chap_amd.guard.StepGuard owns the workspace and the state block)
def guard_state_words(ring):
    """int32 words of a state block with `ring` rows: CHAP_GUARD_STATE_BYTES(ring) / 4."""
    import ctypes
    return (ctypes.sizeof(L.GuardState) + int(ring) * ctypes.sizeof(L.GuardRow)) // 4


def grad_norm(grad, grad2, ws, state, ring, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True):
    """norm = sqrt(sum (grad + grad2)^2) * grad_scale in a fixed order (fp64), and from it the clip coefficient min(1, max_norm / (norm + 1e-6))
    (max_norm <= 0: 1) and the skip flag (a non-finite element and `skip_nonfinite`) into `state`: an int32 tensor of guard_state_words(ring)
    words whose three counters and ring row the launch advances itself.  `ws`: L.GRADNORM_SLOTS fp64 words."""
    if ws.dtype != torch.float64 or ws.numel() < L.GRADNORM_SLOTS or state.dtype != torch.int32 or state.numel() < guard_state_words(ring):
        raise ValueError("grad_norm: ws must hold %d fp64 words and state %d int32 words" % (L.GRADNORM_SLOTS, guard_state_words(ring)))
    p = L.GradNormParams()
    p.grad, p.grad2, p.n, p.grad_scale, p.max_norm = grad.data_ptr(), _p(grad2), grad.numel(), grad_scale, max_norm
    p.skip_nonfinite, p.ring, p.ws, p.state = int(bool(skip_nonfinite)), int(ring), ws.data_ptr(), state.data_ptr()
    L.call("chap_grad_norm", p, _stream())


def sgd_guard_step(param, grad, mom, lr_dev, momentum, weight_decay, state, ema=None, coef_dev=None, grad_scale=1.0, zero_grad=True, grad2=None):
    """sgd_step (ema None) or sgd_ema_step with the gradient scaled by fl32(grad_scale * state.scale), and nothing but the zeroing of the
    buckets when state.skip is set; `state` as grad_norm left it."""
    q = L.SgdGuardParams()
    p = q.se.sgd
    p.param, p.grad, p.grad2, p.mom, p.lr = param.data_ptr(), grad.data_ptr(), _p(grad2), mom.data_ptr(), lr_dev.data_ptr()
    p.momentum, p.weight_decay, p.grad_scale, p.n, p.zero_grad = momentum, weight_decay, grad_scale, param.numel(), int(zero_grad)
    q.se.ema, q.se.coef, q.state = _p(ema), _p(coef_dev), _p(state)
    L.call("chap_sgd_guard_step", q, _stream())


# ------------------------------------------------------------------------------------------
# Adam / AdamW (include/chap_hip_optim.h; chap_amd.train.FusedAdamW owns the moments and the state block)
ADAM_STATE_WORDS = 4                    # chap_adam_state: step | step_size | bc2_sqrt | decay


def _adam_state_check(who, state, guard_state, dev):
    if state.dtype != torch.int32 or state.numel() < ADAM_STATE_WORDS or state.device != dev or not state.is_contiguous():
        raise ValueError("%s: state must be a contiguous int32 tensor of %d words on %s, got %s [%d] on %s"
                         % (who, ADAM_STATE_WORDS, dev, state.dtype, state.numel(), state.device))
    if guard_state is not None and (guard_state.dtype != torch.int32 or guard_state.numel() < guard_state_words(0) or guard_state.device != dev
                                    or not guard_state.is_contiguous()):
        raise ValueError("%s: guard_state must hold %d contiguous int32 words on %s" % (who, guard_state_words(0), dev))


def adam_tick(state, lr_dev, beta1, beta2, weight_decay, decoupled, guard_state=None):
    """Once per optimizer step, before adam_step: t = state[0] + 1 and, in fp64 and rounded once each, step_size = lr / (1 - beta1^t),
    bc2_sqrt = sqrt(1 - beta2^t), decay = 1 - lr * weight_decay (`decoupled`) or 1, into `state`: an int32 tensor of ADAM_STATE_WORDS words.
    With a `guard_state` (as grad_norm left it) whose skip flag is set nothing is written: a skipped step does not count."""
    if lr_dev.dtype != torch.float32 or lr_dev.numel() < 1 or lr_dev.device != state.device:
        raise ValueError("adam_tick: lr_dev must be an fp32 word on %s, got %s [%d] on %s" % (state.device, lr_dev.dtype, lr_dev.numel(), lr_dev.device))
    _adam_state_check("adam_tick", state, guard_state, state.device)
    p = L.AdamTickParams()
    p.state, p.lr, p.guard = state.data_ptr(), lr_dev.data_ptr(), _p(guard_state)
    p.beta1, p.beta2, p.weight_decay, p.decoupled = beta1, beta2, weight_decay, int(bool(decoupled))
    L.call("chap_adam_tick", p, _stream())


def adam_step(param, grad, exp_avg, exp_avg_sq, state, beta1, beta2, eps, weight_decay, decoupled, ema=None, coef_dev=None, guard_state=None,
              grad_scale=1.0, zero_grad=True, grad2=None):
    """One Adam (`decoupled` false: L2 weight decay, torch.optim.Adam) or AdamW (true) update of the flat fp32 buffers with the step size and
    bias correction adam_tick left in `state`; the gradient is (grad + grad2) * fl32(grad_scale * guard_state.scale).  With `ema`, the same pass
    averages the new parameters into it (coef_dev: two device words a, b).  A set skip flag in `guard_state`: nothing but the zeroing of the
    buckets."""
    n, dev = param.numel(), param.device
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("grad2", grad2), ("ema", ema)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != n or t.device != dev or not t.is_contiguous()):
            raise ValueError("adam_step: %s must be a contiguous fp32 tensor of %d elements on %s, got %s [%d] on %s"
                             % (name, n, dev, t.dtype, t.numel(), t.device))
    _adam_state_check("adam_step", state, guard_state, dev)
    if coef_dev is not None and (coef_dev.dtype != torch.float32 or coef_dev.numel() < 2 or coef_dev.device != dev):
        raise ValueError("adam_step: coef_dev must hold two fp32 words on %s" % (dev,))
    q = L.AdamParams()
    q.param, q.grad, q.grad2, q.exp_avg, q.exp_avg_sq = param.data_ptr(), grad.data_ptr(), _p(grad2), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    q.state, q.guard, q.ema, q.coef = state.data_ptr(), _p(guard_state), _p(ema), _p(coef_dev)
    q.beta1, q.beta2, q.eps, q.weight_decay = beta1, beta2, eps, weight_decay
    q.decoupled, q.grad_scale, q.zero_grad, q.n = int(bool(decoupled)), grad_scale, int(bool(zero_grad)), n
    L.call("chap_adam_step", q, _stream())


# ------------------------------------------------------------------------------------------
# training monitor (include/chap_hip_monitor.h; chap_amd.monitor.StepMonitor owns the workspace and the ring)
def monitor_group_words(C):
    return 8 + 5 * C                    # CHAP_MONITOR_GROUP_WORDS


def monitor_label_words(C):
    return 4 * C                        # CHAP_MONITOR_LABEL_WORDS


def monitor_row_words(C):
    return 1 + 2 * monitor_group_words(C) + 2 * monitor_label_words(C) + L.MONITOR_MAX_SCALARS       # CHAP_MONITOR_ROW_WORDS


def monitor_label_region(C):
    return L.MONITOR_HDR + 2 * L.MONITOR_SLOTS * monitor_group_words(C)      # CHAP_MONITOR_LABEL_REGION


def monitor_ws_words(C):
    return monitor_label_region(C) + L.MONITOR_HDR + 2 * L.MONITOR_SLOTS * monitor_label_words(C)     # CHAP_MONITOR_WS_WORDS


def monitor_accumulate(logits1, logits2, labels, ws, n_first):
    """Counts of acc_conf_analysis (train_ours_2D.py:152-193) for two heads' fp32 planar logits [N, C, *sp] against int64 labels [N, *sp]:
    one partial row per block into the logits region of `ws` (int64 / fp64 words).  Samples [0, n_first) are group 0, the rest group 1."""
    p = L.MonitorParams()
    p.logits[0], p.logits[1], p.labels, p.ws = logits1.data_ptr(), logits2.data_ptr(), labels.data_ptr(), ws.data_ptr()
    p.N, p.C, p.P, p.n_first = logits1.shape[0], logits1.shape[1], logits1[0, 0].numel(), n_first
    L.call("chap_monitor_accumulate", p, _stream())


def monitor_accumulate_labels(map1, map2, labels, ws, n_first, num_classes):
    """The Dice terms (inter_f, pred_f) of two int64 label maps [N, *sp] against `labels`, into the label-map region of `ws`."""
    p = L.MonitorLabelsParams()
    p.maps[0], p.maps[1], p.labels, p.ws = map1.data_ptr(), map2.data_ptr(), labels.data_ptr(), ws.data_ptr()
    p.N, p.C, p.P, p.n_first = map1.shape[0], num_classes, map1[0].numel(), n_first
    L.call("chap_monitor_accumulate_labels", p, _stream())


def monitor_finalize(ws, ring, slot_iter, num_classes, scalars=(), has_labels=True):
    """Fixed-order totals of the partial rows -> row slot_iter[0] % len(ring) of `ring` (fp64 [R, monitor_row_words(C)]), stamped with the
    iteration slot_iter[1]; `scalars`: up to 16 one-element fp32 device tensors (or views) copied into the row."""
    p = L.MonitorFinalizeParams()
    p.ws, p.ring, p.slot_iter = ws.data_ptr(), ring.data_ptr(), slot_iter.data_ptr()
    if len(scalars) > L.MONITOR_MAX_SCALARS:
        raise ValueError("monitor_finalize: %d scalars (at most %d)" % (len(scalars), L.MONITOR_MAX_SCALARS))
    for k, t in enumerate(scalars):
        p.scalars[k] = t.data_ptr()
    p.C, p.ring_rows, p.nscalars, p.has_labels = num_classes, ring.shape[0], len(scalars), int(has_labels)
    L.call("chap_monitor_finalize", p, _stream())


# ------------------------------------------------------------------------------------------
# inference callers (val_2D.py:54-97, test_3D_util.py:14-79)
ENSEMBLE_MODES = {"model1": 0, "model2": 1, "logit_ensemble": 2, "prob_ensemble": 3}


def ensemble_argmax(logits1, logits2, mode, want_prob=False):
    """logits*: fp32 [N, C, *spatial] (planar).  Returns (label uint8 [N, *spatial], prob or None)."""
    ref = logits1 if logits1 is not None else logits2
    N, Cc = ref.shape[0], ref.shape[1]
    p = L.EnsembleParams()
    label = L.hold_empty((N,) + tuple(ref.shape[2:]), dtype=torch.uint8, device=ref.device)
    prob = L.hold_empty_like(ref) if want_prob else None
    p.logits1, p.logits2, p.prob, p.label = _p(logits1), _p(logits2), _p(prob), label.data_ptr()
    p.N, p.C, p.P, p.mode = N, Cc, ref[0, 0].numel(), ENSEMBLE_MODES[mode] if isinstance(mode, str) else mode
    L.call("chap_ensemble_argmax", p, _stream())
    return label, prob


def window_accumulate(logits, origins, score, cnt):
    """logits fp32 [K, C, pw, ph, pd]; origins int32 [K, 3]; score fp32 [C, W, H, D]; cnt fp32 [W, H, D] (both += )."""
    p = L.WindowAccParams()
    p.logits, p.origins, p.score, p.cnt = logits.data_ptr(), origins.data_ptr(), score.data_ptr(), cnt.data_ptr()
    p.npatch, p.C = logits.shape[0], logits.shape[1]
    p.pw, p.ph, p.pd = logits.shape[2:]
    p.W, p.H, p.D = cnt.shape
    L.call("chap_window_accumulate", p, _stream())


def window_gather(volume, origins, patch_size, pad_lo=(0, 0, 0), out=None):
    """chap_window_gather: volume fp32 [W, H, D] (unpadded); origins int32 device [K, 3] in padded coordinates; returns (or fills
    `out`) patches fp32 [K, 1, pw, ph, pd], zero where a patch reaches into the padding."""
    K = origins.shape[0]
    pw, ph, pd = (int(v) for v in patch_size)
    assert volume.dtype == torch.float32 and volume.dim() == 3 and volume.is_contiguous()
    assert origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 3 and origins.is_contiguous()
    if out is None:
        out = L.hold_empty((K, 1, pw, ph, pd), dtype=torch.float32, device=volume.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (K, 1, pw, ph, pd)
    p = L.WindowGatherParams()
    p.volume, p.origins, p.patches, p.npatch = volume.data_ptr(), origins.data_ptr(), out.data_ptr(), K
    p.W, p.H, p.D = volume.shape
    p.pad_lo[0], p.pad_lo[1], p.pad_lo[2] = (int(v) for v in pad_lo)
    p.pw, p.ph, p.pd = pw, ph, pd
    L.call("chap_window_gather", p, _stream())
    return out


def window_accumulate_heads(logits, origins, score, cnt):
    """chap_window_accumulate_heads: `logits` a tensor or a list of one or two fp32 [K, C, pw, ph, pd] tensors (the heads of one batch
    of patches); two heads add the mean of their soft-maxes; otherwise as window_accumulate."""
    heads = [logits] if isinstance(logits, torch.Tensor) else list(logits)
    if len(heads) not in (1, 2) or any(h.shape != heads[0].shape or h.dtype != torch.float32 or not h.is_contiguous() for h in heads):
        raise ValueError("window_accumulate_heads: one or two contiguous fp32 logits tensors of one shape")
    K, Cc = heads[0].shape[0], heads[0].shape[1]
    dev = heads[0].device
    assert origins.dtype == torch.int32 and tuple(origins.shape) == (K, 3) and origins.is_contiguous() and origins.device == dev
    assert cnt.dtype == torch.float32 and cnt.dim() == 3 and cnt.is_contiguous() and cnt.device == dev
    assert score.dtype == torch.float32 and tuple(score.shape) == (Cc,) + tuple(cnt.shape) and score.is_contiguous() and score.device == dev
    assert all(t.device == dev for t in heads)
    p = L.WindowAccHeadsParams()
    for h, t in enumerate(heads):
        p.logits[h] = t.data_ptr()
    p.origins, p.score, p.cnt = origins.data_ptr(), score.data_ptr(), cnt.data_ptr()
    p.nheads, p.npatch, p.C = len(heads), heads[0].shape[0], heads[0].shape[1]
    p.pw, p.ph, p.pd = heads[0].shape[2:]
    p.W, p.H, p.D = cnt.shape
    L.call("chap_window_accumulate_heads", p, _stream())


def window_finalize(score, cnt):
    """score /= cnt in place; returns label uint8 [W, H, D] = argmax over classes."""
    p = L.WindowFinParams()
    label = L.hold_empty(cnt.shape, dtype=torch.uint8, device=cnt.device)
    p.score, p.cnt, p.label, p.C, p.P = score.data_ptr(), cnt.data_ptr(), label.data_ptr(), score.shape[0], cnt.numel()
    L.call("chap_window_finalize", p, _stream())
    return label


def metrics(a, b, classes, *, ndim, spacing=(1.0, 1.0, 1.0), binary=False, distances=True):
    """chap_metrics: a, b contiguous uint8 / int64 device tensors of one shape [D, H, W] (ndim 2: D == 1); classes: device int64 [K]
    (None when binary).  spacing: per axis (D, H, W).  Returns (results uint8 [K * sizeof(chap_metric_result)] on the device,
    border_a, border_b uint8 [D, H, W], dist fp64 [K, 2, D, H, W] or None)."""
    D, H, W = a.shape
    K = 1 if binary else classes.numel()
    p = L.MetricsParams()
    p.a, p.b = a.data_ptr(), b.data_ptr()
    p.a_i64, p.b_i64 = int(a.dtype == torch.int64), int(b.dtype == torch.int64)
    p.classes, p.K, p.binary = (None if binary else classes.data_ptr()), K, int(binary)
    p.ndim, p.D, p.H, p.W, p.distances = ndim, D, H, W, int(distances)
    p.spacing[0], p.spacing[1], p.spacing[2] = (float(s) for s in spacing)
    border_a = L.hold_empty((D, H, W), dtype=torch.uint8, device=a.device)
    border_b = L.hold_empty((D, H, W), dtype=torch.uint8, device=a.device)
    results = L.hold_empty(K * L.C.sizeof(L.MetricResult), dtype=torch.uint8, device=a.device)
    p.border_a, p.border_b, p.results = border_a.data_ptr(), border_b.data_ptr(), results.data_ptr()
    dist = None
    if distances:
        dist = L.hold_empty((K, 2, D, H, W), dtype=torch.float64, device=a.device)
        ws = L.hold_empty(L.size_of("chap_metrics_ws", p), dtype=torch.uint8, device=a.device)
        p.dist, p.ws = dist.data_ptr(), ws.data_ptr()
    L.call("chap_metrics", p, _stream())
    return results, border_a, border_b, dist


def augment2d(images, labels, records, image_out, label_out):
    """chap_augment2d: images fp32 / labels uint8 flat device buffers of one store, records a device uint8 buffer holding
    B chap_augment2d_record (chap_amd.data fills and uploads them), image_out fp32 [B, 1, H, W], label_out int64 or uint8 [B, H, W];
    writes both outputs on the current stream."""
    B, _, H, W = image_out.shape
    assert images.dtype == torch.float32 and labels.dtype == torch.uint8 and images.numel() == labels.numel()
    assert image_out.dtype == torch.float32 and image_out.is_contiguous() and label_out.is_contiguous()
    assert label_out.dtype in (torch.int64, torch.uint8) and tuple(label_out.shape) == (B, H, W)
    assert records.numel() * records.element_size() >= B * L.C.sizeof(L.Augment2dRecord)
    p = L.Augment2dParams()
    p.images, p.labels, p.store_elems, p.records = images.data_ptr(), labels.data_ptr(), images.numel(), records.data_ptr()
    p.image_out, p.label_out, p.label_i64 = image_out.data_ptr(), label_out.data_ptr(), int(label_out.dtype == torch.int64)
    p.B, p.H, p.W = B, H, W
    L.call("chap_augment2d", p, _stream())


def augment3d(images, labels, records, image_out, label_out):
    """chap_augment3d: as augment2d for volumes; image_out fp32 [B, 1, P0, P1, P2], label_out int64 or uint8 [B, P0, P1, P2]."""
    B, _, P0, P1, P2 = image_out.shape
    assert images.dtype == torch.float32 and labels.dtype == torch.uint8 and images.numel() == labels.numel()
    assert image_out.dtype == torch.float32 and image_out.is_contiguous() and label_out.is_contiguous()
    assert label_out.dtype in (torch.int64, torch.uint8) and tuple(label_out.shape) == (B, P0, P1, P2)
    assert records.numel() * records.element_size() >= B * L.C.sizeof(L.Augment3dRecord)
    p = L.Augment3dParams()
    p.images, p.labels, p.store_elems, p.records = images.data_ptr(), labels.data_ptr(), images.numel(), records.data_ptr()
    p.image_out, p.label_out, p.label_i64 = image_out.data_ptr(), label_out.data_ptr(), int(label_out.dtype == torch.int64)
    p.B, p.P0, p.P1, p.P2 = B, P0, P1, P2
    L.call("chap_augment3d", p, _stream())


def augment3d_padded(images, labels, records, image_out, label_out):
    """chap_augment3d_padded: augment3d with B chap_augment3d_pad_record (corner in padded coordinates, per-axis zero padding)."""
    B, _, P0, P1, P2 = image_out.shape
    assert images.dtype == torch.float32 and labels.dtype == torch.uint8 and images.numel() == labels.numel()
    assert image_out.dtype == torch.float32 and image_out.is_contiguous() and label_out.is_contiguous()
    assert label_out.dtype in (torch.int64, torch.uint8) and tuple(label_out.shape) == (B, P0, P1, P2)
    assert records.numel() * records.element_size() >= B * L.C.sizeof(L.Augment3dPadRecord)
    p = L.Augment3dPadParams()
    p.images, p.labels, p.store_elems, p.records = images.data_ptr(), labels.data_ptr(), images.numel(), records.data_ptr()
    p.image_out, p.label_out, p.label_i64 = image_out.data_ptr(), label_out.data_ptr(), int(label_out.dtype == torch.int64)
    p.B, p.P0, p.P1, p.P2 = B, P0, P1, P2
    L.call("chap_augment3d_padded", p, _stream())
