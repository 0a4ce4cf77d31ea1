"""Every launch of one training iteration at the bench shapes against fp64 (tests/kernel_ref.py), with the default dispatch: the kernels
the block-count thresholds pick there (wave-private 2D, K-parallel 3D, bricks, the first-conv MFMA kernel, the 1x1x1 head, ...) are the
ones checked.  The step is built as bench.build_step builds it, run eagerly on one stream and ungrouped (concurrent=False,
CHAP_GROUP=0): the stream schedule, grouping and graph replay are asserted bit-identical elsewhere (test_group_region_contract, the
eager == replay tests).  One warm-up step, then one instrumented step: on the FIRST call of each signature (op, shapes, flags,
dtype) the wrapper synchronises, snapshots what the call accumulates into, launches, synchronises, and checks every output element
against the fp64 restatement with the per-element bound.  The loss, VAT / BCP, RNG, mask and optimizer launches are checked the same way
(exactly where the result is a label, a mask or a draw; largest_cc through scipy on the host), and so are bn_finalize (from the slots the conv
just wrote, with the running statistics snapshotted), the first conv's backward, the channel sums, the layout copies and the channel-drop kernels:
no entry point a step calls is left without a restatement.  test_every_launch_of_one_residual_step does the same for the residual 3D net
(has_residual=True: residual_fwd / residual_bwd / grad_sum, dx += dxin), at a shape chosen with the host-only launch planner.  Run with -s for one
line per signature (worst err / bound; 0.000 for an exact comparison)."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import inspect

import bench
from chap_amd import _lib, ops
from oracle import train_step as ots
from tests import kernel_ref as kr

DEV = torch.device("cuda", 0)

# ops.* entry points a step may call without a restatement below: none (an entry needs a sentence saying why its full-size fp64 restatement is not affordable)
EXCLUDED = {}
HELPERS = {"dt", "pack_weights", "stats_size", "stats_buffer", "stats_totals", "stats_from_moments", "act_bwd_sums_size"}


def nc(t, dims):
    """[N, D, H, W, C] -> [N, C, D, H, W]; dims = 2: the N*D slices as the batch, [N*D, C, H, W]."""
    t = t.permute(0, 4, 1, 2, 3)
    if dims == 2:
        n, c, d, h, w = t.shape
        t = t.transpose(1, 2).reshape(n * d, c, h, w)
    return t


def lazy_nc(lz, dims):
    """(v, dv) of a Lazy source: the fp32 values its consumers compute (kr.lazy_f32), NC(D)HW."""
    x = lz.raw[..., lz.coff:lz.coff + lz.C].permute(0, 4, 1, 2, 3)
    keep = None if lz.keep is None else lz.keep.permute(0, 4, 1, 2, 3)
    v, dv = kr.lazy_f32(x, scale=lz.scale, shift=lz.shift, act=lz.act, slope=lz.slope, keep=keep, keep_scale=lz.keep_scale, chan_mul=lz.chan_mul)
    if dims == 2:
        n, c, d, h, w = v.shape
        v, dv = (t.transpose(1, 2).reshape(n * d, c, h, w) for t in (v, dv))
    return v, dv


def operand(srcs, combine, dims, dtype):
    parts = [lazy_nc(s, dims) for s in srcs]
    v, dv = (torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)) if combine == 0 else kr.add_f32(parts)
    return kr.mfma_operand(v, dv, dtype)


def sig(x):
    if isinstance(x, torch.Tensor):
        return ("T", tuple(x.shape), str(x.dtype))
    if isinstance(x, ops.Lazy):
        return ("L", tuple(x.raw.shape), str(x.raw.dtype), x.C, x.coff, x.scale is not None, x.act, x.keep is not None, x.chan_mul is not None)
    if isinstance(x, (list, tuple)):
        return tuple(sig(v) for v in x)
    if isinstance(x, dict):
        return tuple(sorted((k, sig(v)) for k, v in x.items()))
    return x


class Checker:
    def __init__(self, weights, dtype):
        self.weights, self.dtype = weights, dtype
        self.recorded, self.checked, self.lines, self.called, self.deferred = set(), set(), [], set(), []
        self.cm_of, self.cm_matched = {}, 0

    # ---- wiring ACROSS launches, on every call (not only the first of a signature): the Dropout3d multipliers the forward consumers applied to a
    # stored tensor are the ones chap_residual_bwd gets for it (a restatement from the call's own arguments cannot see a multiplier left out)
    def note(self, name, a, k):
        ptr = lambda t: None if t is None else t.data_ptr()
        if name == "residual_bwd":
            q = self._args(name, a, k)
            key = (q["out"].data_ptr(), 0, q["out"].shape[-1])
            if key in self.cm_of:
                assert self.cm_of[key] == ptr(q["chan_mul"]), "residual_bwd: chan_mul is not the one the forward consumers of this output applied"
                self.cm_matched += q["chan_mul"] is not None
            return

        def walk(v):
            if isinstance(v, ops.Lazy):
                self.cm_of[(v.raw.data_ptr(), v.coff, v.C)] = ptr(v.chan_mul)
            elif isinstance(v, (list, tuple)):
                for x in v:
                    walk(x)
        walk(a)
        walk(list(k.values()))

    def report(self, key, worst):
        self.checked.add(key)
        self.lines.append("%-14s worst err/bound %s   %s" % (key[0], " ".join("%.3f" % w for w in worst), key[1:]))

    # ---- conv_fwd
    def conv_fwd(self, f, srcs, wpacked, bias, cout, out, *, grid, in_dims, ksize, stride, dims, combine=0, out_ld=None, out_coff=0,
                 out_mode=0, out_cn=0, out_planar=False, out_f32=False, stats=None, stats_shift=None, out2=None):
        f(srcs, wpacked, bias, cout, out, grid=grid, in_dims=in_dims, ksize=ksize, stride=stride, dims=dims, combine=combine, out_ld=out_ld,
          out_coff=out_coff, out_mode=out_mode, out_cn=out_cn, out_planar=out_planar, out_f32=out_f32, stats=stats, stats_shift=stats_shift, out2=out2)
        torch.cuda.synchronize()
        w, kind = self.weights[wpacked.data_ptr()]
        a, flip = operand(srcs, combine, dims, self.dtype)
        k = w.shape[1] if kind in (kr.PACK_CONV_FWD, kr.PACK_DECONV_DGRAD) else w.shape[0]     # K channels of the weight: the first conv's
        a, flip = a[:, :k], flip[:, :k]                    # input arrives zero-padded to 16 channels (the packed weights are 0 beyond K)
        r = kr.conv_ref(kind, a, kr.weight_operand(w, self.dtype).to(DEV), bias, flip=flip)
        del a, flip
        creal = out_cn if out_mode == 1 else cout
        if out_planar:
            got = out.permute(0, 2, 3, 4, 1) if out.dim() == 5 else out.permute(0, 2, 3, 1).unsqueeze(1)
        elif out2 is not None:
            got = torch.cat((out[..., out_coff:out_coff + out.shape[-1] - out_coff], out2[..., out_coff:out_coff + cout - out.shape[-1]]), -1)
        else:
            got = out[..., out_coff:out_coff + creal]
        got = nc(got, dims)
        store = torch.float32 if (out_planar or out_f32) else self.dtype
        worst = [kr.check("conv_fwd out", got, r["y"], kr.conv_bound(r, store))]
        if stats is not None:
            (s1, b1), (s2, b2) = kr.stats_ref(r, stats_shift)
            st = ops.stats_totals(stats, cout, creal)
            worst += [kr.check("conv_fwd stats S", st[0], s1, b1), kr.check("conv_fwd stats Q", st[1], s2, b2)]
        return worst

    # ---- wgrad (accumulates into dw, db)
    def wgrad(self, f, a_srcs, b, dw, strides, *, grid, in_dims, ksize, stride, dims, combine=0, db=None, kc_valid=0, kn_valid=0):
        p_dw, p_db = dw.detach().double().clone(), None if db is None else db.detach().double().clone()
        f(a_srcs, b, dw, strides, grid=grid, in_dims=in_dims, ksize=ksize, stride=stride, dims=dims, combine=combine, db=db,
          kc_valid=kc_valid, kn_valid=kn_valid)
        torch.cuda.synchronize()
        A, fA = operand(a_srcs, combine, dims, self.dtype)
        B, fB = operand([b], 0, dims, self.dtype)
        rw = kr.wgrad_ref(A, B, ksize=ksize, stride=stride, flipA=fA, flipB=fB if bool((fB != 0).any()) else None)
        del A, fA, fB
        taps, ca, cb = rw["dw"].shape
        kcv, knv = kc_valid or ca, kn_valid or cb
        ref, bnd = p_dw.clone(), torch.zeros_like(p_dw)
        view = ref.as_strided((taps, kcv, knv), strides)
        part = rw["dw"][:, :kcv, :knv]
        bv = kr.wgrad_bound(rw)[:, :kcv, :knv] + kr.U32 * (view + part).abs()
        view += part
        bnd.as_strided((taps, kcv, knv), strides).copy_(bv)
        worst = [kr.check("wgrad dW", dw, ref, bnd)]
        if db is not None:
            ref = p_db.clone()
            ref[:knv] += rw["db"][:knv]
            bd = torch.zeros_like(ref)
            bd[:knv] = kr.wgrad_bound(rw, which="db")[:knv] + kr.U32 * ref[:knv].abs()
            worst.append(kr.check("wgrad db", db, ref, bd))
        return worst

    # ---- act_bwd (accumulates into dgamma, dbeta)
    def act_bwd(self, f, lazy, grads, gout, *, g_pool=None, pool_idx=None, mean=None, invstd=None, gamma=None, dgamma=None, dbeta=None,
                count=1.0, bn_mode=None, sums=None):
        pg = None if dgamma is None else dgamma.detach().double().clone()
        pb = None if dbeta is None else dbeta.detach().double().clone()
        f(lazy, grads, gout, g_pool=g_pool, pool_idx=pool_idx, mean=mean, invstd=invstd, gamma=gamma, dgamma=dgamma, dbeta=dbeta, count=count,
          bn_mode=bn_mode, sums=sums)
        torch.cuda.synchronize()
        bn = bn_mode if bn_mode is not None else (1 if mean is not None else 0)
        C = lazy.C
        cut = lambda t, c0: t[..., c0:c0 + C].permute(0, 4, 1, 2, 3)
        raw = cut(lazy.raw, lazy.coff)
        ref = kr.act_bwd_ref(raw, [cut(t, c0) for t, c0 in grads], scale=lazy.scale, shift=lazy.shift, act=lazy.act, slope=lazy.slope,
                             keep=None if lazy.keep is None else cut(lazy.keep, 0), keep_scale=lazy.keep_scale, chan_mul=lazy.chan_mul,
                             g_pool=None if g_pool is None else cut(g_pool, 0), pool_idx=None if pool_idx is None else cut(pool_idx, 0),
                             bn_mode=bn, mean=mean, invstd=invstd, gamma_=gamma, count=count)
        worst = [kr.check("act_bwd gout", cut(gout, 0), ref["g"], kr.bound(ref["g"], extra=ref["g_bound"], store=self.dtype))]
        if ref["S0"] is not None and (bn == 1 or dgamma is not None or dbeta is not None):
            if dbeta is not None:
                worst.append(kr.check("act_bwd dbeta", dbeta, pb + ref["S0"], kr.param_grad_bound(ref["S0"], ref["b0"], pb)))
            if dgamma is not None:
                worst.append(kr.check("act_bwd dgamma", dgamma, pg + ref["S1"], kr.param_grad_bound(ref["S1"], ref["b1"], pg)))
        return worst

    # ---- first conv (Cin = 1): the image rounded to the operand type, like the weights
    def conv_c1_fwd(self, f, x, w, bias, out, *, dims, stats=None, stats_shift=None):
        f(x, w, bias, out, dims=dims, stats=stats, stats_shift=stats_shift)
        torch.cuda.synchronize()
        a = x.unsqueeze(1).double()
        a = a.float().to(self.dtype).double() if self.dtype == torch.bfloat16 else a
        if dims == 2:
            a = a[:, :, 0]
        r = kr.conv_ref(kr.PACK_CONV_FWD, a, kr.weight_operand(w, self.dtype).to(DEV), bias)
        worst = [kr.check("conv_c1 out", nc(out, dims), r["y"], kr.conv_bound(r, self.dtype))]
        if stats is not None:
            (s1, b1), (s2, b2) = kr.stats_ref(r, stats_shift)
            st = ops.stats_totals(stats, out.shape[-1])
            worst += [kr.check("conv_c1 stats S", st[0], s1, b1), kr.check("conv_c1 stats Q", st[1], s2, b2)]
        return worst

    # ---- 2x2(x2) max-pool of a lazy activation (values; the index is what act_bwd routes the pooled gradient by, checked there)
    def act_pool2(self, f, lazy, out, idx=None, dims=2):
        f(lazy, out, idx, dims=dims)
        torch.cuda.synchronize()
        v, dv = lazy_nc(lazy, 3)
        pool = F.max_pool3d if dims == 3 else (lambda t, k: F.max_pool2d(t[:, :, 0], k).unsqueeze(2))
        ref = pool(v, 2)
        return [kr.check("act_pool2 out", nc(out, 3), ref, kr.bound(ref, extra=pool(dv, 2), store=self.dtype))]

    # ---- bilinear / trilinear x2 and its adjoint.  Bound: the interpolation chain (<= 8 terms), the fp32 source coordinate
    # (<= 4 U32 * size off, times |v| on both sides of the cell: 8 U32 * size * max |v| of the channel), the operand term, the store.
    def _interp(self, t, dims, half_pixel):
        mode = "trilinear" if dims == 3 else "bilinear"
        t2 = t if dims == 3 else t[:, :, 0]
        y = F.interpolate(t2, scale_factor=2, mode=mode, align_corners=not half_pixel)
        return y if dims == 3 else y.unsqueeze(2)

    def upsample2x(self, f, lazy, out, *, dims, out_coff=0, half_pixel=False):
        f(lazy, out, dims=dims, out_coff=out_coff, half_pixel=half_pixel)
        torch.cuda.synchronize()
        v, dv = lazy_nc(lazy, 3)
        ref = self._interp(v, dims, half_pixel)
        size = max(v.shape[2:])
        vmax = v.abs().amax(dim=(2, 3, 4), keepdim=True)
        extra = self._interp(dv, dims, half_pixel) + 8 * kr.U32 * size * vmax
        got = nc(out[..., out_coff:out_coff + lazy.C], 3)
        return [kr.check("upsample2x out", got, ref, kr.bound(ref, sabs=self._interp(v.abs(), dims, half_pixel), chain=8, extra=extra, store=self.dtype))]

    def upsample2x_bwd(self, f, g, g_coff, C, out, *, dims):
        f(g, g_coff, C, out, dims=dims)
        torch.cuda.synchronize()
        gf = nc(g[..., g_coff:g_coff + C], 3).double()
        coarse = nc(out, 3).shape

        def adj(t):
            with torch.enable_grad():
                x = torch.zeros(coarse, dtype=torch.float64, device=DEV, requires_grad=True)
                return torch.autograd.grad(self._interp(x, dims, False), x, t)[0]
        ref = adj(gf)
        size = max(coarse[2:])
        extra = 8 * kr.U32 * size * adj(gf.abs().amax(dim=(2, 3, 4), keepdim=True).expand_as(gf).contiguous())
        return [kr.check("upsample2x_bwd", nc(out, 3), ref, kr.bound(ref, sabs=adj(gf.abs()), chain=64, extra=extra, store=self.dtype))]

    # ---- losses, VAT / BCP helpers, RNG, optimizer: the restatements of the second half of kernel_ref.py, on the GPU in fp64.  Inputs a
    # launch overwrites (in-place perturb / l2_normalize, accumulated gradients, the optimizer's buffers) are snapshotted first.
    @staticmethod
    def _args(name, a, k):
        b = inspect.signature(_ORIG[name]).bind(*a, **k)
        b.apply_defaults()
        return b.arguments

    def mix_loss_fwd(self, f, *a, **k):
        q = self._args("mix_loss_fwd", a, k)
        f(*a, **k)
        torch.cuda.synchronize()
        loss, acc = self._last(f)
        r = kr.mix_loss_ref(q["logits"], q["target_a"], q["target_b"], q["mask"], q["w_a"], q["w_b"], q["smooth"], q["k_dice"], q["k_ce"])
        NA = 2 + 3 * q["logits"].shape[1]
        return [kr.check("mix_loss acc", acc[:2 * NA].view(2, NA), r["acc"], r["acc_b"], "ka"), kr.check("mix_loss loss", loss, r["loss"], r["loss_b"], "k")]

    def mix_loss_bwd(self, f, *a, **k):
        q = self._args("mix_loss_bwd", a, k)
        prior = q["dlogits"].clone() if q["accumulate"] else None
        f(*a, **k)
        torch.cuda.synchronize()
        r = kr.mix_loss_ref(q["logits"], q["target_a"], q["target_b"], q["mask"], q["w_a"], q["w_b"], q["smooth"], q["k_dice"], q["k_ce"],
                            gscale=q["gscale"], gscale_dev=None if q["gscale_dev"] is None else float(q["gscale_dev"]), prior=prior)
        return [kr.check("mix_loss dlogits", q["dlogits"], r["dlogits"], r["dlogits_b"])]

    def pseudo_block(self, f, *a, **k):
        q = self._args("pseudo_block", a, k)
        f(*a, **k)
        torch.cuda.synchronize()
        s1, s2, a1, a2, kn = self._last(f)
        r = kr.pseudo_ref(q["logits1"], q["logits2"])
        ok = ~r["near"]
        assert float(r["near"].double().mean()) <= kr.NEAR_TIE_CAP, ("near ties", int(r["near"].sum()), r["near"].numel())
        assert bool((a1[ok] == r["arg1"][ok]).all()) and bool((a2[ok] == r["arg2"][ok]).all())
        worst = [kr.check("pseudo knowledge", torch.where(ok, kn.double(), r["knowledge"]), r["knowledge"], r["knowledge_b"], "ndhw")]
        if s1 is not None:
            worst += [kr.check("pseudo soft1", s1, r["soft1"], r["soft1_b"]), kr.check("pseudo soft2", s2, r["soft2"], r["soft2_b"])]
        return worst

    def kl_fwd_bwd(self, f, *a, **k):
        q = self._args("kl_fwd_bwd", a, k)
        prior = 0.0 if q["loss"] is None else float(q["loss"])
        f(*a, **k)
        torch.cuda.synchronize()
        r = kr.kl_ref(q["logits"], q["targets"], q["mode"], gscale=q["gscale"], gscale_dev=None if q["gscale_dev"] is None else float(q["gscale_dev"]), prior=prior)
        worst = [] if q["loss"] is None else [kr.check("kl loss", q["loss"], r["loss"], r["loss_b"], "k")]
        return worst + [kr.check("kl g%d" % h, q["dlogits"][h], r["g"][h], r["g_b"][h]) for h in range(2) if q["dlogits"][h] is not None] or [0.0]

    def l2_normalize(self, f, *a, **k):
        q = self._args("l2_normalize", a, k)
        ref, b = kr.l2_normalize_ref(q["x"], q["eps"])
        f(*a, **k)
        torch.cuda.synchronize()
        return [kr.check("l2_normalize", q["out"].reshape(ref.shape), ref, b)]

    def perturb(self, f, *a, **k):
        q = self._args("perturb", a, k)
        d = q["d"]
        if d.shape != q["x"].shape and d.numel() == q["x"].numel():      # dx [N, 1, D, H, W] += dxin [N, D*H*W] (the residual first block): the kernel is flat
            d = d.reshape(q["x"].shape)
        ref, b = kr.perturb_ref(q["x"], d, q["alpha"], q["mask"], q["sign"])      # before the launch: out may BE x
        f(*a, **k)
        torch.cuda.synchronize()
        return [kr.check("perturb", q["out"].reshape(ref.shape), ref, b)]

    def rand_uniform(self, f, *a, **k):
        q = self._args("rand_uniform", a, k)
        sd = None if q["seed_dev"] is None else int(q["seed_dev"])
        f(*a, **k)
        torch.cuda.synchronize()
        out = q["out"].reshape(-1)
        ref, b = kr.rand_uniform_ref(q["seed"], out.numel(), q["lo"], q["hi"], sd, DEV)
        assert float(out.min()) >= q["lo"] and float(out.max()) < q["hi"]
        return [kr.check("rand_uniform", out, ref, b, "i")]

    # keep_mask / chan_mask go through the launch layer: inside a grouped region (the executor issues the masks of a pass as ONE grid,
    # whatever CHAP_GROUP says) the launch is only recorded, so the comparison waits until the region has been closed (Checker.flush).
    def _mask(self, f, name, a, k, buf, ref_fn):
        q = self._args(name, a, k)
        sd = None if q["seed_dev"] is None else int(q["seed_dev"])
        f(*a, **k)

        def verify():
            torch.cuda.synchronize()
            assert torch.equal(q[buf].reshape(-1), ref_fn(q["seed"], q[buf].numel(), q["prob"], sd, DEV)), name
            return [0.0]
        return verify if _lib.group.held is not None else verify()

    def keep_mask(self, f, *a, **k):
        return self._mask(f, "keep_mask", a, k, "keep", kr.keep_mask_ref)

    def chan_mask(self, f, *a, **k):
        return self._mask(f, "chan_mask", a, k, "mul", kr.chan_mask_ref)

    def flush(self):
        if _lib.group.held is None:
            while self.deferred:
                key, verify = self.deferred.pop(0)
                self.report(key, verify())

    def box_mix(self, f, *a, **k):
        q = self._args("box_mix", a, k)
        ref = kr.box_mix_ref(q["a"].clone(), q["b"].clone(), q["box"].tolist())
        f(*a, **k)
        torch.cuda.synchronize()
        assert torch.equal(q["out"], ref.reshape(q["out"].shape))
        return [0.0]

    def box_mask(self, f, *a, **k):
        q = self._args("box_mask", a, k)
        f(*a, **k)
        torch.cuda.synchronize()
        box = q["box"].tolist()
        assert torch.equal(q["mask"].cpu(), kr.box_mask_ref(q["mask"].shape[0], tuple(q["mask"].shape[-(len(box) // 2):]), box).reshape(q["mask"].shape))
        return [0.0]

    def largest_cc(self, f, *a, **k):
        q = self._args("largest_cc", a, k)
        f(*a, **k)
        torch.cuda.synchronize()
        lab, nc_ = q["labels"].cpu(), q["num_classes"]
        assert torch.equal(self._last(f).cpu(), ots.largest_cc(torch.where((lab > 0) & (lab < nc_), lab, torch.zeros_like(lab)), nc_))
        return [0.0]

    def diff_mask(self, f, *a, **k):
        """knowledge is arbitrary here: the fp32 pooled means (16 adds: <= 16 U32 relative) may order two cells differently from fp64 where they
        lie within that band of the threshold.  Outside the band the mask is exact; the band may hold, beyond the threshold cell of each
        sample, at most 0.01 % of the cells (rounded up)."""
        q = self._args("diff_mask", a, k)
        f(*a, **k)
        torch.cuda.synchronize()
        got, kn = self._last(f), q["knowledge"]
        n = kn.shape[0]
        kn3, p1, p2 = kn.reshape(n, -1, kn.shape[-1]), q["p1"].reshape(n, -1, kn.shape[-1]), q["p2"].reshape(n, -1, kn.shape[-1])
        sc = q["scale"]
        pooled = F.avg_pool2d(kn3.double().unsqueeze(1), sc).squeeze(1).clamp_min(0)
        kk = kr.diff_mask_k(q["topk"], pooled[0].numel())
        thr = pooled.reshape(n, -1).topk(kk, dim=1).values[:, -1].view(n, 1, 1)
        band = (pooled - thr).abs() <= 16 * kr.U32 * (pooled + thr)
        assert int(band.sum()) - n <= -(-band.numel() // 10000), ("cells at the threshold", int(band.sum()), band.numel())
        up = lambda t: t.repeat_interleave(sc, 1).repeat_interleave(sc, 2)
        ref = kr.diff_mask_ref(p1, p2, kn3, sc, kk)
        free = up(band)
        assert torch.equal(torch.where(free, ref, got.reshape(ref.shape)), ref)
        return [0.0]

    def sgd_step(self, f, *a, **k):
        q = self._args("sgd_step", a, k)
        p2, e_p, m2, e_m = kr.sgd_ref(q["param"], q["grad"], q["mom"], float(q["lr_dev"]), q["momentum"], q["weight_decay"], q["grad_scale"], q["grad2"])
        g0 = [None if t is None else t.clone() for t in (q["grad"], q["grad2"])]
        f(*a, **k)
        torch.cuda.synchronize()
        for t, t0 in zip((q["grad"], q["grad2"]), g0):
            if t is not None:
                assert torch.equal(t, torch.zeros_like(t) if q["zero_grad"] else t0)
        return [kr.check("sgd param", q["param"], p2, e_p, "i"), kr.check("sgd mom", q["mom"], m2, e_m, "i")]

    def grad_sim(self, f, *a, **k):
        q = self._args("grad_sim", a, k)
        ref, b = kr.grad_sim_ref(q["gl"], q["gu"], q["score"], q["ema"])
        f(*a, **k)
        torch.cuda.synchronize()
        return [kr.check("grad_sim", q["score"], ref, b, "c")]

    # ---- residual blocks (csrc/residual.hip): the add + ReLU, its backward with the image's gradient, the fold of more than three contributions.
    # Chain lengths as in tests/test_residual_kernels_gpu.py: r + (src0 + src1); ((g0 + g1) + g2) and the multiplier; C for dxin's channel sum.
    def residual_fwd(self, f, r, srcs, out, xin=None):
        f(r, srcs, out, xin=xin)
        torch.cuda.synchronize()
        parts = [lazy_nc(r, 3)] + [lazy_nc(s, 3) for s in srcs]
        if not srcs:                                        # block_one: the one-channel image, broadcast over the channels
            n, d, h, w = out.shape[:4]
            xi = xin.double().reshape(n, 1, d, h, w).expand_as(parts[0][0])
            parts.append((xi, torch.zeros_like(xi)))
        pre = sum(p[0] for p in parts)
        ref = pre.clamp_min(0)                              # ReLU is 1-Lipschitz: the bound of the sum holds behind it
        bnd = kr.bound(ref, sabs=sum(p[0].abs() for p in parts), chain=len(parts), flip=sum(p[1] for p in parts), store=out.dtype)
        return [kr.check("residual_fwd out", nc(out, 3), ref, bnd)]

    def residual_bwd(self, f, grads, out, gout, chan_mul=None, dxin=None):
        f(grads, out, gout, chan_mul=chan_mul, dxin=dxin)
        torch.cuda.synchronize()
        C = out.shape[-1]
        gs = [nc(t[..., c0:c0 + C], 3).double() for t, c0 in grads]
        o = nc(out, 3).double()
        fac = (o > 0).double()
        if chan_mul is not None:
            fac = fac * kr._bcast(chan_mul, o, per_sample=True)
        ref, sabs = sum(gs) * fac, sum(t.abs() for t in gs) * fac
        got = nc(gout, 3)
        worst = [kr.check("residual_bwd gout", got, ref, kr.bound(ref, sabs=sabs, chain=len(gs) + 1, store=gout.dtype))]
        assert bool((got[o == 0] == 0).all())               # strictly-greater test: exact zeros where out == 0
        if dxin is not None:                                # the channel sum of the UNROUNDED values (each within its bound without the store term)
            e = kr.bound(ref, sabs=sabs, chain=len(gs) + 1)
            dref = ref.sum(1)
            dbnd = kr.bound(dref, sabs=ref.abs().sum(1), chain=C, extra=e.sum(1), store=torch.float32)
            worst.append(kr.check("residual_bwd dxin", dxin.reshape(dref.shape), dref, dbnd, "ndhw"))
        return worst

    def grad_sum(self, f, grads, out):
        f(grads, out)
        torch.cuda.synchronize()
        C = out.shape[-1]
        gs = [nc(t[..., c0:c0 + C], 3).double() for t, c0 in grads]
        ref = sum(gs)
        return [kr.check("grad_sum", nc(out, 3), ref, kr.bound(ref, sabs=sum(t.abs() for t in gs), chain=len(gs), store=out.dtype))]

    # ---- BatchNorm finalize / eval affine, the first conv's backward, channel sums, layout copies, the channel-drop kernels
    def bn_finalize(self, f, stats, gamma, beta, running_mean, running_var, nbt, count, eps, momentum, scale, shift, mean=None, invstd=None,
                    stats_shift=None, clog=None):
        C = gamma.numel()
        clog = C if clog is None else clog
        nslots = int(stats[:1].view(torch.int32).item())
        slots = stats[_lib.STATS_HDR:_lib.STATS_HDR + nslots * 2 * clog].view(nslots, 2, clog).clone()
        snap = lambda t: None if t is None else t.clone()
        rm0, rv0, sh0, nbt0 = snap(running_mean), snap(running_var), snap(stats_shift), snap(nbt)      # stats_shift may BE running_mean
        f(stats, gamma, beta, running_mean, running_var, nbt, count, eps, momentum, scale, shift, mean=mean, invstd=invstd, stats_shift=stats_shift, clog=clog)
        torch.cuda.synchronize()
        ref = kr.bn_finalize_ref(slots, nslots, C, clog, count, sh0, gamma, beta, rm0, rv0, momentum, eps)
        outs = dict(scale=scale, shift=shift, mean=mean, invstd=invstd, running_mean=running_mean, running_var=running_var)
        worst = [kr.check("bn_finalize " + k, outs[k], ref[k][0], ref[k][1], "c") for k in ref if outs[k] is not None]
        if "running_mean" in ref:
            assert nbt is None or int(nbt) == int(nbt0) + 1
        elif running_mean is not None:
            assert torch.equal(running_mean, rm0) and torch.equal(running_var, rv0) and (nbt is None or int(nbt) == int(nbt0))
        return worst

    def bn_eval_affine(self, f, gamma, beta, running_mean, running_var, eps, scale, shift):
        f(gamma, beta, running_mean, running_var, eps, scale, shift)
        torch.cuda.synchronize()
        (sc, e_sc), (sh, e_sh) = kr.bn_eval_ref(gamma, beta, running_mean, running_var, eps)
        return [kr.check("bn_eval scale", scale, sc, e_sc, "c"), kr.check("bn_eval shift", shift, sh, e_sh, "c")]

    def conv_c1_bwd(self, f, g, w, x, *, dims, dx=None, dw=None, db=None):
        p_dw, p_db = (None if t is None else t.detach().double().clone() for t in (dw, db))
        f(g, w, x, dims=dims, dx=dx, dw=dw, db=db)
        torch.cuda.synchronize()
        gy = nc(g, dims).double()
        worst = []
        if dw is not None or db is not None:
            A = x.double().reshape(gy.shape[0], 1, *gy.shape[2:])
            rw = kr.wgrad_ref(A, gy, ksize=3, stride=1)
            taps = 3 ** dims
            st = (1, taps, taps)
            if dw is not None:
                worst.append(kr.check("conv_c1_bwd dW", dw, kr.to_layout(rw["dw"], st, dw.shape) + p_dw,
                                      kr.to_layout(kr.wgrad_bound(rw, p_dw.as_strided((taps, 1, dw.shape[0]), st)), st, dw.shape)))
            if db is not None:
                worst.append(kr.check("conv_c1_bwd db", db, rw["db"] + p_db, kr.wgrad_bound(rw, p_db, which="db"), "c"))
        if dx is not None:
            r = kr.conv_ref(kr.PACK_CONV_DGRAD, gy, w.detach().double())
            worst.append(kr.check("conv_c1_bwd dx", dx.reshape(r["y"].shape), r["y"], kr.conv_bound(r, torch.float32)))
        return worst

    def channel_sum(self, f, lazy, out):
        prior = out.clone()
        f(lazy, out)
        torch.cuda.synchronize()
        ref, b = kr.channel_sum_ref(lazy_nc(lazy, 3), prior)
        return [kr.check("channel_sum", out, ref, b, "c")]

    def planar_to_cl(self, f, x, out, out_coff=0, cpad=0):
        out0 = out.clone()
        f(x, out, out_coff=out_coff, cpad=cpad)
        torch.cuda.synchronize()
        iv = torch.int32 if out.dtype == torch.float32 else torch.int16
        assert torch.equal(out.view(iv), kr.planar_to_cl_ref(x, out0, out_coff, cpad).view(iv)), "planar_to_cl"
        return [0.0]

    def cl_to_planar(self, f, lazy, out):
        f(lazy, out)
        torch.cuda.synchronize()
        v, dv = lazy_nc(lazy, 3)                            # the output is the lazy value itself (exact without an affine)
        return [kr.check("cl_to_planar", out.reshape(v.shape), v, dv)]

    def sample_channel_sum(self, f, lazy, nchunk=32):
        f(lazy, nchunk=nchunk)
        torch.cuda.synchronize()
        r = kr.sample_channel_sum_ref(lazy_nc(lazy, 3))
        tot = self._last(f).double().sum(1)
        return [kr.check("sample_channel_sum", tot, r["sum"], r["sum_b"], "nc"), kr.check("sample_channel_sum mean", tot / lazy.raw[0, ..., 0].numel(), r["mean"], r["mean_b"], "nc")]

    def channel_drop(self, f, mul1, mul2, u1, u2, B, mode, **k):
        f(mul1, mul2, u1, u2, B, mode, **k)
        torch.cuda.synchronize()
        r = kr.channel_drop_ref(u1, u2, B, mode, **{n: v for n, v in k.items() if n != "probs_out"})
        return [kr.channel_drop_check("channel_drop", r, B, mul1, mul2, k.get("probs_out"))]

    def fold_perturbed(self, f, g, coff, Cc, mul, B, U):
        f(g, coff, Cc, mul, B, U)
        torch.cuda.synchronize()
        ref, b = kr.fold_ref(g, coff, Cc, mul, B, U, g.dtype)
        return [kr.check("fold_perturbed", self._last(f), ref, b, "ndhwc")]

    @staticmethod
    def _last(f):
        return f.res[-1]


_ORIG = {}


def instrument(monkeypatch, chk):
    for name in [n for n in dir(ops) if not n.startswith("_") and callable(getattr(ops, n))]:
        fn = getattr(ops, name)
        if name in HELPERS or isinstance(fn, type) or getattr(fn, "__module__", None) != ops.__name__:
            continue
        _ORIG[name] = fn

        def wrap(*a, _f=fn, _n=name, **k):
            chk.called.add(_n)
            chk.flush()
            chk.note(_n, a, k)
            handler = getattr(chk, _n, None)
            if handler is None:
                return _f(*a, **k)
            key = (_n, sig(a), sig(k))
            if key in chk.recorded:
                return _f(*a, **k)
            chk.recorded.add(key)
            torch.cuda.synchronize()
            res = []
            call = lambda *a2, **k2: res.append(_f(*a2, **k2))
            call.res = res                                  # the handlers of ops that RETURN their outputs read them here
            worst = handler(call, *a, **k)
            torch.cuda.empty_cache()
            if callable(worst):
                chk.deferred.append((key, worst))
            else:
                chk.report(key, worst)
            return res[0]
        monkeypatch.setattr(ops, name, wrap)


def run_checked_step(name, model, step, dtype, vol, lab, monkeypatch):
    """One warm-up step, then one instrumented step; every recorded signature was checked and nothing called is unrestated.  Returns the Checker."""
    step.step(vol, lab)                                    # warm-up: packs the weights, picks every launch once
    torch.cuda.synchronize()
    ex = model._exec
    sd = ex._sd()
    weights = {buf.data_ptr(): (sd[name_], kind) for (name_, kind), buf in ex._packed[dtype]["bufs"].items()}
    chk = Checker(weights, dtype)
    instrument(monkeypatch, chk)
    step.step(vol, lab)
    torch.cuda.synchronize()
    chk.flush()
    monkeypatch.undo()
    print("\n%s: %d signatures checked" % (name, len(chk.checked)))
    for line in chk.lines:
        print("  " + line)
    assert chk.checked == chk.recorded and chk.checked
    unrestated = {n for n in chk.called if not hasattr(Checker, n)}
    assert unrestated <= set(EXCLUDED), sorted(unrestated - set(EXCLUDED))
    return chk


@pytest.mark.parametrize("dtype_name", ["bf16", "fp32"])
@pytest.mark.parametrize("cfg", ["2d", "3d"])
def test_every_launch_of_one_step(cfg, dtype_name, monkeypatch):
    monkeypatch.setenv("CHAP_GROUP", "0")
    B, sp = (24, (256, 256)) if cfg == "2d" else (4, (112, 112, 80))
    if cfg == "3d" and dtype_name == "fp32":
        sp = (64, 64, 48)                                  # the fp32 3D step at full size would take a third of the time budget alone
    np.random.seed(1337)
    random.seed(1337)
    model, step, dtype = bench.build_step(cfg, dtype_name, B, sp, 1, {"concurrent": False}, 1, DEV)
    vol, lab = bench.synthetic(cfg, 1337, B, sp, DEV)
    run_checked_step("%s %s" % (cfg, dtype_name), model, step, dtype, vol, lab, monkeypatch)


RESIDUAL_SP = (16, 16, 48)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp32"])
def test_every_launch_of_one_residual_step(dtype_name, monkeypatch):
    """Every launch of one training iteration of the RESIDUAL 3D net (DualDecoder3d(has_residual=True, has_dropout=True), VAT on), as above: the step is
    built with bench.build_step's lines for the 3D configuration (which builds the plain nets only), run eagerly, ungrouped, on one stream.  Beyond the
    plain step's launches it checks residual_fwd (image / one source / up + skip), residual_bwd (with chan_mul on a dropped block output, with dxin in
    block_one), grad_sum (the program-order fold of a skip feature's five contributions, from the very tensors the executor passed), perturb as
    dx += dxin, and bn_finalize / conv_fwd / wgrad / act_bwd on Lazies with act=False (a BatchNorm with no activation behind it) and on residual
    outputs (no affine, with and without Dropout3d multipliers, alone or as the second operand of the skip add).

    Shape: B = 4 (2 labelled + 2 unlabelled; the executor passes N = 2 per pass) at 16 x 16 x 48, the smallest multiple of 16 per axis (five levels)
    at which the bf16 step still takes conv bricks (level 0: 2 * 4 * 4 * 3 = 96 bricks >= 64), the K-parallel route, the 1x1x1 head, weight-gradient
    bricks with 16-wide (level 0) and 32-wide B tiles (level 1: 2 * 2 * 2 * 2 = 16 bricks >= CHAP_WGRAD_BRICK's 16; 16 x 16 x 32 gives 8) and
    weight-gradient slabs.  Routes of the 3x3x3 layers per level from the host-only planner (conv_plan.h / wgrad_plan.h through the probe of
    tests/test_launch_plan_cpu.py, N = 2), conv = forward and input-gradient conv of one source / add-combined forward conv:

      bf16   level  channels   112 x 112 x 80                                      16 x 16 x 48
             0      16         conv bricks NT1 MR4          wgrad brick bn16       conv bricks NT1 MR4          wgrad brick bn16
             1      32         conv bricks NT2 MR4          wgrad brick bn32       conv slabs NT2 MR1           wgrad brick bn32
             2      64         conv bricks NT2 MR4          wgrad brick bn32       kpar cpar4 / slabs NT4 MR1   wgrad slab KC32
             3      128        kpar cpar4 / slabs NT4 MR1   wgrad brick bn32       kpar cpar4 / slabs NT4 MR1   wgrad slab KC32
             4      256        kpar cpar4 / slabs NT4 MR1   wgrad slab KC32        kpar cpar4 / slabs NT4 MR1   wgrad slab KC32
             head   16 -> 2    conv_head1x1                                        conv_head1x1
      fp32   0 .. 4            slabs NT1 / NT2 / NT4 / NT4 / NT4, MR1; wgrad slab KC16 / KC32 / KC32 / KC32 / KC32: the same at both shapes

    What the full-size step takes and this one cannot reach (a brick conv needs >= 64 bricks, and from 128 up it takes NT2): the bf16 brick conv with
    32 K-channels and NT2 and the one with 64 K-channels (four chunks), both also add-combined -- covered with residual-style sources by
    tests/test_kernels_gpu.py::test_conv3d_residual_sources[brick32 / brick64]; the weight-gradient bricks with 64 and 128 A channels are the
    bn32 instance of level 1 with more chunks -- tests/test_kernels_bwd_gpu.py::test_wgrad_conv3d_residual_sources forces the bricks onto 32 -> 32
    and 64 -> 128."""
    from chap_amd.networks import DualDecoder3d
    from chap_amd.train import ChapStep
    monkeypatch.setenv("CHAP_GROUP", "0")
    B, sp = 4, RESIDUAL_SP
    np.random.seed(1337)
    random.seed(1337)
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    torch.manual_seed(1337)                                 # bench.build_step's lines for the 3D configuration, with has_residual=True
    model = DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True, has_residual=True).to(DEV).train().set_compute_dtype(dtype)
    step = ChapStep(model, dict(batch_size=B, labeled_bs=B // 2, vat_iters=1, num_classes=2, concurrent=False), world_size=1)
    vol, lab = bench.synthetic("3d", 1337, B, sp, DEV)
    chk = run_checked_step("3d residual %s" % dtype_name, model, step, dtype, vol, lab, monkeypatch)
    # the residual path's own launches were among the checked signatures (key = (op, sig(args), sig(kwargs)); a Lazy's sig: ..., has scale, act, ...)
    ops_seen = {k[0] for k in chk.checked}
    assert {"residual_fwd", "residual_bwd", "grad_sum", "perturb", "act_bwd", "conv_fwd", "wgrad", "bn_finalize"} <= ops_seen
    kw = lambda k: dict(k[2])
    assert any(k[0] == "residual_fwd" and kw(k).get("xin") is not None for k in chk.checked)                   # block_one: the image as the block's input
    assert any(k[0] == "residual_fwd" and len(k[1][1]) == 2 for k in chk.checked)                               # a decoder block: up + skip
    assert any(k[0] == "residual_bwd" and kw(k).get("dxin") is not None for k in chk.checked)
    assert any(k[0] == "residual_bwd" and kw(k).get("dxin") is None and kw(k).get("chan_mul") is not None for k in chk.checked)
    assert chk.cm_matched > 0                                                                                   # ... and it was the consumers' multiplier (Checker.note)
    assert any(k[0] == "grad_sum" for k in chk.checked)
    assert any(k[0] == "perturb" and k[1][0][1] != k[1][1][1] for k in chk.checked)                             # dx [N, 1, D, H, W] += dxin [N, D*H*W]
    assert any(k[0] == "act_bwd" and k[1][0][5] and not k[1][0][6] for k in chk.checked)                        # a BatchNorm with no activation behind it
