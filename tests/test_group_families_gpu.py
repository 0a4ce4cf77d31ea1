"""Merged (grouped) launches of every kernel family behind the trampoline of chap_amd/csrc/launch.h, case by case of tests/group_cases.py: each
case runs as 2 and as 4 lanes of the same shapes and different data -- once lane by lane as single launches, once inside one chap_amd._lib.group region --
and group_cases.check_lanes() asserts that everything merged into one grid per recorded position, that every lane's merged outputs are the single
launches' bit for bit, per element within the kernel's own fp64 bound of THAT lane's reference, different from the other lanes', and that the NaN guards
around them are untouched.  Conv and weight-gradient cases go through the inputs, references and bounds of tests/small_conv_cases.py /
tests/k3_conv_cases.py (the weight gradient through ops.wgrad, whose per-lane workspace comes from _lib.hold_empty); the other families through the
fp64 restatements of tests/test_step_launches_gpu.py's Checker, handed the launch's own arguments.  Further: the lane-count rules (3 lanes, 5 = 4 + 1,
A-B-A, the same shape in the other dtype, lanes of unequal length) on three chains, and the refusal of every directly launched entry point inside a
region.  A runtime error ends the session; nothing is retried.  Each case prints one `groupcase {json}` line.  Needs a GPU."""
import contextlib
import json
import math
import os
import re
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

if os.path.dirname(os.path.dirname(os.path.abspath(__file__))) not in sys.path:      # (run as a program: the child process of the read-once-knob cases)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chap_amd import _lib as L
from chap_amd import ops
from tests import group_cases as gc
from tests import k3_conv_cases as kc
from tests import kernel_ref as kr
from tests import small_conv_cases as sc
from tests.plan_probe import KNOBS
from tests.test_k3_conv_families_gpu import device_alive as k3_device_alive
from tests.test_k3_conv_families_gpu import sources
from tests.test_small_conv_families_gpu import DEV, cl, g4, lazy_of
from tests.test_step_launches_gpu import Checker, nc

NAN = float("nan")
G = gc.GUARD


REFUSED = re.compile(r" failed \((-1|-2)\): ")             # _lib.call's text for CHAP_EINVAL / CHAP_EUNSUPPORTED: an argument check, in front of any launch


class device_alive(k3_device_alive):
    """the guard of tests/test_k3_conv_families_gpu.py -- launch and synchronise inside; an error of the runtime there ends the whole session -- with ONE
    exception, told by the library's return code, not by wording: an entry point that returned CHAP_EINVAL or CHAP_EUNSUPPORTED refused its arguments
    before it started anything, which is a failed test.  Every other ChapError (CHAP_ELAUNCH, a code this file does not know) and every other exception
    ends the session as there."""
    def __exit__(self, et, ev, tb):
        if et is not None and issubclass(et, L.ChapError) and REFUSED.search(str(ev)):
            raise AssertionError("refused: %s" % ev) from ev
        return super().__exit__(et, ev, tb)


@contextlib.contextmanager
def knobs_set(knobs):
    """the planner's live knobs, for the calls inside (the plan is made when a launch is issued or recorded)"""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in knobs.items()})
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def captured():
    """kernel_ref.check, for the calls inside, records (got, reference, bound) instead of asserting: group_cases.check_lanes asserts"""
    cap, orig = {}, kr.check

    def record(name, got, ref, bnd, dims="ncdhw"):
        ref = kr._c(ref)
        cap[name] = (kr._c(got, ref).cpu(), ref.cpu(), kr._c(bnd, ref).cpu())
        return 0.0
    kr.check = record
    try:
        yield cap
    finally:
        kr.check = orig


class Lane:
    """one lane: its device inputs, its outputs (NaN-filled, NaN guard bands around them), the ops calls that make them"""

    def __init__(self, dtype, knobs=None):
        self.dtype, self.knobs = dtype, dict(knobs or {})
        self.calls, self.bufs, self.ret, self.exact, self.extra = [], {}, {}, {}, None

    def out(self, name, shape, dtype, fill=NAN, init=None):
        n = math.prod(shape)
        buf = torch.full((n + 2 * G,), fill, device=DEV, dtype=dtype)
        view = buf[G:G + n].view(shape)
        if init is not None:
            view.copy_(init)
        self.bufs[name] = (buf, n)
        return view

    def plain(self, name, t):
        self.bufs[name] = (t, None)
        return t

    def call(self, op, *a, writes, **k):
        self.calls.append((op, a, k, tuple(writes)))

    def ready(self):
        self.prior = {n: b.clone() for n, (b, _) in self.bufs.items()}
        return self

    def run(self):
        with knobs_set(self.knobs):
            for i, (op, a, k, _) in enumerate(self.calls):
                r = getattr(ops, op)(*a, **k)
                if isinstance(r, torch.Tensor):
                    self.ret[i] = r

    def tensors(self):
        """what the bit comparison sees: every buffer whole, its guard bands, the returned tensors"""
        res = {}
        for n, (b, cnt) in self.bufs.items():
            res[n + "#raw"] = b.cpu()
            if cnt is not None:
                res[n + "#guard"] = torch.cat((b[:G], b[G + cnt:])).cpu()
        res.update({"ret%d#raw" % i: t.cpu() for i, t in self.ret.items()})
        return res

    def verify(self):
        """(got, reference, bound) by name: every call through the Checker's fp64 restatement of its op, from the call's own arguments.  A restatement
        snapshots what its op accumulates into and then launches: here the `launch` puts the finished buffers back over their priors.

        What this leans on, and what holds it in place: (a) a Checker method reads a buffer its op writes only BEFORE it calls f (a snapshot of the prior)
        or AFTER (the result) -- true of every method used here (read with this file; tests/test_step_launches_gpu.py states it as the Checker's design:
        "snapshots what the call accumulates into, launches, ... checks"); a method that read an output first and kept it as the result would compare the
        prior, which is the NaN fill for everything but the accumulated outputs, and kernel_ref.check fails on a NaN.  (b) f is called exactly once
        (asserted below).  (c) kernel_ref.check is replaced for the duration of ONE handler call, in this process, and put back in a finally; what a
        handler asserts directly (residual_bwd's exact zeros, bn_finalize's counter) is asserted there and then, in addition to check_lanes.  (d) the
        bounds are the Checker's own, unchanged."""
        got, ref, bnd = {}, {}, {}
        chk = Checker({}, self.dtype)
        for i, (op, a, k, writes) in enumerate(self.calls):
            if op in self.exact:
                continue
            saved = {n: self.bufs[n][0].clone() for n in writes}
            for n in writes:
                self.bufs[n][0].copy_(self.prior[n])

            launched = []

            def put_back(*_a, _s=saved, _l=launched, **_k):
                _l.append(1)
                for n, t in _s.items():
                    self.bufs[n][0].copy_(t)
            put_back.res = [self.ret.get(i)]
            with captured() as cap:
                getattr(chk, op)(put_back, *a, **k)
            assert cap and len(launched) == 1, (op, len(launched))
            for name, (g_, r_, b_) in cap.items():
                got["%d %s" % (i, name)], ref["%d %s" % (i, name)], bnd["%d %s" % (i, name)] = g_, r_, b_
        for op, fn in self.exact.items():
            for name, (g_, r_) in fn().items():
                got[name], ref[name], bnd[name] = g_, r_, None
        if self.extra is not None:
            for d, e in zip((got, ref, bnd), self.extra()):
                d.update(e)
        return got, ref, bnd


def dev(t):
    return None if t is None else t.to(DEV)


# ---- conv and weight-gradient lanes: the launches of tests/test_small_conv_families_gpu.py / test_k3_conv_families_gpu.py -----------------------------------------
def fwd_lane(e, lane, finalize=False):
    c, dt = gc.conv_case(e["mod"], e["name"]), e["dt"]
    dtype = gc.DT[dt]
    inp = gc.conv_inputs(e, lane)
    ln = Lane(dtype, c["knobs"] if e["mod"] == "kc" else {})
    bias, shift = dev(inp["bias"]), dev(inp["shift"])
    if e["mod"] == "kc":
        srcs = sources(c, inp["srcs"], dtype)
        wp = ops.pack_weights(inp["w"].to(DEV), c["kind"], dtype, *kc.pack_args(c))
        M = Cl = c["cout"]
        D, H, W = kc.spatial(c)
        outs = kc.new_outs(c, dt, DEV)
        if c["out"] == "planar":
            out, kw = outs[0][1], dict(out_planar=True, out_f32=True)
        elif c["out"] == "out2":
            out = outs[0][1][..., :M // 2]
            kw = dict(out_ld=M // 2 + sc.SLOT_EXTRA, out_coff=sc.SLOT_COFF, out2=outs[1][1][..., :M // 2])
        else:
            out = outs[0][1]
            kw = dict(out_ld=out.shape[-1], out_coff=sc.SLOT_COFF)
        kw.update(grid=(c["N"], D, H, W), in_dims=(D, H, W), ksize=3, stride=1, dims=c["dims"], combine=int(c["arr"] == "add"))
    else:
        srcs = [lazy_of(s, dtype) for s in inp["srcs"]]
        wp = ops.pack_weights(inp["w"].to(DEV), c["kind"], dtype, *sc.pack_args(c))
        Cl, M = sc.launch_cout(c), c["cout"]
        outs = [sc.new_out(c, dtype, DEV)]
        out = outs[0][1]
        k = 2 if c["op"] == "k2" else 1
        kw = dict(out_planar=True, out_f32=True) if c["op"] == "head" else dict(out_ld=out.shape[-1], out_coff=sc.SLOT_COFF)
        if c["op"] == "d2s":
            kw.update(out_mode=1, out_cn=M)
        kw.update(grid=(c["N"],) + g4(c["grid"]), in_dims=g4(sc.in_spatial(c)), ksize=k, stride=k, dims=c["dims"])
    for i, (flat, _) in enumerate(outs):
        ln.plain("flat%d" % i, flat)
    stats = ln.plain("stats", torch.full((ops.stats_size(Cl),), NAN, device=DEV)) if c["stats"] else None
    ln.keep = (srcs, wp, bias, shift)
    ln.call("conv_fwd", srcs, wp, bias, Cl, out, stats=stats, stats_shift=shift, writes=["flat%d" % i for i in range(len(outs))] + (["stats"] if c["stats"] else []), **kw)
    ln.exact["conv_fwd"] = dict
    if finalize:                                            # the layer's BatchNorm behind it: reads the slots the conv wrote
        assert c["stats"] and Cl == M
        gen = torch.Generator().manual_seed(900 + lane)
        gam, bet = dev(torch.rand(M, generator=gen) + 0.5), dev(torch.randn(M, generator=gen) * 0.2)
        o = {k_: ln.out(k_, (M,), torch.float32) for k_ in ("scale", "shift", "mean", "invstd")}
        n, sp = kc.images(c) if e["mod"] == "kc" else (c["N"], c["grid"])
        ln.call("bn_finalize", stats, gam, bet, None, None, None, n * math.prod(sp), 1e-5, 0.0, o["scale"], o["shift"], mean=o["mean"], invstd=o["invstd"],
                stats_shift=shift, writes=list(o))

    def views():
        r = gc.conv_reference(e, inp)
        totals = ops.stats_totals(stats, Cl, M).cpu() if c["stats"] else None
        return gc.fwd_views(e, r, [f.cpu() for f, _ in outs], totals)
    ln.extra = views
    return ln.ready()


def wgrad_lane(e, lane):
    c, dt = gc.conv_case(e["mod"], e["name"]), e["dt"]
    dtype = gc.DT[dt]
    inp = gc.conv_inputs(e, lane)
    ln = Lane(dtype, c["knobs"] if e["mod"] == "kc" else {})
    n, knv = inp["prior_dw"].numel(), inp["knv"]
    buf = ln.plain("dw", torch.full((n + sc.GUARD,), NAN, device=DEV))           # dW with a NaN guard behind it
    dw = buf[:n].view(inp["prior_dw"].shape)
    dw.copy_(inp["prior_dw"])
    dbuf = db = None
    if c["db"]:
        dbuf = ln.plain("db", torch.full((knv + sc.GUARD,), NAN, device=DEV))
        db = dbuf[:knv]
        db.copy_(inp["prior_db"])
    if e["mod"] == "kc":
        As, B = sources(c, inp["As"], dtype), sources(c, [inp["B"]], dtype)[0]
        D, H, W = kc.spatial(c)
        kw = dict(grid=(c["N"], D, H, W), in_dims=(D, H, W), ksize=3, stride=1, dims=c["dims"], combine=int(c["arr"] == "add"), kc_valid=c["kc_valid"])
    else:
        As, B = [lazy_of(inp["A"], dtype)], lazy_of(inp["B"], dtype)
        ks = c["ks"]
        kw = dict(grid=(c["N"],) + g4(c["grid"]), in_dims=g4(tuple(ks * s for s in c["grid"])), ksize=ks, stride=ks, dims=c["dims"])
    ln.call("wgrad", As, B, dw, inp["strides"], db=db, kn_valid=c["kn_valid"], writes=["dw"] + (["db"] if c["db"] else []), **kw)
    ln.exact["wgrad"] = dict

    def views():
        rw = gc.conv_reference(e, inp)
        return gc.wgrad_views(e, rw, inp, dw.cpu(), None if db is None else db.cpu(), buf[n:].cpu(), None if dbuf is None else dbuf[knv:].cpu())
    ln.extra = views
    return ln.ready()


# ---- the other families ------------------------------------------------------------------------------------------------------------------------------------------------
def other_lane(c, lane):
    dt, k = c["dt"], c["kind"]
    dtype = gc.DT[dt]
    inp = gc.other_inputs(c, lane)
    ln = Lane(dtype)
    f32 = torch.float32
    if k == "c1f":
        N, D, H, W = c["shape"]
        out = ln.out("out", (N, D, H, W, 16), dtype)
        stats = ln.out("stats", (ops.stats_size(16),), f32)
        x, w, b, c0 = dev(inp["x"]), dev(inp["w"]), dev(inp["b"]), dev(inp["c0"])
        ln.call("conv_c1_fwd", x, w, b, out, dims=c["dims"], stats=stats, stats_shift=c0, writes=("out", "stats"))
        if c.get("env"):
            # the scalar kernel in bf16 (CHAP_C1_MFMA=0) is the fp32 kernel's arithmetic with a bf16 store: it reads the fp32 image and the fp32 weights as
            # they are (conv_c1_fwd_kernel<T, ...>: only the st8 depends on T), where the MFMA kernel, and the Checker's restatement of the product path,
            # round both to bf16 first.  So: kernel_ref.conv_ref on the UNROUNDED operands, kernel_ref.conv_bound with the bf16 store, the same error model.
            ln.exact["conv_c1_fwd"] = dict

            def views():
                a = x.unsqueeze(1).double()
                r = kr.conv_ref(kr.PACK_CONV_FWD, a[:, :, 0] if c["dims"] == 2 else a, kr.weight_operand(inp["w"], torch.float32).to(DEV), b)
                (s1, b1), (s2, b2) = kr.stats_ref(r, c0)
                st = ops.stats_totals(stats, 16)
                got = {"out": nc(out, c["dims"]).double().cpu(), "S": st[0].cpu(), "Q": st[1].cpu()}
                return got, {"out": r["y"].cpu(), "S": s1.cpu(), "Q": s2.cpu()}, {"out": kr.conv_bound(r, dtype).cpu(), "S": b1.cpu(), "Q": b2.cpu()}
            ln.extra = views
    elif k == "c1b":
        N, D, H, W = c["shape"]
        dx = ln.out("dx", (N, D, H, W), f32)
        dw = ln.out("dw", tuple(inp["w"].shape), f32, init=inp["prior_dw"])
        db = ln.out("db", (16,), f32, init=inp["prior_db"])
        ln.call("conv_c1_bwd", cl(inp["g"], dtype), dev(inp["w"]), dev(inp["x"]), dims=c["dims"], dx=dx, dw=dw, db=db, writes=("dx", "dw", "db"))
    elif k == "bnfin":
        C, nsub, ns = c["C"], c["nsub"], c["nslots"]
        st = torch.full((ops.stats_size(C * nsub),), NAN)
        st[:L.STATS_HDR] = 0
        st[:1].view(torch.int32).fill_(ns)
        body = st[L.STATS_HDR:L.STATS_HDR + ns * 2 * C * nsub].view(ns, 2, C * nsub)
        body[:, 0], body[:, 1] = inp["S"], inp["Q"]
        o = {n: ln.out(n, (C,), f32) for n in ("scale", "shift", "mean", "invstd")}
        rm, rv = ln.out("rm", (C,), f32, init=inp["rm"]), ln.out("rv", (C,), f32, init=inp["rv"])
        nbt = ln.plain("nbt", torch.full((1,), 5, dtype=torch.int64, device=DEV))
        ln.call("bn_finalize", dev(st), dev(inp["gamma"]), dev(inp["beta"]), rm, rv, nbt, inp["count"], 1e-5, 0.1, o["scale"], o["shift"], mean=o["mean"],
                invstd=o["invstd"], stats_shift=dev(inp["shift"]), clog=C * nsub, writes=list(o) + ["rm", "rv", "nbt"])
    elif k == "bneval":
        C = c["C"]
        ln.call("bn_eval_affine", dev(inp["gamma"]), dev(inp["beta"]), dev(inp["rm"]), dev(inp["rv"]), 1e-5, ln.out("scale", (C,), f32), ln.out("shift", (C,), f32),
                writes=("scale", "shift"))
    elif k == "pool":
        N, D, H, W = c["shape"]
        oshape = (N, max(D // 2, 1), H // 2, W // 2, c["C"])
        ln.call("act_pool2", lazy_of(inp["src"], dtype), ln.out("out", oshape, dtype), ln.out("idx", oshape, torch.uint8, fill=0xAB), dims=3 if D > 1 else 2,
                writes=("out", "idx"))
    elif k == "up":
        N, D, H, W = c["shape"]
        C = c["C"]
        ld = 2 * C if c["slot"] else C
        out = ln.out("out", (N, 2 * D if c["dims"] == 3 else D, 2 * H, 2 * W, ld), dtype)
        ln.call("upsample2x", lazy_of(inp["src"], dtype), out, dims=c["dims"], out_coff=ld - C, half_pixel=bool(c["hp"]), writes=("out",))
    elif k == "upbwd":
        N, D, H, W = c["shape"]
        ln.call("upsample2x_bwd", cl(inp["g"], dtype), 0, c["C"], ln.out("out", (N, D, H, W, c["C"]), dtype), dims=c["dims"], writes=("out",))
    elif k == "actbwd":
        N, D, H, W = c["shape"]
        C = c["C"]
        gout = ln.out("gout", (N, D, H, W, C), dtype)
        sums = ln.out("sums", (ops.act_bwd_sums_size(C),), f32)
        dgamma, dbeta = ln.out("dgamma", (C,), f32, init=inp["prior"][0]), ln.out("dbeta", (C,), f32, init=inp["prior"][1])
        kw = dict(g_pool=cl(inp["gp"], dtype), pool_idx=cl(inp["idx"], torch.uint8)) if c["pool"] else {}
        ln.call("act_bwd", lazy_of(inp["src"], dtype), [(cl(t, dtype), 0) for t in inp["grads"]], gout, mean=dev(inp["mean"]), invstd=dev(inp["invstd"]),
                gamma=dev(inp["gamma"]), dgamma=dgamma, dbeta=dbeta, count=inp["count"], bn_mode=1, sums=sums, writes=("gout", "sums", "dgamma", "dbeta"), **kw)
    elif k == "p2cl":
        out = ln.out("out", (2, 3, 9, 7, c["ld"]), dtype)
        ln.call("planar_to_cl", dev(inp["x"]), out, out_coff=c["coff"], cpad=c["cpad"], writes=("out",))
        out0 = torch.full((2, 3, 9, 7, c["ld"]), NAN, dtype=dtype)
        ln.exact["planar_to_cl"] = lambda: {"planar_to_cl": (out.cpu(), kr.planar_to_cl_ref(inp["x"], out0, c["coff"], c["cpad"]))}
    elif k == "cl2p":
        ln.call("cl_to_planar", lazy_of(inp["src"], dtype), ln.out("out", (2, c["C"]) + gc.RES_SP, f32), writes=("out",))
    elif k == "chansum":
        ln.call("channel_sum", lazy_of(inp["src"], dtype), ln.out("out", (c["C"],), f32, init=inp["prior"]), writes=("out",))
    elif k == "chansum_big":
        lz = ops.Lazy(big_raw(c), dev(inp["scale"]), dev(inp["shift"]), True, sc.SLOPE, C=c["C"], coff=inp["coff"])
        ln.call("channel_sum", lz, ln.out("out", (c["C"],), f32, init=inp["prior"]), writes=("out",))
    elif k == "keepmask":
        keep = ln.out("keep", (c["n"],), torch.uint8, fill=0xAB)
        ln.call("keep_mask", keep, inp["seed"], c["p"], writes=("keep",))
        ln.exact["keep_mask"] = lambda: {"keep_mask": (keep.cpu(), kr.keep_mask_ref(inp["seed"], c["n"], c["p"]))}
    elif k == "chanmask":
        mul = ln.out("mul", (c["n"],), f32)
        ln.call("chan_mask", mul, inp["seed"], c["p"], writes=("mul",))
        ln.exact["chan_mask"] = lambda: {"chan_mask": (mul.cpu(), kr.chan_mask_ref(inp["seed"], c["n"], c["p"]))}
    elif k == "fold":
        B, U, C = c["B"], c["U"], c["C"]
        gfull = torch.full((B + U, 1, 5, 7, C + 16), 1e30, device=DEV, dtype=dtype)
        gfull[..., 8:8 + C] = cl(inp["g"], dtype)
        ln.call("fold_perturbed", gfull, 8, C, dev(inp["mul"]), B, U, writes=())
    elif k == "resfwd":
        C = c["C"]
        rl = ops.Lazy(cl(inp["r"], dtype), dev(inp["rs"]), dev(inp["rb"]), False)
        srcs = [] if c["nsrc"] == 0 else [lazy_of(inp["a"], dtype), lazy_of(inp["b"], dtype)]
        xin = dev(inp["xin"].reshape(2, -1)) if c["nsrc"] == 0 else None
        ln.call("residual_fwd", rl, srcs, ln.out("out", (2,) + gc.RES_SP + (C,), dtype), xin=xin, writes=("out",))
    elif k == "resbwd":
        C = c["C"]
        gout = ln.out("gout", (2,) + gc.RES_SP + (C,), dtype)
        dxin = ln.out("dxin", (2, math.prod(gc.RES_SP)), f32) if c["dxin"] else None
        ln.call("residual_bwd", [(cl(t, dtype), 0) for t in inp["grads"]], cl(inp["o"], dtype), gout, chan_mul=dev(inp["cm"]), dxin=dxin,
                writes=("gout", "dxin") if c["dxin"] else ("gout",))
    elif k == "gradsum":
        ln.call("grad_sum", [(cl(t, dtype), 0) for t in inp["grads"]], ln.out("out", (2,) + gc.RES_SP + (c["C"],), dtype), writes=("out",))
    else:
        raise KeyError(k)
    return ln.ready()


_BIG = {}


def big_raw(c):
    """the 4 GiB source of the chansum_big cases, [N, 1, H, W, 512] in the case's dtype: drawn once per dtype on the device (group_cases.BIG_SEED), shared
    by the lanes and by the single and the merged run (the kernel only reads it); the other dtype's is dropped first"""
    if c["dt"] not in _BIG:
        _BIG.clear()
        torch.cuda.empty_cache()
        gen = torch.Generator(device=DEV).manual_seed(gc.BIG_SEED)
        raw = torch.empty(tuple(c["shape"]) + (c["ld"],), device=DEV, dtype=gc.DT[c["dt"]])
        for n in range(raw.shape[0]):                       # (sample by sample: 2^29 to 2^30 elements per draw)
            raw[n].normal_(generator=gen)
        _BIG[c["dt"]] = raw
    return _BIG[c["dt"]]


@pytest.fixture(scope="module", autouse=True)
def _release_big():
    yield
    _BIG.clear()
    torch.cuda.empty_cache()


def make_lane(cid, lane, **kw):
    if cid in gc.CONV_BY_ID:
        e = gc.CONV_BY_ID[cid]
        return fwd_lane(e, lane, **kw) if gc.is_fwd(e) else wgrad_lane(e, lane)
    return other_lane(gc.OTHER_BY_ID[cid], lane)


def positions(cid):
    if cid in gc.CONV_BY_ID:
        return 1 if gc.is_fwd(gc.CONV_BY_ID[cid]) else 2    # the weight gradient: the kernel and its reduce
    return gc.OTHER_BY_ID[cid]["positions"]


# ---- running ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def run_single(lanes):
    with device_alive():
        for ln in lanes:
            ln.run()
        torch.cuda.synchronize()


def run_region(lanes):
    """all lanes inside ONE region; returns the number of grids it issued"""
    before = L.group.launched
    with device_alive():
        with L.group(torch.cuda.current_stream().cuda_stream) as region:
            for i, ln in enumerate(lanes):
                if i:
                    region.next_lane()
                ln.run()
        torch.cuda.synchronize()
    assert L.group.held is None
    return L.group.launched - before


def results(lanes):
    res, refs, bounds = [], [], []
    for ln in lanes:
        raw = ln.tensors()
        got, ref, bnd = ln.verify()
        res.append(dict(raw, **got))
        refs.append(ref)
        bounds.append(bnd)
    return res, refs, bounds


def run_and_check(who, spec, want_grids, differ=True):
    """spec: [(case id, lane seed, kwargs)] per lane.  Single launches, then one region; check_lanes; returns (grids, worst error / bound)."""
    single = [make_lane(cid, seed, **kw) for cid, seed, kw in spec]
    grouped = [make_lane(cid, seed, **kw) for cid, seed, kw in spec]
    run_single(single)
    grids = run_region(grouped)
    s_res, _, _ = results(single)
    g_res, refs, bounds = results(grouped)
    worst = gc.check_lanes(s_res, g_res, refs, bounds, who, differ=differ)
    assert grids == want_grids, (who, "grids issued", grids, "expected", want_grids)
    return grids, worst


def report(**kw):
    print("groupcase " + json.dumps(kw))


@pytest.mark.parametrize("lanes", gc.LANES)
@pytest.mark.parametrize("cid", gc.HERE_CASE_IDS)
def test_merged_case(cid, lanes):
    t0 = time.perf_counter()
    grids, worst = run_and_check(cid, [(cid, k, {}) for k in range(lanes)], positions(cid))      # everything merged: one grid per recorded position
    report(case=cid, lanes=lanes, grids=grids, bit_equal=True, worst=round(worst, 4), seconds=round(time.perf_counter() - t0, 3))


# ---- the cases under a knob that is read once per process: ONE child process that has it set from its start runs them all ------------------------------------------------
def _child_main():
    """the child: every (case with an `env`, lanes) through run_and_check; one GROUPCHILD line with the outcomes.  Exit code 3: a runtime error"""
    out = {}
    try:
        for cid in gc.ENV_CASE_IDS:
            assert all(os.environ.get(k) == v for k, v in gc.OTHER_BY_ID[cid]["env"].items()), cid
            for lanes in gc.LANES:
                t0 = time.perf_counter()
                try:
                    grids, worst = run_and_check(cid, [(cid, k, {}) for k in range(lanes)], positions(cid))
                    out["%s-%d" % (cid, lanes)] = dict(ok=True, grids=grids, worst=round(worst, 4), seconds=round(time.perf_counter() - t0, 3))
                except AssertionError as e:
                    out["%s-%d" % (cid, lanes)] = dict(ok=False, err=str(e)[:3000])
    except BaseException as e:                                # (pytest.exit of device_alive among them)
        print("child: %s: %s" % (type(e).__name__, e), file=sys.stderr)
        sys.exit(3)
    print("GROUPCHILD " + json.dumps(out))


@pytest.fixture(scope="module")
def env_child():
    env = dict(os.environ, **gc.OTHER_BY_ID[gc.ENV_CASE_IDS[0]]["env"])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=gc.ROOT, capture_output=True, text=True, timeout=300)
    if r.returncode == 3:
        pytest.exit("the child process met a runtime error: %s" % r.stderr[-2000:], returncode=3)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("GROUPCHILD ")][-1][len("GROUPCHILD "):])


@pytest.mark.parametrize("lanes", gc.LANES)
@pytest.mark.parametrize("cid", gc.ENV_CASE_IDS)
def test_merged_case_under_a_read_once_knob(env_child, cid, lanes):
    res = env_child["%s-%d" % (cid, lanes)]
    assert res["ok"], res.get("err")
    report(case=cid, lanes=lanes, grids=res["grids"], bit_equal=True, worst=res["worst"], seconds=res["seconds"], env=gc.OTHER_BY_ID[cid]["env"])


# ---- the lane-count rules, on three chains: a ragged generic conv with statistics + its bn_finalize; a base_z = 2 weight gradient + its reduce; act_bwd reduce + sum + apply
# chain: (case, lane kwargs, recorded positions, a case of another shape, the same shape in fp32, grids of bf16 + fp32 lanes).  The last: the kernels that
# read the operand type are other instances per dtype (two grids), bn_finalize, the weight-gradient reduce and the act_bwd sum work on fp32 alone (one grid)
CHAINS = {"conv_finalize": ("kc:g2_16_20_n2m2:bf16", dict(finalize=True), 2, "kc:g2_16_16_n1m1:f32", "kc:g2_16_20_n2m2:f32", 2 + 1),
          "wgrad_reduce": ("kc:w2_16_40:bf16", {}, 2, "kc:w2_16_16:f32", "kc:w2_16_40:f32", 2 + 1),
          "act_bwd": ("actbwd_gen_bf16", {}, 3, "actbwd_one_f32", "actbwd_gen_twin_f32", 2 + 1 + 2)}


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_three_lanes(chain):
    cid, kw, npos = CHAINS[chain][:3]
    grids, worst = run_and_check(chain + " x3", [(cid, k, kw) for k in range(3)], npos)
    report(case=chain, rule="3 lanes", lanes=3, grids=grids, bit_equal=True, worst=round(worst, 4))


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_five_lanes_split_four_and_one(chain):
    cid, kw, npos = CHAINS[chain][:3]
    grids, worst = run_and_check(chain + " x5", [(cid, k, kw) for k in range(5)], 2 * npos)      # CHAP_MAX_LANES = 4: every position as 4 + 1
    report(case=chain, rule="5 lanes = 4 + 1", lanes=5, grids=grids, bit_equal=True, worst=round(worst, 4))


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_a_b_a_merges_the_two_a(chain):
    cid, kw, npos, other = CHAINS[chain][:4]
    okw = dict(finalize=True) if chain == "conv_finalize" else {}
    grids, worst = run_and_check(chain + " A-B-A", [(cid, 0, kw), (other, 1, okw), (cid, 2, kw)], 2 * npos)      # A + A as one grid, B alone
    report(case=chain, rule="A-B-A", lanes=3, grids=grids, bit_equal=True, worst=round(worst, 4))


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_same_shape_in_the_other_dtype_is_not_merged(chain):
    cid, kw, npos, _, twin, want = CHAINS[chain]
    grids, worst = run_and_check(chain + " A-B dtype", [(cid, 0, kw), (twin, 1, kw)], want)
    report(case=chain, rule="A-B other dtype", lanes=2, grids=grids, bit_equal=True, worst=round(worst, 4))


def test_lanes_of_unequal_length():
    """lane 0: conv + finalize, lane 1: the conv only -- the convs merge, the finalize goes alone"""
    cid = CHAINS["conv_finalize"][0]
    grids, worst = run_and_check("unequal", [(cid, 0, dict(finalize=True)), (cid, 1, {})], 2)
    report(case="conv_finalize", rule="unequal length", lanes=2, grids=grids, bit_equal=True, worst=round(worst, 4))


# ---- refusals: an entry point that launches directly fails inside a region and the region is left ---------------------------------------------------------------------------
def _direct_calls():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    N, C, H, W = 2, 2, 8, 12
    logits, logits2 = r(N, C, H, W), r(N, C, H, W)
    tgt = torch.randint(0, C, (N, H, W), generator=g).to(DEV)
    soft = torch.softmax(r(N, C, H, W), 1).contiguous()
    mask = torch.ones(N, H, W, dtype=torch.int64, device=DEV)
    box = torch.tensor([1, 2, 5, 8], dtype=torch.int32, device=DEV)
    imask = lambda: torch.empty(N, H, W, dtype=torch.int64, device=DEV)
    img = r(N, 1, H, W)
    lr = torch.full((1,), 0.1, device=DEV)
    calls = {
        "sgd_step": lambda: ops.sgd_step(torch.zeros(64, device=DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV), lr, 0.9, 0.0),
        "sgd_ema_step": lambda: ops.sgd_ema_step(torch.zeros(64, device=DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV), lr, 0.9, 0.0,
                                                 torch.zeros(64, device=DEV), torch.tensor([0.99, 0.01], device=DEV)),
        "rand_uniform": lambda: ops.rand_uniform(torch.empty(100, device=DEV), 7),
        "perturb": lambda: ops.perturb(r(100), r(100), torch.empty(100, device=DEV), 0.5),
        "l2_normalize": lambda: ops.l2_normalize(r(2, 1, 8, 12), torch.empty(2, 1, 8, 12, device=DEV)),
        "grad_sim": lambda: ops.grad_sim(r(16, 16, 3, 3), r(16, 16, 3, 3), torch.zeros(16, device=DEV)),
        "mix_loss_fwd": lambda: ops.mix_loss_fwd(logits, tgt, tgt, mask, 1.0, 0.5),
        "mix_loss_multi_fwd": lambda: ops.mix_loss_multi_fwd([dict(logits=logits, target_a=tgt, target_b=tgt, mask=mask, w_a=1.0, w_b=0.5)]),
        "pseudo_block": lambda: ops.pseudo_block(logits, logits2),
        "kl_fwd_bwd": lambda: ops.kl_fwd_bwd((logits, logits2), (soft, soft), torch.zeros(1, device=DEV), (torch.empty_like(logits), torch.empty_like(logits2))),
        "largest_cc": lambda: ops.largest_cc(tgt, C),
        "diff_mask": lambda: ops.diff_mask(tgt, torch.roll(tgt, 1, 2).contiguous(), torch.rand(N, H, W, generator=g).to(DEV), 4, 0.5),
        "box_mask": lambda: ops.box_mask(imask(), box),
        "box_mix": lambda: ops.box_mix(img, r(N, 1, H, W), torch.empty_like(img), box),
        "bcp_mix": lambda: ops.bcp_mix(img, r(N, 1, H, W), torch.empty_like(img), r(N, 1, H, W), r(N, 1, H, W), torch.empty_like(img), imask(), box),
        "sample_channel_sum": lambda: ops.sample_channel_sum(ops.Lazy(r(2, 1, 5, 6, 8)), nchunk=4),
        "ensemble_argmax": lambda: ops.ensemble_argmax(logits, logits2, "prob_ensemble"),
        "pack_weights": lambda: ops.pack_weights(r(16, 16, 3, 3), L.PACK_CONV_FWD, torch.bfloat16, 16, 16, 9),
    }
    u = torch.rand(2, 16, generator=g).to(DEV)
    calls["channel_drop"] = lambda: ops.channel_drop(torch.empty(4, 16, device=DEV), torch.empty(4, 16, device=DEV), u, u.clone(), 2, "dropout2d")
    score, cnt = torch.zeros(C, 6, 5, 4, device=DEV), torch.zeros(6, 5, 4, device=DEV)
    origins = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    calls["window_accumulate"] = lambda: ops.window_accumulate(r(1, C, 4, 4, 4), origins, score, cnt)
    calls["window_accumulate_heads"] = lambda: ops.window_accumulate_heads([r(1, C, 4, 4, 4), r(1, C, 4, 4, 4)], origins, score, cnt)
    calls["window_gather"] = lambda: ops.window_gather(r(6, 5, 4), origins, (4, 4, 4))
    calls["window_finalize"] = lambda: ops.window_finalize(score, cnt + 1)
    # the backward forms of the losses: the accumulators of a forward call made here, outside any region
    _, acc = ops.mix_loss_fwd(logits, tgt, tgt, mask, 1.0, 0.5)
    calls["mix_loss_bwd"] = lambda: ops.mix_loss_bwd(logits, tgt, tgt, mask, 1.0, 0.5, acc, torch.empty_like(logits))
    calls["mix_loss_multi_bwd"] = lambda: ops.mix_loss_multi_bwd([dict(logits=logits, target_a=tgt, target_b=tgt, mask=mask, w_a=1.0, w_b=0.5, acc=acc,
                                                                       dlogits=torch.empty_like(logits))])
    # metrics as chap_amd.metrics calls them (binary masks, one 2D slice, with distances)
    ma = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    ma[0, 2:6, 1:5] = 1
    mb = torch.roll(ma, 1, 2).contiguous()
    calls["metrics"] = lambda: ops.metrics(ma, mb, None, ndim=2, binary=True, distances=True)
    # the augmentation kernels through the device-resident loader, which builds their records
    import numpy as np
    from chap_amd.data import DeviceLoader, SliceStore, VolumeStore
    rng = np.random.default_rng(3)
    sl = SliceStore([rng.random((20, 24), dtype=np.float32) for _ in range(4)], [rng.integers(0, 3, (20, 24)).astype(np.uint8) for _ in range(4)], DEV)
    vol = VolumeStore([rng.random((12, 12, 10), dtype=np.float32) for _ in range(4)], [rng.integers(0, 2, (12, 12, 10)).astype(np.uint8) for _ in range(4)], DEV)
    l2d = DeviceLoader(sl, range(2), range(2, 4), 2, 1, (16, 16), seed=1)
    l3d = DeviceLoader(vol, range(2), range(2, 4), 2, 1, (8, 8, 8), seed=1)
    l3p = DeviceLoader(vol, range(2), range(2, 4), 2, 1, (8, 8, 8), seed=1, pad=True)
    i2, b2 = torch.empty(2, 1, 16, 16, device=DEV), torch.empty(2, 16, 16, dtype=torch.int64, device=DEV)
    i3, b3 = torch.empty(2, 1, 8, 8, 8, device=DEV), torch.empty(2, 8, 8, 8, dtype=torch.int64, device=DEV)
    calls["augment2d"] = lambda: l2d.next_into(i2, b2)
    calls["augment3d"] = lambda: l3d.next_into(i3, b3)
    calls["augment3d_padded"] = lambda: l3p.next_into(i3, b3)
    return calls


DIRECT = ("sgd_step", "sgd_ema_step", "rand_uniform", "perturb", "l2_normalize", "grad_sim", "mix_loss_fwd", "mix_loss_multi_fwd", "pseudo_block", "kl_fwd_bwd",
          "largest_cc", "diff_mask", "box_mask", "box_mix", "bcp_mix", "sample_channel_sum", "ensemble_argmax", "pack_weights", "channel_drop", "window_accumulate",
          "window_accumulate_heads", "window_gather", "window_finalize", "mix_loss_bwd", "mix_loss_multi_bwd", "metrics", "augment2d", "augment3d", "augment3d_padded")


@pytest.fixture(scope="module")
def direct_calls():
    with device_alive():                                    # (it launches: the forward loss for the backward forms' accumulators, the stores' uploads)
        calls = _direct_calls()
        torch.cuda.synchronize()
    assert set(calls) == set(DIRECT)
    return calls


@pytest.mark.parametrize("name", DIRECT)
def test_direct_launch_is_refused_inside_a_region(direct_calls, name):
    call = direct_calls[name]
    with device_alive():
        call()                                              # outside a region the call is valid
        torch.cuda.synchronize()
    with device_alive():
        with pytest.raises(L.ChapError, match="chap_group"):
            with L.group(torch.cuda.current_stream().cuda_stream):
                call()
        torch.cuda.synchronize()
    assert L.group.held is None                             # the region was left
    n0 = L.group.launched
    with L.group(torch.cuda.current_stream().cuda_stream):      # and nothing of it is left behind: the next region starts empty
        pass
    assert L.group.launched == n0


if __name__ == "__main__":
    _child_main()
