"""The 3x3(x3) stride-1 conv and weight-gradient kernels on small ragged grids, one launch per (case, dtype) of tests/k3_conv_cases.py: every
conv_fwd_kernel / conv_wp_kernel / conv_kpar(2d)_kernel / wgrad_kernel / wgrad_wp_kernel instance the bench-shaped steps launch and the blockings only
the lab knobs reach (tests/test_k3_conv_cases_cpu.py proves which case reaches which instance), per element against the fp64 restatements of
tests/kernel_ref.py under their own bounds.  Lazy, concatenated (with a K chunk that straddles the sources) and add-combined sources, bias, shifted
statistics, outputs in a channel slot of a wider NaN buffer with a NaN guard behind it, which must come back untouched; the `trip` cases assert from the
statistics header that a persistent block owned at least two pixel tiles; the weight-gradient cases force the tile dealing (one split, splits with several
tiles, splits with none) through CHAP_WGRAD_BLOCKS.  Each case prints one `k3case {json}` line with its worst error / bound.  Needs a GPU."""
import json
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import ops
from tests import k3_conv_cases as kc
from tests import small_conv_cases as sc
from tests.plan_probe import KNOBS
from tests.test_small_conv_families_gpu import DEV, lazy_of


def sources(c, srcs, dtype):
    """the sources of small_conv_cases.make_source on the device; dims = 2 with D > 1: the N * D images as [N, D, H, W, C]"""
    out = []
    for s in srcs:
        lz = lazy_of(s, dtype)
        if kc.slices(c):
            shape = (c["N"],) + tuple(c["grid"])
            lz.raw = lz.raw.view(shape + (-1,))
            if lz.keep is not None:
                lz.keep = lz.keep.view(shape + (-1,))
        out.append(lz)
    return out


def set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))


class device_alive:
    """launch and synchronise inside: an error of the runtime there (not a failed check) ends the whole session, so that nothing more is started on a
    device that has faulted"""
    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is not None and not issubclass(et, AssertionError):
            pytest.exit("the launch failed in the runtime: %s: %s" % (et.__name__, ev), returncode=3)
        return False


def report(kind, name, dt, instance, worst, t0, **more):
    print("k3case " + json.dumps(dict(kind=kind, case=name, dtype=dt, instance=instance, worst=[round(v, 4) for v in worst], seconds=round(time.perf_counter() - t0, 3), **more)))


@pytest.mark.parametrize("name,dt", kc.FWD_IDS)
def test_forward_case(name, dt, monkeypatch):
    t0 = time.perf_counter()
    c, dtype = kc.BY_NAME[name], kc.DTYPES[dt]
    inp = kc.fwd_inputs(c, dt)
    srcs = sources(c, inp["srcs"], dtype)
    wp = ops.pack_weights(inp["w"].to(DEV), c["kind"], dtype, *kc.pack_args(c))
    M = c["cout"]
    D, H, W = kc.spatial(c)
    bias = None if inp["bias"] is None else inp["bias"].to(DEV)
    shift = None if inp["shift"] is None else inp["shift"].to(DEV)
    r = kc.fwd_reference(c, dt, inp)
    t_ref = time.perf_counter() - t0
    # (the K-parallel cases: once on their route, once with CHAP_CONV_KPAR = 0 on the generic kernel, both against the same reference)
    for knobs in ([c["knobs"], dict(c["knobs"], CHAP_CONV_KPAR=0)] if c["route"] == "kpar" else [c["knobs"]]):
        set_knobs(monkeypatch, knobs)
        outs = kc.new_outs(c, dt, DEV)
        stats = ops.stats_buffer(M, DEV) if c["stats"] else None
        if c["out"] == "planar":
            kw = dict(out_planar=True, out_f32=True)
            out = outs[0][1]
        elif c["out"] == "out2":
            h = M // 2
            out = outs[0][1][..., :h]
            kw = dict(out_ld=h + sc.SLOT_EXTRA, out_coff=sc.SLOT_COFF, out2=outs[1][1][..., :h])
        else:
            out = outs[0][1]
            kw = dict(out_ld=out.shape[-1], out_coff=sc.SLOT_COFF)
        with device_alive():
            ops.conv_fwd(srcs, wp, bias, M, out, grid=(c["N"], D, H, W), in_dims=(D, H, W), ksize=3, stride=1, dims=c["dims"], combine=int(c["arr"] == "add"),
                         stats=stats, stats_shift=shift, **kw)
            torch.cuda.synchronize()
        totals = ops.stats_totals(stats, M).cpu() if c["stats"] else None
        worst = kc.fwd_check(c, dt, r, [f.cpu() for f, _ in outs], totals)
        more = {}
        if c["stats"]:
            slots = int(stats[:1].view(torch.int32).item())
            more = dict(tiles=kc.pixel_tiles(c, dt), slots=slots)
            if c["trip"] and knobs is c["knobs"]:
                assert kc.pixel_tiles(c, dt) >= 2 * slots, (name, dt, "no block owned two tiles", more)
        report("fwd", name, dt, kc.fwd_instance(c, dt) if knobs is c["knobs"] else "generic (CHAP_CONV_KPAR=0)", worst, t0, ref_seconds=round(t_ref, 3), **more)


@pytest.mark.parametrize("name,dt", kc.WGRAD_IDS)
def test_weight_gradient_case(name, dt, monkeypatch):
    t0 = time.perf_counter()
    c, dtype = kc.BY_NAME[name], kc.DTYPES[dt]
    set_knobs(monkeypatch, c["knobs"])
    inp = kc.wgrad_inputs(c, dt)
    As, B = sources(c, inp["As"], dtype), sources(c, [inp["B"]], dtype)[0]
    n = inp["prior_dw"].numel()
    buf = torch.full((n + sc.GUARD,), float("nan"), device=DEV)                 # dW with a NaN guard behind it
    dw = buf[:n].view(inp["prior_dw"].shape)
    dw.copy_(inp["prior_dw"])
    dbuf = None
    if c["db"]:
        dbuf = torch.full((inp["knv"] + sc.GUARD,), float("nan"), device=DEV)
        dbuf[:inp["knv"]] = inp["prior_db"].to(DEV)
    D, H, W = kc.spatial(c)
    with device_alive():
        ops.wgrad(As, B, dw, inp["strides"], grid=(c["N"], D, H, W), in_dims=(D, H, W), ksize=3, stride=1, dims=c["dims"], combine=int(c["arr"] == "add"),
                  db=None if dbuf is None else dbuf[:inp["knv"]], kc_valid=c["kc_valid"], kn_valid=c["kn_valid"])
        torch.cuda.synchronize()
    rw = kc.wgrad_reference(c, dt, inp)
    worst = kc.wgrad_check(c, dt, rw, inp, dw.cpu(), None if dbuf is None else dbuf[:inp["knv"]].cpu())
    assert bool(torch.isnan(buf[n:]).all()), name + ": the guard behind dW was written"
    assert dbuf is None or bool(torch.isnan(dbuf[inp["knv"]:]).all()), name + ": the guard behind db was written"
    report("wgrad", name, dt, kc.wgrad_instance(c, dt), worst, t0, tiles=kc.wgrad_tiles(c), nsplit=c["nsplit"])
