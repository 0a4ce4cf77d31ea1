"""The conv families next to the 3x3 kernels on small ragged grids, one launch per case of tests/small_conv_cases.py: 1x1(x1), k2 s2 (2D, 3D),
1x1 + depth-to-space, the V-Net head kernel, the k1 / k2 s2 weight gradients -- every (KC, NT, MR) / (KC, bn) instance the bench-shaped steps launch
(tests/test_small_conv_cases_cpu.py proves which case reaches which), per element against the fp64 restatements of tests/kernel_ref.py under their own
bounds.  Lazy sources (BatchNorm affine + LeakyReLU, keep masks, per-sample multipliers, channel slices of NaN buffers), bias, shifted statistics, and
outputs in a channel slot of a wider NaN buffer with a NaN guard behind it, which must come back untouched.  Needs a GPU."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import ops
from tests import small_conv_cases as sc

DEV = "cuda"
DTS = ("f32", "bf16")


def cl(x, dtype):
    """NC(D)HW cpu -> [N, D, H, W, C] device tensor of dtype"""
    if x.dim() == 4:
        x = x.unsqueeze(2)
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def lazy_of(s, dtype):
    """a source of small_conv_cases.make_source on the device"""
    raw, C = cl(s["x"], dtype), s["x"].shape[1]
    kw = {}
    if s["kind"] == "sl":
        buf = torch.full(raw.shape[:-1] + (C + sc.SRC_EXTRA,), float("nan"), device=DEV, dtype=dtype)
        buf[..., sc.SRC_COFF:sc.SRC_COFF + C] = raw
        raw, kw = buf, dict(C=C, coff=sc.SRC_COFF)
    z = s["lazy"]
    if "keep" in z:
        kw.update(keep=cl(z["keep"], torch.uint8), keep_scale=z["keep_scale"])
    if "chan_mul" in z:
        kw.update(chan_mul=z["chan_mul"].to(DEV))
    if "scale" in z:
        return ops.Lazy(raw, z["scale"].to(DEV), z["shift"].to(DEV), True, z["slope"], **kw)
    return ops.Lazy(raw, **kw)


def g4(sp):
    return tuple(sp) if len(sp) == 3 else (1,) + tuple(sp)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [c["name"] for c in sc.ALL_FWD])
def test_forward_case(name, dt):
    t0 = time.perf_counter()
    c, dtype = sc.BY_NAME[name], sc.DTYPES[dt]
    inp = sc.fwd_inputs(c, dt)
    srcs = [lazy_of(s, dtype) for s in inp["srcs"]]
    cin, cout, taps = sc.pack_args(c)
    wp = ops.pack_weights(inp["w"].to(DEV), c["kind"], dtype, cin, cout, taps)
    flat, out = sc.new_out(c, dtype, DEV)
    Cl, M = sc.launch_cout(c), c["cout"]
    stats = ops.stats_buffer(Cl, DEV) if c["stats"] else None
    k = 2 if c["op"] == "k2" else 1
    kw = dict(out_planar=True, out_f32=True) if c["op"] == "head" else dict(out_ld=out.shape[-1], out_coff=sc.SLOT_COFF)
    if c["op"] == "d2s":
        kw.update(out_mode=1, out_cn=M)
    ops.conv_fwd(srcs, wp, None if inp["bias"] is None else inp["bias"].to(DEV), Cl, out, grid=(c["N"],) + g4(c["grid"]), in_dims=g4(sc.in_spatial(c)),
                 ksize=k, stride=k, dims=c["dims"], stats=stats, stats_shift=None if inp["shift"] is None else inp["shift"].to(DEV), **kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    totals = ops.stats_totals(stats, Cl, M).cpu() if c["stats"] else None
    r = sc.fwd_reference(c, dt, inp)
    worst = sc.fwd_check(c, dt, r, flat.cpu(), totals)
    print("small conv %-22s %-4s %s KC%d NT%d MR%d: worst err/bound %s  (gpu side %.2f s, all %.2f s)" % (
        name, dt, c["route"][dt], *c["plan"], " ".join("%.3f" % v for v in worst), t1 - t0, time.perf_counter() - t0))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [c["name"] for c in sc.WGRAD_CASES])
def test_weight_gradient_case(name, dt):
    t0 = time.perf_counter()
    c, dtype = sc.BY_NAME[name], sc.DTYPES[dt]
    inp = sc.wgrad_inputs(c, dt)
    A, B = lazy_of(inp["A"], dtype), lazy_of(inp["B"], dtype)
    n = inp["prior_dw"].numel()
    buf = torch.full((n + sc.GUARD,), float("nan"), device=DEV)                 # dW with a NaN guard behind it
    dw = buf[:n].view(inp["prior_dw"].shape)
    dw.copy_(inp["prior_dw"])
    db = inp["prior_db"].to(DEV) if c["db"] else None
    ks = c["ks"]
    ops.wgrad([A], B, dw, inp["strides"], grid=(c["N"],) + g4(c["grid"]), in_dims=g4(tuple(ks * s for s in c["grid"])), ksize=ks, stride=ks,
              dims=c["dims"], db=db, kn_valid=c["kn_valid"])
    torch.cuda.synchronize()
    rw = sc.wgrad_reference(c, dt, inp)
    worst = sc.wgrad_check(c, dt, rw, inp, dw.cpu(), None if db is None else db.cpu())
    assert bool(torch.isnan(buf[n:]).all()), name + ": the guard behind dW was written"
    print("small wgrad %-20s %-4s KC%d bn%d: worst err/bound %s  (%.2f s)" % (name, dt, *c["plan"][dt], " ".join("%.3f" % v for v in worst), time.perf_counter() - t0))
