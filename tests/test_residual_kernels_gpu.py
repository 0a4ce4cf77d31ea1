"""chap_residual_fwd / chap_residual_bwd / chap_grad_sum (csrc/residual.hip), per element against fp64 restatements with the error model
of tests/kernel_ref.py (its `unit` / `gamma` / `bound`, its constants).  Stored inputs are rounded to the storage type first; the lazy
transforms are restated by kernel_ref.lazy_f32 (rounded where the kernel rounds).  Chain lengths: at most 4 fp32 adds per element
(r + (src0 + src1); ((g0 + g1) + g2) and the multiplier; ((g0 + g1) + g2) + g3), C for dxin's channel sum.

Shapes: N = 2, D x H x W = 3 x 5 x 7 (odd: ragged last wave and block), C in {16, 32, 128} (2, 4, 16 lanes per voxel; one to 14 blocks).
One further case, `two_trips`, is large enough (528 000 voxels x 16 channels = 1 056 000 lanes > 2048 blocks x 256) that every block
takes a second grid-stride trip and the last trip is ragged -- with dxin on, the loop in which all lanes of a wave stay in step."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from tests import kernel_ref as kr
from tests.test_kernels_gpu import cl, rq, uncl

DEV = "cuda"
SP = (3, 5, 7)
N = 2
DTYPES = [torch.float32, torch.bfloat16]


def _wide(x, dtype, coff, extra):
    """x (NCDHW, rounded) as channels [coff, coff + C) of a wider channel-last tensor filled with other finite values."""
    n, c = x.shape[:2]
    w = torch.full((n, c + extra) + tuple(x.shape[2:]), 3.0)
    w[:, coff:coff + c] = x
    return cl(w, dtype)


def _fwd_case(dtype, C, nsrc, xin, sp=SP, seed=0):
    g = torch.Generator().manual_seed(1000 + C + 10 * nsrc + seed)
    sh = (N, C) + tuple(sp)
    r = rq(torch.randn(sh, generator=g), dtype)
    rs, rb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    vr, dvr = kr.lazy_f32(r, rs, rb)
    rl = ops.Lazy(cl(r, dtype), rs.to(DEV), rb.to(DEV), False)
    parts, srcs, xin_t = [], [], None
    if xin:
        xi = torch.randn((N, 1) + tuple(sp), generator=g)
        parts.append((xi.double().expand(sh), torch.zeros(sh, dtype=torch.float64)))
        xin_t = xi.reshape(N, -1).to(DEV)
    else:
        a = rq(torch.randn(sh, generator=g), dtype)
        sa, sb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        cm = (torch.rand(N, C, generator=g) >= 0.5).float() * 2.0
        parts.append(kr.lazy_f32(a, sa, sb, act=True, slope=0.0, chan_mul=cm))
        srcs.append(ops.Lazy(cl(a, dtype), sa.to(DEV), sb.to(DEV), True, 0.0, chan_mul=cm.to(DEV)))
        if nsrc == 2:
            b = rq(torch.randn(sh, generator=g), dtype)
            parts.append(kr.lazy_f32(b))
            srcs.append(ops.Lazy(_wide(b, dtype, 8, 16), C=C, coff=8))
    pre = vr + sum(p[0] for p in parts)
    sabs = vr.abs() + sum(p[0].abs() for p in parts)
    flip = dvr + sum(p[1] for p in parts)
    ref = pre.clamp_min(0)                                   # ReLU is 1-Lipschitz: the bound of the sum holds behind it
    bnd = kr.bound(ref, sabs=sabs, chain=1 + len(parts), flip=flip, store=dtype)
    assert bool((pre > 0).any()) and bool((pre < 0).any())   # both signs of the output's argument are present
    out = torch.empty((N,) + tuple(sp) + (C,), device=DEV, dtype=dtype)
    return rl, srcs, xin_t, out, ref, bnd


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [16, 32, 128])
@pytest.mark.parametrize("nsrc", [1, 2])
def test_residual_fwd_sources(dtype, C, nsrc):
    rl, srcs, _, out, ref, bnd = _fwd_case(dtype, C, nsrc, False)
    ops.residual_fwd(rl, srcs, out)
    kr.check("residual_fwd C=%d nsrc=%d" % (C, nsrc), uncl(out), ref, bnd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_fwd_image(dtype):
    rl, _, xin, out, ref, bnd = _fwd_case(dtype, 16, 0, True)
    ops.residual_fwd(rl, [], out, xin=xin)
    kr.check("residual_fwd xin", uncl(out), ref, bnd)


def _bwd_case(dtype, C, ng, with_cm, sp=SP):
    g = torch.Generator().manual_seed(2000 + C + 10 * ng + int(with_cm))
    sh = (N, C) + tuple(sp)
    gs = [rq(torch.randn(sh, generator=g), dtype) for _ in range(ng)]
    grads = [(_wide(t, dtype, 8, 8), 8) if k == ng - 1 else (cl(t, dtype), 0) for k, t in enumerate(gs)]      # the last one: g_coff = 8 in rows of C + 8
    o = rq(torch.randn(sh, generator=g).clamp_min(0), dtype)                                                  # a ReLU output: about half exact zeros
    cm = (torch.rand(N, C, generator=g) >= 0.5).float() * 2.0 if with_cm else None
    fac = kr._bcast(cm, o, per_sample=True) if with_cm else 1.0
    on = (o > 0).double()
    ref = sum(t.double() for t in gs) * fac * on
    sabs = sum(t.double().abs() for t in gs) * fac * on
    return grads, o, cm, ref, sabs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [16, 32, 128])
@pytest.mark.parametrize("ng", [1, 2, 3])
@pytest.mark.parametrize("with_cm", [False, True])
def test_residual_bwd(dtype, C, ng, with_cm):
    grads, o, cm, ref, sabs = _bwd_case(dtype, C, ng, with_cm)
    gout = torch.empty((N,) + SP + (C,), device=DEV, dtype=dtype)
    ops.residual_bwd(grads, cl(o, dtype), gout, chan_mul=cm.to(DEV) if with_cm else None)
    got = uncl(gout)
    kr.check("residual_bwd C=%d ng=%d" % (C, ng), got, ref, kr.bound(ref, sabs=sabs, chain=ng + 1, store=dtype))
    assert bool((o == 0).any()) and bool((got[o == 0] == 0).all())          # strictly-greater test: exact zeros where out == 0


def _check_dxin(name, dtype, grads, o, cm, ref, sabs, ng, sp):
    C = o.shape[1]
    gout = torch.empty((N,) + tuple(sp) + (C,), device=DEV, dtype=dtype)
    dxin = torch.full((N, sp[0] * sp[1] * sp[2]), float("nan"), device=DEV)
    ops.residual_bwd(grads, cl(o, dtype), gout, chan_mul=None if cm is None else cm.to(DEV), dxin=dxin)
    kr.check(name + " gout", uncl(gout), ref, kr.bound(ref, sabs=sabs, chain=ng + 1, store=dtype))
    # dxin: the channel sum of the UNROUNDED values (each within its bound without the store term), a C-term fp32 chain
    e = kr.bound(ref, sabs=sabs, chain=ng + 1)
    dref = ref.sum(1)
    dbnd = kr.bound(dref, sabs=ref.abs().sum(1), chain=C, extra=e.sum(1), store=torch.float32)
    kr.check(name + " dxin", dxin.cpu().reshape((N,) + tuple(sp)), dref, dbnd, dims="ndhw")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ng", [1, 3])
def test_residual_bwd_dxin(dtype, ng):
    grads, o, cm, ref, sabs = _bwd_case(dtype, 16, ng, ng == 3)
    _check_dxin("residual_bwd dxin ng=%d" % ng, dtype, grads, o, cm, ref, sabs, ng, SP)


def test_residual_bwd_dxin_wide_voxel():
    """C = 128: 16 lanes per voxel, the longest butterfly a 3D net's first block could ask for here."""
    grads, o, cm, ref, sabs = _bwd_case(torch.float32, 128, 2, False)
    _check_dxin("residual_bwd dxin C=128", torch.float32, grads, o, cm, ref, sabs, 2, SP)


def test_two_grid_stride_trips():
    sp = (33, 64, 125)
    dtype = torch.bfloat16
    rl, _, xin, out, ref, bnd = _fwd_case(dtype, 16, 0, True, sp=sp)
    ops.residual_fwd(rl, [], out, xin=xin)
    kr.check("residual_fwd two trips", uncl(out), ref, bnd)
    grads, o, cm, ref, sabs = _bwd_case(dtype, 16, 2, False, sp=sp)
    _check_dxin("residual_bwd two trips", dtype, grads, o, cm, ref, sabs, 2, sp)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ng", [2, 4])
def test_grad_sum(dtype, ng):
    C = 32
    g = torch.Generator().manual_seed(3000 + ng)
    sh = (N, C) + SP
    gs = [rq(torch.randn(sh, generator=g), dtype) for _ in range(ng)]
    grads = [(_wide(t, dtype, 8, 8), 8) if k == 1 else (cl(t, dtype), 0) for k, t in enumerate(gs)]
    out = torch.empty((N,) + SP + (C,), device=DEV, dtype=dtype)
    ops.grad_sum(grads, out)
    ref = sum(t.double() for t in gs)
    kr.check("grad_sum ng=%d" % ng, uncl(out), ref, kr.bound(ref, sabs=sum(t.double().abs() for t in gs), chain=ng, store=dtype))


def test_two_lanes_of_a_group_equal_the_single_launches():
    """Two lanes (the two decoders' blocks) inside one group region: forward, backward and grad_sum of each lane are recorded and issued as
    merged grids; bit for bit the results of the one-by-one launches."""
    dtype, C = torch.bfloat16, 32
    lanes = []
    for seed in (0, 1):
        rl, srcs, _, out, _, _ = _fwd_case(dtype, C, 2, False, seed=seed)
        grads, o, cm, _, _ = _bwd_case(dtype, C, 3, True)
        lanes.append(dict(rl=rl, srcs=srcs, grads=grads, o=cl(o + seed, dtype), cm=cm.to(DEV)))

    def run(ln):
        out, gout, gsum = (torch.empty((N,) + SP + (C,), device=DEV, dtype=dtype) for _ in range(3))
        ops.residual_fwd(ln["rl"], ln["srcs"], out)
        ops.residual_bwd(ln["grads"], ln["o"], gout, chan_mul=ln["cm"])
        ops.grad_sum(ln["grads"], gsum)
        return out, gout, gsum

    single = [run(ln) for ln in lanes]
    before = L.group.launched
    with L.group(torch.cuda.current_stream().cuda_stream) as region:
        grouped = [run(lanes[0])]
        region.next_lane()
        grouped.append(run(lanes[1]))
    assert L.group.launched - before == 3                   # three merged grids instead of six launches
    torch.cuda.synchronize()
    for a, b in zip(single, grouped):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert not torch.equal(single[0][0], single[1][0])
