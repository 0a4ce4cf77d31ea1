"""tests/kernel_ref.py on the CPU: the fp64 restatements equal torch's fp64 ops, an emulated CORRECT kernel (the same operands, an
fp32 sum in another order, a bf16 / fp32 store) passes `check`, and each emulated fault fails it.  For each fault the per-kernel GPU
tests' max-normalised check (relerr < tolerance) is evaluated as well, and its verdict is asserted: the record of what those checks
accept."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import kernel_ref as kr

TOL = {torch.float32: 2e-5, torch.bfloat16: 2.5e-2}       # tests/test_kernels_gpu.py: conv outputs (statistics: 1e-3 + TOL)
WTOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}        # tests/test_kernels_bwd_gpu.py: dW / db
ATOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2}        # tests/test_kernels_bwd_gpu.py: act_bwd outputs, dgamma / dbeta


def relerr(a, b):          # tests/test_kernels_gpu.py:relerr
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def gen(s):
    return torch.Generator().manual_seed(s)


def rq(x, dtype):
    return x.to(dtype).float()


def close(a, b):
    return (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())


def fails(name, got, ref, bnd):
    with pytest.raises(AssertionError, match=name):
        kr.check(name, got, ref, bnd)
    return True


# ---- restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [2, 3])
def test_restatements_equal_torch_fp64(dims):
    g = gen(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    conv, convT = (F.conv2d, F.conv_transpose2d) if dims == 2 else (F.conv3d, F.conv_transpose3d)
    sp = (7, 10) if dims == 2 else (5, 6, 7)              # ragged
    ev = (6, 10) if dims == 2 else (4, 6, 8)              # even (k2 s2)
    half = [s // 2 for s in ev]
    N, ci, co = 2, 8, 12
    x, xe = r(N, ci, *sp), r(N, ci, *ev)
    w3, w1, w2 = r(co, ci, *[3] * dims), r(co, ci, *[1] * dims), r(co, ci, *[2] * dims)
    wd = r(ci, co, *[2] * dims)                            # transposed conv weight [cin, cout, 2..]
    assert close(kr.conv_linear(kr.PACK_CONV_FWD, x, w3), conv(x, w3, padding=1))
    assert close(kr.conv_linear(kr.PACK_CONV_FWD, x, w1), conv(x, w1))
    assert close(kr.conv_linear(kr.PACK_CONV_FWD, xe, w2), conv(xe, w2, stride=2))
    gy = r(N, co, *sp)
    assert close(kr.conv_linear(kr.PACK_CONV_DGRAD, gy, w3), convT(gy, w3, padding=1))
    xh = r(N, ci, *half)
    assert close(kr.conv_linear(kr.PACK_DECONV_FWD, xh, wd), convT(xh, wd, stride=2))
    gf = r(N, co, *ev)
    assert close(kr.conv_linear(kr.PACK_DECONV_DGRAD, gf, wd), conv(gf, wd, stride=2))
    gh = r(N, co, *half)
    assert close(kr.conv_linear(kr.PACK_DOWN_DGRAD, gh, w2), convT(gh, w2, stride=2))
    # weight gradients (dW[co, ci, taps] <- [taps, kc = ci, kn = co]) and bias gradients
    red = [0] + list(range(2, dims + 2))
    for A, w, kw in ((x, w3, dict(padding=1)), (x, w1, {}), (xe, w2, dict(stride=2))):
        B = r(*conv(A, w, **kw).shape)
        wv = torch.zeros_like(w, requires_grad=True)
        conv(A, wv, **kw).backward(B)
        k = w.shape[-1]
        res = kr.wgrad_ref(A, B, ksize=k, stride=2 if k == 2 else 1)
        assert close(kr.to_layout(res["dw"], (1, k ** dims, ci * k ** dims), w.shape), wv.grad)
        assert close(res["db"], B.sum(red))
    # transposed conv: A = the fine gradient (kc = co), B = the coarse input (kn = ci) -> dW[ci, co, taps]
    wt = torch.zeros_like(wd, requires_grad=True)
    gf2 = r(N, co, *ev)
    convT(xh, wt, stride=2).backward(gf2)
    res = kr.wgrad_ref(gf2, xh, ksize=2, stride=2)
    assert close(kr.to_layout(res["dw"], (1, 2 ** dims, co * 2 ** dims), wd.shape), wt.grad)


def test_act_bwd_restatement_equals_autograd():
    """training-mode BatchNorm + LeakyReLU + keep mask + 2x2 max-pool consumer (2D), and the fixed affine + Dropout3d multipliers (3D)."""
    g = gen(2)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N, C, H, W = 2, 8, 6, 10
    raw = r(N, C, H, W) * 1.5 + 0.3
    gam, bet = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, r(C) * 0.2
    keep = (torch.rand(N, C, H, W, generator=g) > 0.2).double()
    g1, g2, gp = r(N, C, H, W), r(N, C, H, W), r(N, C, H // 2, W // 2)
    rr, gm, bt = raw.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    a = F.leaky_relu(F.batch_norm(rr, None, None, gm, bt, True, 0.1, 1e-5), 0.125) * keep * 1.25      # slope, keep scale exact in fp32
    p, idx = F.max_pool2d(a, 2, return_indices=True)
    ((a * (g1 + g2)).sum() + (p * gp).sum()).backward()
    pos = (((idx // W) & 1) << 1) | ((idx % W) & 1)
    mean = raw.mean((0, 2, 3))
    invstd = (raw.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    scale = gam * invstd
    shift = bet - mean * scale
    ref = kr.act_bwd_ref(raw, [g1, g2], scale=scale, shift=shift, act=True, slope=0.125, keep=keep, keep_scale=1.25, g_pool=gp,
                         pool_idx=pos, bn_mode=1, mean=mean, invstd=invstd, gamma_=gam, count=N * H * W)
    assert close(ref["g"], rr.grad) and close(ref["S1"], gm.grad) and close(ref["S0"], bt.grad)
    # 3D, fixed affine (bn 2): d/d raw of sum(g * cm * leaky(raw*scale + shift))
    raw3, g3 = r(2, 16, 3, 4, 6), r(2, 16, 3, 4, 6)
    sc3, sh3, cm = torch.rand(16, generator=g, dtype=torch.float64) + 0.5, r(16) * 0.2, (torch.rand(2, 16, generator=g) > 0.3).double() * 1.5
    rr = raw3.clone().requires_grad_(True)
    (F.leaky_relu(rr * sc3.view(1, -1, 1, 1, 1) + sh3.view(1, -1, 1, 1, 1), 0.125) * cm.view(2, 16, 1, 1, 1) * g3).sum().backward()
    ref = kr.act_bwd_ref(raw3, [g3], scale=sc3, shift=sh3, act=True, slope=0.125, chan_mul=cm, bn_mode=2)
    assert close(ref["g"], rr.grad)


# ---- emulated correct kernels ---------------------------------------------------------------------------------------------------
def _conv_case(dtype, dims, seed, N=2, ci=32, co=16, sp=None, lazy=True):
    g = gen(seed)
    sp = sp or ((13, 21) if dims == 2 else (5, 7, 9))
    x = rq(torch.randn(N, ci, *sp, generator=g), dtype)
    kw = {}
    if lazy:
        kw = dict(scale=torch.rand(ci, generator=g) + 0.5, shift=torch.randn(ci, generator=g) * 0.2, act=True, slope=0.01)
        if dims == 2:
            kw.update(keep=(torch.rand(N, ci, *sp, generator=g) > 0.3).float(), keep_scale=1.25)
        else:
            kw.update(chan_mul=(torch.rand(N, ci, generator=g) > 0.3).float() * 1.5)
    a, flip = kr.operand(x, dtype, **kw)
    w = torch.randn(co, ci, *[3] * dims, generator=g) / (ci * 3 ** dims) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    wq = kr.weight_operand(w, dtype)
    r = kr.conv_ref(kr.PACK_CONV_FWD, a, wq, b, flip=flip)
    conv = F.conv2d if dims == 2 else F.conv3d
    acc = conv(a.float(), wq.float(), None, padding=1) + b.view([1, -1] + [1] * dims)      # torch's fp32 conv: another summation order
    return dict(g=g, a=a, flip=flip, wq=wq, b=b, r=r, acc=acc, w=w, dims=dims, ci=ci, co=co)


def _chunked_fp32(a, wq, b, dims):
    """fp32 sum in yet another order: taps last to first, 8 channels at a time."""
    ap, wf = F.pad(a.float(), [1] * (2 * dims)), wq.float()
    osp = a.shape[2:]
    y = torch.zeros(a.shape[0], wq.shape[0], *osp)
    for t in reversed(list(itertools.product(range(3), repeat=dims))):
        win = (slice(None), slice(None)) + tuple(slice(t[i], t[i] + osp[i]) for i in range(dims))
        for c in range(0, a.shape[1], 8):
            y += torch.einsum("nc...,oc->no...", ap[win][:, c:c + 8], wf[(slice(None), slice(c, c + 8)) + t])
    return y + b.view([1, -1] + [1] * dims)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dims", [2, 3])
def test_emulated_correct_kernels_pass(dtype, dims):
    cs = _conv_case(dtype, dims, 3)
    r, acc = cs["r"], cs["acc"]
    red = [0] + list(range(2, dims + 2))
    for v in (acc, _chunked_fp32(cs["a"], cs["wq"], cs["b"], dims)):
        kr.check("conv out", v.to(dtype), r["y"], kr.conv_bound(r, dtype))
        kr.check("conv acc", v, r["y"], kr.conv_bound(r, None))
    c0 = torch.randn(cs["co"], generator=cs["g"])
    (s1, b1), (s2, b2) = kr.stats_ref(r, c0)
    d = acc - c0.view([1, -1] + [1] * dims)
    kr.check("stats S", d.sum(red), s1, b1)
    kr.check("stats Q", (d * d).sum(red), s2, b2)
    # weight gradient (fp32 autograd of the same operands), accumulated into an existing dW
    gy = rq(torch.randn(r["y"].shape, generator=cs["g"]), dtype)
    rw = kr.wgrad_ref(cs["a"], gy.double(), ksize=3, stride=1, flipA=cs["flip"])
    wgt = torch.nn.grad.conv2d_weight if dims == 2 else torch.nn.grad.conv3d_weight
    got = 0.5 + wgt(cs["a"].float(), cs["w"].shape, gy, padding=1)
    taps, ci, co = 3 ** dims, cs["ci"], cs["co"]
    st = (1, taps, ci * taps)
    prior = torch.full((taps, ci, co), 0.5, dtype=torch.float64)
    kr.check("dW", got, kr.to_layout(rw["dw"] + prior, st, cs["w"].shape), kr.to_layout(kr.wgrad_bound(rw, prior), st, cs["w"].shape))
    kr.check("db", gy.sum(red), rw["db"], kr.wgrad_bound(rw, which="db"))


def _act_case(dtype, seed, C=8, shape=(2, 16, 24)):
    g = gen(seed)
    N, H, W = shape
    raw = rq(torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3, dtype)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    mean = raw.double().mean((0, 2, 3)).float()
    invstd = (raw.double().var((0, 2, 3), unbiased=False) + 1e-5).rsqrt().float()
    scale = gam * invstd
    shift = bet - mean * scale
    keep = (torch.rand(N, C, H, W, generator=g) > 0.2).float()
    g1, g2 = rq(torch.randn(N, C, H, W, generator=g), dtype), rq(torch.randn(N, C, H, W, generator=g), dtype)
    ref = kr.act_bwd_ref(raw, [g1, g2], scale=scale, shift=shift, act=True, slope=0.01, keep=keep, keep_scale=1.25, bn_mode=1,
                         mean=mean, invstd=invstd, gamma_=gam, count=N * H * W)
    # the kernel's arithmetic in fp32 (sums in torch's order); the activation's sign from the exact z, as the kernel's fmaf gives it
    z = raw.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    sl = torch.tensor(0.01, dtype=torch.float32)
    dz = (g1 + g2) * torch.where(z > 0, torch.ones(()), sl) * torch.where(keep != 0, 1.25, 0.0)
    istd, mu = invstd.view(1, -1, 1, 1), mean.view(1, -1, 1, 1)
    xh = raw * istd + (-mu * istd)
    S0, S1 = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    return dict(ref=ref, dz=dz, xh=xh, S0=S0, S1=S1, raw=raw, gam=gam, istd=istd, mu=mu, cnt=N * H * W)


def _act_apply(c, S0, S1):
    k0 = c["gam"].view(1, -1, 1, 1) * c["istd"]
    k1, k2 = (S0 / c["cnt"]).view(1, -1, 1, 1), (S1 / c["cnt"]).view(1, -1, 1, 1)
    cB, cC = -c["istd"] * k0 * k2, c["mu"] * c["istd"] * k0 * k2 - k0 * k1
    return c["dz"] * k0 + (c["raw"] * cB + cC)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_emulated_correct_act_bwd_passes(dtype):
    c = _act_case(dtype, 4)
    ref = c["ref"]
    kr.check("gout", _act_apply(c, c["S0"], c["S1"]).to(dtype), ref["g"], kr.bound(ref["g"], extra=ref["g_bound"], store=dtype))
    prior = torch.full((8,), 0.25)
    kr.check("dgamma", prior + c["S1"], ref["S1"] + 0.25, kr.param_grad_bound(ref["S1"], ref["b1"], prior))
    kr.check("dbeta", prior + c["S0"], ref["S0"] + 0.25, kr.param_grad_bound(ref["S0"], ref["b0"], prior))


# ---- mutations: each emulated fault fails the check; relerr's verdict on it is recorded ----------------------------------------
def test_mutation_a_largest_term_missing_at_one_interior_pixel():
    dtype = torch.bfloat16
    cs = _conv_case(dtype, 2, 5, ci=256, sp=(12, 20))
    a, wq, acc, r = cs["a"], cs["wq"], cs["acc"].clone(), cs["r"]
    n, o, y, x = 1, 3, 9, 13
    terms = a[n, :, y - 1:y + 2, x - 1:x + 2] * wq[o]                   # [ci, 3, 3]
    acc[n, o, y, x] -= terms.reshape(-1)[terms.abs().reshape(-1).argmax()].float()
    got = acc.to(dtype)
    assert fails("mut a", got, r["y"], kr.conv_bound(r, dtype))
    assert relerr(got.float(), r["y"]) >= TOL[dtype]                    # (the existing check rejects this one: one term is 4 % of max |y|)


def test_mutation_b_one_channel_of_one_tap_missing_along_a_border_column():
    dtype = torch.bfloat16
    cs = _conv_case(dtype, 2, 6, ci=32, sp=(20, 37))
    a, wq, acc, r = cs["a"], cs["wq"], cs["acc"].clone(), cs["r"]
    W = a.shape[-1]
    # output column W - 1, tap (dy = 1, dx = 0) reads column W - 2: drop channel 5 of that tap there
    acc[:, :, :, W - 1] -= torch.einsum("nh,o->noh", a[:, 5, :, W - 2], wq[:, 5, 1, 0]).float()
    got = acc.to(dtype)
    assert fails("mut b", got, r["y"], kr.conv_bound(r, dtype))
    assert relerr(got.float(), r["y"]) >= TOL[dtype]                    # (rejected at this size)


def test_mutation_c_ragged_tail_pixel_written_with_its_neighbour():
    dtype = torch.bfloat16
    cs = _conv_case(dtype, 2, 7, ci=16, sp=(18, 37))
    got = cs["acc"].to(dtype)
    got[0, :, -1, -1] = got[0, :, -1, -2]
    assert fails("mut c", got, cs["r"]["y"], kr.conv_bound(cs["r"], dtype))
    assert relerr(got.float(), cs["r"]["y"]) >= TOL[dtype]              # (the existing check rejects this one)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mutation_d_statistics_missing_one_4x16_tile(dtype):
    cs = _conv_case(dtype, 2, 8, N=4, ci=16, co=16, sp=(256, 256), lazy=False)
    r, acc = cs["r"], cs["acc"]
    c0 = torch.randn(16, generator=cs["g"])
    (s1, b1), (s2, b2) = kr.stats_ref(r, c0)
    d = (acc - c0.view(1, -1, 1, 1)).double()
    q = (d * d).sum((0, 2, 3)) - (d[2, :, 100:104, 32:48] ** 2).sum((1, 2))
    assert fails("mut d", q, s2, b2)
    assert relerr(q, s2) < 1e-3 + TOL[dtype]


def test_mutation_e_dw_missing_the_ragged_last_row_of_one_image():
    dtype = torch.bfloat16
    cs = _conv_case(dtype, 2, 9, N=3, ci=16, co=16, sp=(37, 50))
    gy = rq(torch.randn(cs["r"]["y"].shape, generator=cs["g"]), dtype)
    rw = kr.wgrad_ref(cs["a"], gy.double(), ksize=3, stride=1, flipA=cs["flip"])
    gm = gy.clone()
    gm[2, :, 36, :] = 0
    got = torch.nn.grad.conv2d_weight(cs["a"].float(), cs["w"].shape, gm, padding=1)
    st = (1, 9, 16 * 9)
    ref = kr.to_layout(rw["dw"], st, cs["w"].shape)
    assert fails("mut e", got, ref, kr.to_layout(kr.wgrad_bound(rw), st, cs["w"].shape))
    assert relerr(got, ref) >= WTOL[dtype]                              # (the existing check rejects this one at this size)


def test_mutation_f_act_bwd_dgamma_from_4_of_every_64_pixels():
    """the C = 8 reduction fault: lanes l, l+16, l+32, l+48 summed, lanes 1..15 of each row left out."""
    dtype = torch.bfloat16
    c = _act_case(dtype, 10)
    ref = c["ref"]
    p = (c["dz"] * c["xh"]).permute(0, 2, 3, 1).reshape(-1, 8)          # pixel-major, as the kernel walks them
    S1 = p[0::16].sum(0)
    assert fails("mut f", S1, ref["S1"], kr.param_grad_bound(ref["S1"], ref["b1"]))
    assert relerr(S1, ref["S1"]) >= ATOL[dtype]                         # (rejected -- but no existing test runs C = 8)


def test_mutation_g_dw_and_db_missing_one_blocks_partial_row():
    dtype = torch.bfloat16
    cs = _conv_case(dtype, 2, 11, N=4, ci=16, co=16, sp=(64, 64))
    gy = rq(torch.randn(cs["r"]["y"].shape, generator=cs["g"]), dtype)
    rw = kr.wgrad_ref(cs["a"], gy.double(), ksize=3, stride=1, flipA=cs["flip"])
    gm = gy.permute(0, 2, 3, 1).reshape(-1, 16).clone()                # 256 blocks of 64 consecutive pixels; block 100 lost
    gm[100 * 64:101 * 64] = 0
    gm = gm.reshape(4, 64, 64, 16).permute(0, 3, 1, 2)
    got = torch.nn.grad.conv2d_weight(cs["a"].float(), cs["w"].shape, gm, padding=1)
    st = (1, 9, 16 * 9)
    ref = kr.to_layout(rw["dw"], st, cs["w"].shape)
    assert fails("mut g dW", got, ref, kr.to_layout(kr.wgrad_bound(rw), st, cs["w"].shape))
    db = gm.sum((0, 2, 3))
    assert fails("mut g db", db, rw["db"], kr.wgrad_bound(rw, which="db"))
    assert relerr(got, ref) >= WTOL[dtype] and relerr(db, rw["db"]) >= WTOL[dtype]     # (rejected at this size)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_gradient_of_a_lazy_b_is_the_sum_of_its_fp32_values(dtype):
    """wgrad_ref(Bv=, dBv=): the kernel sums db of a lazy B before the value is packed to the operand type.  An fp32 sum of the fp32 values passes under
    wgrad_bound(which="db"); in bf16 the sum of the rounded operands does not (and without Bv the reference is that sum, as it was); a plain B has
    Bv = B and dBv = 0, which changes nothing."""
    g = torch.Generator().manual_seed(17)
    x = rq(torch.randn(2, 32, 9, 21, generator=g), dtype)
    A = rq(torch.randn(2, 16, 18, 42, generator=g), dtype).double()
    sc_, sh_ = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.2
    v, dv = kr.lazy_f32(x, scale=sc_, shift=sh_, act=True, slope=0.01)
    B, fB = kr.mfma_operand(v, dv, dtype)
    rw = kr.wgrad_ref(A, B, ksize=2, stride=2, flipB=fB, Bv=v, dBv=dv)
    old = kr.wgrad_ref(A, B, ksize=2, stride=2, flipB=fB)
    assert torch.equal(rw["dw"], old["dw"]) and torch.equal(old["db"], B.sum((0, 2, 3))) and torch.equal(rw["db"], v.sum((0, 2, 3)))
    assert kr.check("db of fp32 values", v.float().sum((0, 2, 3)), rw["db"], kr.wgrad_bound(rw, which="db")) <= 1.0
    if dtype == torch.bfloat16:
        assert fails("db of operands", B.float().sum((0, 2, 3)), rw["db"], kr.wgrad_bound(rw, which="db"))
    plain = kr.wgrad_ref(A, x.double(), ksize=2, stride=2, Bv=x.double(), dBv=torch.zeros_like(x).double())
    ref = kr.wgrad_ref(A, x.double(), ksize=2, stride=2)
    assert torch.equal(plain["db"], ref["db"]) and torch.equal(kr.wgrad_bound(plain, which="db"), kr.wgrad_bound(ref, which="db"))


# ==== plumbing kernels (losses, VAT / BCP helpers, RNG, diff mask, largest component, SGD) ==========================================
import numpy as np

from oracle import train_step as ots

LTOL, GTOL = 1e-5, 1e-4                                   # tests/test_kernels_bwd_gpu.py::test_losses_vs_oracle: loss values, gradients
STOL = 1e-6                                                # ::test_lcc_diffmask_vat_helpers_sgd: SGD parameters and momenta


def test_loss_restatements_equal_fp64_autograd():
    for name, kw in (("2d_ragged", dict(w=(0.5, 1.0))), ("3d_c2", dict(w=(1.0, 0.5))), ("3d_c2_offset", dict(w=(0.75, 0.25), plain=True))):
        c = kr.loss_inputs(name)
        lo = c["l1"].double().requires_grad_(True)
        plain = kw.get("plain", False)
        m = torch.ones_like(c["mask"]) if plain else c["mask"]
        tb = c["ta"] if plain else c["tb"]
        wa, wb = kw["w"]
        li, lp, tot = ots.mix_loss(lo, c["ta"], tb, m.double(), l_weight=wa, u_weight=wb)
        (tot * 0.25).backward()                            # weights and scale exact in fp32, as the kernel receives them
        r = kr.mix_loss_ref(c["l1"], c["ta"], None if plain else tb, None if plain else m, wa, wb, gscale=0.25)
        assert close(r["loss"], torch.stack([li, lp, tot]).detach()) and close(r["dlogits"], lo.grad)
        # k_dice / k_ce: loss_k = w_k (kd Dice_k + kc CE_k)
        lo = c["l1"].double().requires_grad_(True)
        soft = F.softmax(lo, 1)
        parts = []
        for t, mk, w in ((c["ta"], m.double(), wa), (tb, 1.0 - m.double(), wb)):
            ce = (F.cross_entropy(lo, t, reduction="none") * mk).sum() / (mk.sum() + 1e-16)
            parts.append(w * (0.3 * ots.dice_loss_bcp(soft, t, mk, c["C"]) + 1.7 * ce))
        (parts[0] + parts[1]).backward()
        r = kr.mix_loss_ref(c["l1"], c["ta"], tb, m, wa, wb, k_dice=0.3, k_ce=1.7)
        assert abs(float(r["loss"][2] - (parts[0] + parts[1]).detach())) < 1e-6 * float(r["loss"][2])      # 0.3f, 1.7f: the fp32 scalars the kernel gets
        assert (r["dlogits"] - lo.grad).abs().max() < 1e-6 * lo.grad.abs().max()
        # pseudo block
        pr = kr.pseudo_ref(c["l1"], c["l2"])
        s1, s2, a1, a2, kn = ots.pseudo_block(c["l1"].double(), c["l2"].double())
        assert close(pr["soft1"], s1) and close(pr["soft2"], s2) and close(pr["knowledge"], kn)
        assert torch.equal(pr["arg1"], a1) and torch.equal(pr["arg2"], a2)
        # the two distances, accumulated onto a prior loss value
        for mode, fn in (("kl", ots.kl_two_heads), ("dice", ots.dice_two_heads)):
            la, lb = c["l1"].double().requires_grad_(True), c["l2"].double().requires_grad_(True)
            d = fn((la, lb), (c["t1"].double(), c["t2"].double()))
            (d * 0.75).backward()
            r = kr.kl_ref((c["l1"], c["l2"]), (c["t1"], c["t2"]), mode, gscale=0.75, prior=0.25)
            assert abs(float(r["loss"]) - 0.25 - float(d.detach())) < 1e-12
            # the kernel's KL gradient gs/total (p - t) is the derivative for targets that sum to 1 over the classes: these do to fp32 rounding
            tol = 1e-12 if mode == "dice" else 4 * kr.U32
            assert (r["g"][0] - la.grad).abs().max() <= tol * la.grad.abs().max() and (r["g"][1] - lb.grad).abs().max() <= tol * lb.grad.abs().max()


@pytest.mark.parametrize("name", list(kr.LOSS_SHAPES))
def test_near_tie_share_of_the_pseudo_block_inputs(name):
    """the GPU test leaves pixels out of the argmax comparison only where fp64 cannot decide it: none on these inputs (cap 0.01 %), while
    the planted exact ties (gap 0) stay in."""
    c = kr.loss_inputs(name)
    r = kr.pseudo_ref(c["l1"], c["l2"])
    assert float(r["near"].double().mean()) <= kr.NEAR_TIE_CAP and int(r["near"].sum()) == 0
    top = r["soft1"].topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) >= 40       # exact ties are present and are compared


def test_helper_restatements_equal_the_oracle():
    g = gen(20)
    x = torch.randn(3, 1, 9, 13, generator=g).double()
    assert close(kr.l2_normalize_ref(x)[0], ots.l2_normalize(x))
    d, m = torch.randn(3, 1, 9, 13, generator=g).double(), (torch.rand(3, 1, 9, 13, generator=g) > 0.5).double()
    assert close(kr.perturb_ref(x, d, 6.0, m)[0], x + 6.0 * m * d) and close(kr.perturb_ref(x, d, 0.5, None, True)[0], x + 0.5 * torch.sign(d))
    p, gr, mo = (torch.randn(1003, generator=g).double() for _ in range(3))
    params, moms = [p.clone()], [mo.clone()]
    ots.sgd_step(params, [gr], moms, 0.5, 0.75, 0.125)       # scalars exact in fp32
    p2, _, m2, _ = kr.sgd_ref(p, gr, mo, 0.5, 0.75, 0.125)
    assert close(p2, params[0]) and close(m2, moms[0])
    a, b = torch.randn(6, 4, 3, 3, generator=g).double(), torch.randn(6, 4, 3, 3, generator=g).double()
    sim = F.cosine_similarity(a.reshape(6, -1), b.reshape(6, -1), dim=1, eps=0)
    assert close(kr.grad_sim_ref(a, b, torch.zeros(6), 0.0)[0], sim)
    assert close(kr.grad_sim_ref(a, b, torch.ones(6), 0.5)[0], 0.5 + 0.5 * sim)
    # boxes: generate_mask's zero box
    mask, lm = ots.box_masks(2, 37, 50, 5, 9)
    box = (5, 9, int(37 * 2 / 3), int(50 * 2 / 3))
    assert torch.equal(kr.box_mask_ref(2, (37, 50), box), lm.long())
    u, v = torch.rand(2, 1, 37, 50, generator=g), torch.rand(2, 1, 37, 50, generator=g)
    assert torch.equal(kr.box_mix_ref(u, v, box), u * mask + v * (1 - mask))
    mask3, lm3 = ots.box_masks_3d(2, 5, 9, 13, 1, 2, 3)
    assert torch.equal(kr.box_mask_ref(2, (5, 9, 13), (1, 2, 3, 3, 6, 8)), lm3.long())
    # diff mask: the exact construction makes fp32 and fp64 pooling agree, so the oracle's fp32 mask is the reference's
    for shape, topk in (((3, 40, 40), 0.29), ((2, 60, 96), 0.35), ((2, 6, 20, 24), 0.1)):
        H, W = (shape[1], shape[2]) if len(shape) == 3 else (shape[1] * shape[2], shape[3])
        kn = kr.exact_knowledge(shape[0], H, W, 4, g).reshape(shape)
        pooled = F.avg_pool2d(kn.reshape(shape[0], 1, H, W), 4)
        assert torch.equal(pooled.double(), F.avg_pool2d(kn.double().reshape(shape[0], 1, H, W), 4))
        assert all(len(set(row.tolist())) == row.numel() for row in pooled.reshape(shape[0], -1))         # distinct
        p1 = torch.randint(0, 4, shape, generator=g)
        p2 = torch.where(torch.rand(shape, generator=g) < 0.02, (p1 + 1) % 4, p1)
        k = kr.diff_mask_k(topk, pooled[0].numel())
        assert torch.equal(kr.diff_mask_ref(p1, p2, kn, 4, k), ots.create_mask_v1(p1, p2, kn, 4, topk))
    assert [kr.diff_mask_k(t, m) for t, m in ((0.29, 100), (0.35, 360), (0.7, 360), (1e-6, 100), (1.0, 100))] == [28, 125, 251, 1, 100]
    assert [int(np.float32(t) * np.float32(m)) for t, m in ((0.29, 100), (0.35, 360), (0.7, 360))] == [29, 126, 252]       # the float product


def test_u01_is_the_splitmix64_finalizer():
    """u01(seed, i) = the top 24 bits of splitmix64's (i + 1)-th output from state `seed`: the published first outputs for seed 0."""
    assert [int(v) for v in kr.u01_np(0, np.arange(2))] == [0xE220A8397B1DCDAF >> 40, 0x6E789E6AA1B965F4 >> 40]
    for seed, sd in ((77, None), (77, 0), (77, 5), ((1 << 64) - 3, 1 << 62), (123, -1)):
        a = kr.u01_np(seed, np.arange(70000), sd)
        assert np.array_equal(a, kr.u01_int(seed, 70000, sd).numpy()) and 0 <= a.min() and a.max() < 1 << 24
    assert np.array_equal(kr.u01_np(77, np.arange(100), None), kr.u01_np(77, np.arange(100), 0))
    assert not np.array_equal(kr.u01_np(77, np.arange(100), 0), kr.u01_np(77, np.arange(100), 5))
    keep = kr.keep_mask_ref(5, 1 << 16, 0.3)
    assert abs(float(keep.float().mean()) - 0.7) < 1e-2 and bool((kr.keep_mask_ref(5, 100, 0.0) == 1).all()) and bool((kr.keep_mask_ref(5, 100, 1.0) == 0).all())
    cm = kr.chan_mask_ref(5, 1000, 0.3)
    assert set(cm.tolist()) == {0.0, float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.3)))}
    v, b = kr.rand_uniform_ref(123, 1000, -0.5, 0.5)
    assert float(v.min()) >= -0.5 and float(v.max()) < 0.5 and float(b.max()) <= 2.0 ** -23


# ---- an emulated CORRECT loss kernel: fp32 arithmetic, one partial row per 256 pixels, another summation order -------------------
def _emulate_mix(c, w=(0.5, 1.0), drop_tail=False, drop_row=None, msum_both=False, smear_last=False):
    lg, C = c["l1"], c["C"]
    N, P = lg.shape[0], lg[0, 0].numel()
    z = lg.reshape(N, C, P)
    p = torch.softmax(z, 1)                                # fp32
    lse = torch.logsumexp(z, 1)
    mk = [c["mask"].reshape(N, P).float(), 1.0 - c["mask"].reshape(N, P).float()]
    ts = [F.one_hot(t.reshape(N, P), C).permute(0, 2, 1).float() for t in (c["ta"], c["tb"])]
    rows = []
    for k in range(2):
        cols = [(lse - (ts[k] * z).sum(1)) * mk[k]] + [p[:, i] * ts[k][:, i] * mk[k] for i in range(C)] + [p[:, i] * p[:, i] * mk[k] for i in range(C)] \
            + [ts[k][:, i] * mk[k] for i in range(C)] + [mk[k]]
        rows.append(torch.stack([v.reshape(-1) for v in cols], 1))          # [N * P, NA], pixel-major as the kernel walks them
    per_px = torch.cat(rows, 1)
    total = N * P
    if drop_tail:
        per_px = per_px[:total - total % 256]
    pad = (-per_px.shape[0]) % 256
    blocks = F.pad(per_px, (0, 0, 0, pad)).reshape(-1, 256, per_px.shape[1]).flip(1).sum(1)      # a block's row, summed back to front
    if drop_row is not None:
        blocks[drop_row] = 0
    acc = blocks.double().sum(0).float().reshape(2, -1)
    if msum_both:
        acc[:, -1] = acc[:, -1].sum()
    s, kd, kc = torch.tensor(1e-10), 0.5, 0.5
    part, dz, dp = [], torch.zeros_like(p), torch.zeros_like(p)
    for k in range(2):
        a = acc[k]
        I, Z, Y = a[1:1 + C], a[1 + C:1 + 2 * C], a[1 + 2 * C:1 + 3 * C]
        den = Z + Y + s
        dice = (1.0 - (2.0 * I + s) / den).sum() / C * w[k]
        ce = w[k] * a[0] / (a[-1] + 1e-16)
        part.append(kd * dice + kc * ce)
        kce = w[k] * mk[k] / (a[-1] + 1e-16)
        dz = dz + kce.unsqueeze(1) * (p - ts[k])
        dp = dp + (w[k] / C) * mk[k].unsqueeze(1) * (-2.0 * ts[k] / den.view(1, C, 1) + ((2.0 * I + s) * 2.0 / (den * den)).view(1, C, 1) * p)
    dl = kc * dz + kd * p * (dp - (dp * p).sum(1, keepdim=True))
    if smear_last:
        dl[:, :, -1] = dl[:, :, -2]
    return acc, torch.stack([part[0], part[1], part[0] + part[1]]), dl.reshape(lg.shape)


@pytest.fixture(scope="module")
def two_trips():
    c = kr.loss_inputs("2d_two_trips")
    return c, kr.mix_loss_ref(c["l1"], c["ta"], c["tb"], c["mask"], 0.5, 1.0)


def test_emulated_correct_loss_kernels_pass(two_trips):
    c, r = two_trips
    acc, loss, dl = _emulate_mix(c)
    kr.check("acc", acc, r["acc"], r["acc_b"], "ka")
    kr.check("loss", loss, r["loss"], r["loss_b"], "k")
    kr.check("dlogits", dl, r["dlogits"], r["dlogits_b"])
    for name in ("2d_ragged", "3d_c2"):                    # and the small shapes; softmax / knowledge / the distances in plain fp32
        c = kr.loss_inputs(name)
        r = kr.mix_loss_ref(c["l1"], c["ta"], c["tb"], c["mask"], 0.5, 1.0)
        acc, loss, dl = _emulate_mix(c)
        kr.check("acc", acc, r["acc"], r["acc_b"], "ka"), kr.check("loss", loss, r["loss"], r["loss_b"], "k"), kr.check("dlogits", dl, r["dlogits"], r["dlogits_b"])
        pr = kr.pseudo_ref(c["l1"], c["l2"])
        s1, s2, a1, a2, kn = ots.pseudo_block(c["l1"], c["l2"])
        kr.check("soft1", s1, pr["soft1"], pr["soft1_b"]), kr.check("knowledge", kn, pr["knowledge"], pr["knowledge_b"], "ndhw")
        assert torch.equal(a1, pr["arg1"]) and torch.equal(a2, pr["arg2"])
        for mode, fn in (("kl", ots.kl_two_heads), ("dice", ots.dice_two_heads)):
            la, lb = c["l1"].clone().requires_grad_(True), c["l2"].clone().requires_grad_(True)
            d = fn((la, lb), (c["t1"], c["t2"]))
            (d * 0.7).backward()
            kr_ = kr.kl_ref((c["l1"], c["l2"]), (c["t1"], c["t2"]), mode, gscale=0.7, prior=0.25)
            kr.check("dist loss", (d.detach() + 0.25).reshape(1), kr_["loss"], kr_["loss_b"], "k")
            kr.check("dist g0", la.grad, kr_["g"][0], kr_["g_b"][0]), kr.check("dist g1", lb.grad, kr_["g"][1], kr_["g_b"][1])


def test_emulated_correct_helpers_pass():
    g = gen(21)
    x = torch.randn(3, 6149, generator=g)
    x[1] = 0
    ref, b = kr.l2_normalize_ref(x)
    kr.check("l2", x / (x.reshape(3, -1, 11).pow(2).sum(2).sum(1).sqrt().view(3, 1) + 1e-8), ref, b, "np")
    n = 1003
    p, gr, g2, mo = (torch.randn(n, generator=g) for _ in range(4))
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    gg = (gr + g2) * f(1 / 3) + f(1e-4) * p
    m2 = f(0.9) * mo + gg
    p2, e_p, mr, e_m = kr.sgd_ref(p, gr, mo, 0.013, 0.9, 1e-4, 1 / 3, g2)
    kr.check("sgd p", p - f(0.013) * m2, p2, e_p, "i"), kr.check("sgd m", m2, mr, e_m, "i")
    d = torch.randn(n, generator=g)
    ref, b = kr.perturb_ref(p, d, 6.0, (mo > 0).float())
    kr.check("perturb", p + f(6.0) * (mo > 0).float() * d, ref, b, "i")
    a, bb, s0 = torch.randn(6, 144, generator=g), torch.randn(6, 144, generator=g), torch.randn(6, generator=g)
    ref, b = kr.grad_sim_ref(a, bb, s0, 0.9)
    kr.check("grad_sim", f(0.9) * s0 + (1 - f(0.9)) * F.cosine_similarity(a.double(), bb.double(), dim=1).float(), ref, b, "c")


# ---- mutations of the plumbing kernels; the old whole-tensor verdict (relerr < tolerance) is recorded next to each ----------------
def test_mutation_h_loss_accumulators_missing_the_last_partial_block(two_trips):
    c, r = two_trips                                       # 132 297 pixels: the last 201 lost
    acc, loss, dl = _emulate_mix(c, drop_tail=True)
    assert fails("mut h acc", acc, r["acc"], r["acc_b"]) and fails("mut h loss", loss, r["loss"], r["loss_b"])
    assert relerr(loss, r["loss"]) >= LTOL                 # (201 of 132 297 pixels: 1.5e-3 of every sum -- the old check rejects it too at this size)


def test_mutation_i_loss_accumulators_missing_one_blocks_row(two_trips):
    c, r = two_trips
    acc, loss, dl = _emulate_mix(c, drop_row=300)
    assert fails("mut i acc", acc, r["acc"], r["acc_b"]) and fails("mut i loss", loss, r["loss"], r["loss_b"])
    assert fails("mut i dlogits", dl, r["dlogits"], r["dlogits_b"])
    assert relerr(loss, r["loss"]) >= LTOL and relerr(dl, r["dlogits"]) >= GTOL     # (rejected at this size: one row of 517 is 2e-3 of every total)


def test_mutation_j_dlogits_last_pixel_of_each_sample_gets_its_neighbours_value(two_trips):
    c, r = two_trips
    acc, loss, dl = _emulate_mix(c, smear_last=True)
    assert fails("mut j", dl, r["dlogits"], r["dlogits_b"])
    assert relerr(dl, r["dlogits"]) >= GTOL                # (rejected: a gradient element is of the size of the largest one)


def test_mutation_k_msum_taken_over_both_parts(two_trips):
    c, r = two_trips
    acc, loss, dl = _emulate_mix(c, msum_both=True)
    assert fails("mut k acc", acc, r["acc"], r["acc_b"]) and fails("mut k loss", loss, r["loss"], r["loss_b"]) and fails("mut k dl", dl, r["dlogits"], r["dlogits_b"])
    assert relerr(loss, r["loss"]) >= LTOL


def test_mutations_l_m_diff_mask_count_off_by_one_and_ties_dropped():
    g = gen(22)
    kn = kr.exact_knowledge(3, 40, 40, 4, g)
    p1 = torch.randint(0, 4, (3, 40, 40), generator=g)
    ref = kr.diff_mask_ref(p1, p1, kn, 4, kr.diff_mask_k(0.29, 100))
    off = kr.diff_mask_ref(p1, p1, kn, 4, int(np.float32(0.29) * np.float32(100)))           # the float product's count: 29
    assert int((ref != off).sum()) == 3 * 16               # one 4x4 cell per sample
    assert relerr(off, ref) == 1.0                         # (a mask: any wrong pixel is a whole-tensor error of 1; the old test only ran topk = 0.1)
    # ties at the threshold: the k-th value occurs 4 times; a select that keeps exactly k cells drops three of them
    kn = kr.exact_knowledge(3, 40, 40, 4, g, ties=(28, 3))
    ref = kr.diff_mask_ref(p1, p1, kn, 4, 28)
    pooled = F.avg_pool2d(kn.unsqueeze(1), 4).reshape(3, -1)
    idx = pooled.topk(28, dim=1).indices
    dropped = torch.zeros(3, 100).scatter_(1, idx, 1.0).reshape(3, 10, 10).repeat_interleave(4, 1).repeat_interleave(4, 2)
    assert int(ref.sum()) == 3 * 31 * 16 and int((ref != dropped).sum()) == 3 * 3 * 16


def test_mutation_n_one_union_missing_cuts_the_spiral():
    whole, cut = kr.spiral(67, 131), kr.spiral(67, 131, cut=0.4)
    ref = ots.largest_cc(whole.unsqueeze(0), 2)
    assert torch.equal(ref[0], whole)                      # one component: all of it is kept
    got = ots.largest_cc(cut.unsqueeze(0), 2)              # what a labelling that misses the union at the cut keeps: the larger arm only
    lost = int((got != ref).sum())
    assert lost > 1000 and not torch.equal(got, ref)
    # the smooth blobs of the old test hold no component that hangs on a single union


def test_mutation_o_keep_bytes_of_the_last_partial_group_shifted():
    n = 65539                                              # 4096 full groups and 3 bytes
    ref = kr.keep_mask_ref(77, n, 0.3)
    got = ref.clone()
    got[n - 3:] = kr.keep_mask_ref(77, n + 1, 0.3)[n - 2:]  # byte i of the tail drawn from index i + 1
    assert not torch.equal(got, ref)
    assert abs(float(got.float().mean()) - 0.7) < 1e-2     # ACCEPTED by the old check (the mean of the mask)


def test_mutation_p_sgd_tail_not_updated():
    g = gen(23)
    n = 1003
    p, gr, mo = (torch.randn(n, generator=g) for _ in range(3))
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    m2 = f(0.9) * mo + (gr + f(1e-4) * p)
    got = p - f(0.01) * m2
    got[n - n % 4:] = p[n - n % 4:]
    p2, e_p, _, _ = kr.sgd_ref(p, gr, mo, 0.01, 0.9, 1e-4)
    assert fails("mut p", got, p2, e_p)
    assert relerr(got, p2) >= STOL                         # (rejected at lr = 0.01: the step is 1e-2 of a parameter)


# ==== evaluation, channel-drop, BatchNorm-finalize and layout kernels ================================================================
from oracle import filter_dropout as ofd
from oracle import inference as oinf


def test_inference_restatements_equal_torch_and_the_oracle_loop():
    a, b = kr.ensemble_inputs(4, (1.0, 3.0))
    ad, bd = a.double(), b.double()
    want = {"model1": torch.softmax(ad, 1), "model2": torch.softmax(bd, 1), "logit_ensemble": torch.softmax((a + b).double() / 2.0, 1),
            "prob_ensemble": (torch.softmax(ad, 1) + torch.softmax(bd, 1)) / 2.0}
    for mode, p in want.items():
        r = kr.ensemble_ref(a, b, mode)
        assert close(r["p"], p) and torch.equal(r["label"], p.argmax(1)) and int(r["label"][0, 0, 0]) == 0
    r = kr.ensemble_ref(a[:, :1], None, "model1")           # C = 1: p = 1, label 0
    assert bool((r["p"] == 1).all()) and not bool(r["label"].any()) and not bool(r["near"].any())
    # sliding window: oracle.inference.test_single_case walks the origins x, y, z in {0, 8} x {0, 8} x {0, 6} and calls `net` once per patch
    C, vol, patch = 3, (20, 18, 14), (12, 10, 8)
    g = gen(30)
    origins = [(x, y, z) for x in (0, 8) for y in (0, 8) for z in (0, 6)]
    logits = torch.randn(len(origins), C, *patch, generator=g, dtype=torch.float64) * 3
    it = iter(range(len(origins)))
    label, score = oinf.test_single_case(lambda patch_: logits[next(it)][None], np.zeros(vol, np.float32), 8, 6, patch, num_classes=C)
    acc = kr.window_accumulate_ref(logits, origins, torch.zeros(C, *vol), torch.zeros(vol))
    fin = kr.window_finalize_ref(acc["score"], acc["cnt"], acc["score_b"])
    assert bool(acc["covered"].all()) and not bool(fin["empty"].any())
    assert np.abs(fin["score"].numpy() - score).max() < 1e-6 and float(acc["cnt"].max()) == 8.0      # (the oracle's score map is fp32)
    assert np.array_equal(fin["label"].numpy()[~fin["near"].numpy()], label[~fin["near"].numpy()])
    # an uncovered voxel keeps what it held (bound 0), and 0 / 0 is named
    lg, s0, c0 = kr.window_inputs(2, **kr.WINDOW_CASE)
    acc = kr.window_accumulate_ref(lg[0], kr.WINDOW_CASE["calls"][0], s0, c0)
    unc = ~acc["covered"]
    assert bool(unc.any()) and torch.equal(acc["score"][:, unc], s0.double()[:, unc]) and float(acc["score_b"][:, unc].max()) == 0.0
    assert bool(kr.window_finalize_ref(acc["score"], acc["cnt"])["empty"][0, -1, -1])


def _bn_case(C=6, nsub=1, nslots=65, N=4, P=130, seed=31, shift=True, count_one=False):
    """a conv output [N, Clog, P] dealt to `nslots` slots of consecutive pixels; the slot buffer as the convs write it (header, [slot][S | Q][Clog], NaN in the slots
    not in use) and the same values as a plain tensor [N * P * nsub, C] for F.batch_norm."""
    g = gen(seed)
    Clog = C * nsub
    x = torch.randn(N * P, Clog, generator=g) * 1.5 + torch.randn(Clog, generator=g)
    if count_one:
        x = x[:1]
    sh = (torch.randn(C, generator=g) * 0.5) if shift else None
    d = x.double() - (sh.double().repeat(nsub) if shift else 0.0)
    owner = torch.arange(x.shape[0]) % nslots
    slots = torch.full((max(nslots + 3, 8), 2, Clog), float("nan"))
    for b in range(nslots):
        slots[b, 0] = d[owner == b].sum(0).float()
        slots[b, 1] = (d[owner == b] ** 2).sum(0).float()
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    flat = x.reshape(-1, nsub, C).reshape(-1, C)
    return dict(slots=slots, nslots=nslots, C=C, Clog=Clog, count=flat.shape[0], shift=sh, gam=gam, bet=bet, rm=rm, rv=rv, flat=flat)


def _bn_ref(c, momentum=0.125, eps=1e-5):
    return kr.bn_finalize_ref(c["slots"], c["nslots"], c["C"], c["Clog"], c["count"], c["shift"], c["gam"], c["bet"], c["rm"], c["rv"], momentum, eps)


def _bn_emulate(c, momentum=0.125, eps=1e-5, drop_slot=None, clamp_unmasked=False, biased=False):
    """the kernel's order: fp64 totals over the slots, then fp32."""
    sl, n = c["slots"][:c["nslots"]].double(), c["nslots"]
    if drop_slot is not None:
        sl = torch.cat((sl[:drop_slot], sl[drop_slot + 1:]))
    tot = sl.sum(0)
    if clamp_unmasked:
        tot = tot + (1024 - n) * c["slots"][0].double()
    S, Q = (t.reshape(-1, c["C"]).sum(0) for t in (tot[0], tot[1]))
    cnt = float(c["count"])
    ms = S / cnt
    var = (Q / cnt - ms * ms).clamp_min(0)
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    mean = ((c["shift"].double() if c["shift"] is not None else 0.0) + ms).float()
    invstd = (1.0 / torch.sqrt(var + float(f(eps)))).float()
    sc = c["gam"] * invstd
    out = dict(mean=mean, invstd=invstd, scale=sc, shift=c["bet"] - mean * sc)
    unb = (var * cnt / (cnt - 1.0) if (cnt > 1 and not biased) else var).float()
    out["running_mean"] = (1 - f(momentum)) * c["rm"] + f(momentum) * mean
    out["running_var"] = (1 - f(momentum)) * c["rv"] + f(momentum) * unb
    return out


def _bn_check(name, got, ref, keys=None):
    for k in keys or ref:
        kr.check("%s %s" % (name, k), got[k], ref[k][0], ref[k][1], "c")


@pytest.mark.parametrize("nsub,nslots,shift", [(1, 1, False), (4, 65, True), (8, 63, True)])
def test_bn_restatement_equals_batch_norm_fp64(nsub, nslots, shift):
    c = _bn_case(nsub=nsub, nslots=nslots, shift=shift)
    r = _bn_ref(c)
    x = c["flat"].double()
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    y = F.batch_norm(x, rm, rv, c["gam"].double(), c["bet"].double(), True, 0.125, 1e-5)
    # the slot values are fp32 roundings of fp64 partial sums: the totals agree to a few 2^-24 of sum |x|, not to 1e-12
    tol = lambda v: 1e-5 * max(1.0, float(v.abs().max()))
    assert (r["mean"][0] - x.mean(0)).abs().max() < tol(x) and (r["running_mean"][0] - rm).abs().max() < tol(rm)
    assert (r["running_var"][0] - rv).abs().max() < tol(rv)
    assert (x * r["scale"][0] + r["shift"][0] - y).abs().max() < 1e-4 * float(y.abs().max())
    assert (r["invstd"][0] - (x.var(0, unbiased=False) + 1e-5).rsqrt()).abs().max() < 1e-5
    assert "running_mean" not in _bn_ref(c, momentum=0.0)
    # count = 1: the unbiased variance is the biased one (0), not 0 / 0
    c1 = _bn_case(count_one=True, nslots=1)
    r1 = _bn_ref(c1)
    assert bool(torch.isfinite(r1["running_var"][0]).all()) and float((r1["running_var"][0] - 0.875 * c1["rv"].double()).abs().max()) < 1e-5


def test_emulated_correct_bn_finalize_passes_and_faults_c_d_e_fail():
    for kw in (dict(nsub=1, nslots=65), dict(nsub=4, nslots=63), dict(nsub=8, nslots=1), dict(count_one=True, nslots=1)):
        c = _bn_case(**kw)
        _bn_check("bn", _bn_emulate(c), _bn_ref(c))
    c = _bn_case(nslots=65)
    ref = _bn_ref(c)
    got = _bn_emulate(c, drop_slot=64)                      # (c) a lane's second slot (lane 0: slots 0, 64, ...) is lost
    assert fails("bn mean", got["mean"], *ref["mean"]) and fails("bn scale", got["scale"], *ref["scale"])
    c = _bn_case(nslots=63)
    ref = _bn_ref(c)
    got = _bn_emulate(c, clamp_unmasked=True)               # (d) b < nslots ? b : 0 without the mask: row 0 added for every slot index >= nslots
    assert fails("bn mean", got["mean"], *ref["mean"]) and fails("bn invstd", got["invstd"], *ref["invstd"])
    got = _bn_emulate(c, biased=True)                       # (e) count instead of count - 1
    assert fails("bn running_var", got["running_var"], *ref["running_var"])
    _bn_check("bn", got, ref, ("mean", "invstd", "scale", "shift", "running_mean"))


def test_bn_eval_restatement_and_emulation():
    g = gen(32)
    C = 65
    gam, bet, rm = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g)
    rv[0], rv[1] = 0.0, 1e6
    (sc, e_sc), (sh, e_sh) = kr.bn_eval_ref(gam, bet, rm, rv, 1e-5)
    x = torch.randn(7, C, generator=g, dtype=torch.float64)
    y = F.batch_norm(x, rm.double(), rv.double(), gam.double(), bet.double(), False, 0.0, kr._fp32_scalar(1e-5))      # eps as the fp32 scalar the kernel gets
    assert (x * sc + sh - y).abs().max() < 1e-12 * float(y.abs().max())
    s32 = gam * torch.rsqrt(rv + 1e-5)
    kr.check("bn_eval scale", s32, sc, e_sc, "c"), kr.check("bn_eval shift", bet - rm * s32, sh, e_sh, "c")
    kr.check("bn_eval shift fused", (bet.double() - rm.double() * s32.double()).float(), sh, e_sh, "c")
    assert fails("bn_eval", gam * torch.rsqrt(rv), sc, e_sc)                  # eps forgotten


def _lazy_case(dtype, N=3, C=16, sp=(5, 7), seed=33, lazy=True):
    g = gen(seed)
    x = rq(torch.randn(N, C, *sp, generator=g), dtype)
    kw = {}
    if lazy:
        kw = dict(scale=torch.rand(C, generator=g) + 0.5, shift=torch.randn(C, generator=g) * 0.2, act=True, slope=0.01,
                  keep=(torch.rand(N, C, *sp, generator=g) > 0.3).float(), keep_scale=1.25, chan_mul=(torch.rand(N, C, generator=g) > 0.3).float() * 1.5)
    return x, kw


def _lazy_emulate(x, kw):
    """src_load8 in fp32 (the affine unfused: within lazy_f32's dv)."""
    v = x.clone()
    bc = lambda t: t.view([1, -1] + [1] * (x.dim() - 2))
    if kw:
        v = v * bc(kw["scale"]) + bc(kw["shift"])
        v = torch.where(v > 0, v, v * torch.tensor(kw["slope"], dtype=torch.float32))
        v = torch.where(kw["keep"] != 0, v * kw["keep_scale"], torch.zeros(()))
        v = v * kw["chan_mul"].view(list(kw["chan_mul"].shape) + [1] * (x.dim() - 2))
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_channel_sums_restatement_emulation_and_fault_f(dtype):
    x, kw = _lazy_case(dtype, N=3, C=16, sp=(37, 23))
    lz = kr.lazy_f32(x, **kw)
    prior = torch.randn(16, generator=gen(34))
    ref, b = kr.channel_sum_ref(lz, prior)
    v = _lazy_emulate(x, kw)
    rows = v.permute(0, 2, 3, 1).reshape(-1, 16)             # pixel-major, 128 pixels per block as C = 16 deals them
    pad = (-rows.shape[0]) % 128
    blocks = F.pad(rows, (0, 0, 0, pad)).reshape(-1, 128, 16).flip(1).sum(1)
    kr.check("channel_sum", prior + blocks.double().sum(0).float(), ref, b, "c")
    assert fails("channel_sum", prior + blocks[:-1].double().sum(0).float(), ref, b)      # (f) the last, partial block is lost
    plain = kr.lazy_f32(x)
    assert close(kr.channel_sum_ref(plain)[0], x.double().sum((0, 2, 3)))
    r = kr.sample_channel_sum_ref(lz)
    part = torch.stack([v[:, :, i::7].sum((2, 3)) for i in range(7)], 1)      # rows i, i + 7, ...: one way of dealing the pixels to 7 chunks
    kr.check("sample sum", part.double().sum(1), r["sum"], r["sum_b"], "nc")
    kr.check("sample mean", part.double().sum(1) / (37 * 23), r["mean"], r["mean_b"], "nc")
    assert close(kr.sample_channel_sum_ref(plain)["mean"], x.double().mean((2, 3)))


def _drop_emulate(c, B, comp, branch, kind, flip=None):
    """channel_drop_kernel's score-driven mode in fp32, in its order."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    U, C = c["u1"].shape
    a = c["part"][:, 0].clone()
    for k in range(1, c["part"].shape[1]):
        a = a + c["part"][:, k]
    s = c["gs"].view(1, C) * (a * f(1.0 / c["npix"]))
    mean = s.sum(1, keepdim=True) / C
    sigma = torch.sqrt(((s - mean) ** 2).sum(1, keepdim=True) / (C - 1))
    if kind == "gauss":
        pr = (0.5 * (1 + torch.erf((s - mean) / (sigma * 2.0 + f(1e-8)) * f(0.70710678118654752)))).clamp(0, 1)
    else:
        pr = 1.0 / (1.0 + torch.exp(2.0 * ((s - mean) / (sigma + f(1e-8)))))
    pk = 1.0 - pr
    m1 = (c["u1"] < (pr if comp and branch == 1 else pk)).float()
    m2 = (c["u2"] < (pr if comp and branch == 0 else pk)).float()
    if flip is not None:
        m1[flip] = 1.0 - m1[flip]
    ones = torch.ones(B, C)
    return pr, torch.cat((ones, m1 * (U * C) / m1.sum())), torch.cat((ones, m2 * (U * C) / m2.sum()))


@pytest.mark.parametrize("kind", ["sigmoid", "gauss"])
def test_channel_drop_restatement_emulation_and_fault_g(kind):
    for (U, C), (comp, branch) in zip(kr.DROP_SHAPES[1:4], ((False, 0), (True, 0), (True, 1))):
        c = kr.channel_drop_inputs(U, C, prob_kind=kind, comp=comp, branch=branch)
        B = 2 * U
        r = kr.channel_drop_ref(c["u1"], c["u2"], B, "scores", pool_partial=c["part"], npix=c["npix"], grad_sim=c["gs"], comp=comp, branch=branch, prob_kind=kind)
        # the oracle in fp64 (its activation: the pooled mean; its 1e-8 and 1 / npix are doubles: agreement to 1e-7, not 1e-12)
        act = c["part"].double().sum(1) / c["npix"]
        want = ofd.drop_probs(c["gs"].double(), act, kind)
        assert (r["probs"] - want).abs().max() < 1e-6
        m1, m2 = ofd.drop_based_on_prob(want, comp, c["u1"].double(), c["u2"].double(), branch)
        assert (r["mul1"][B:] - m1[..., 0, 0]).abs().max() < 1e-6 * U * C and (r["mul2"][B:] - m2[..., 0, 0]).abs().max() < 1e-6 * U * C      # (the oracle's masks are fp32)
        assert not bool(r["near1"].any()) and not bool(r["near2"].any())      # the GPU test's near-tie share on these seeds: 0
        pr, e1, e2 = _drop_emulate(c, B, comp, branch, kind)
        kr.check("probs", pr, r["probs"], r["probs_b"], "uc"), kr.check("mul1", e1, r["mul1"], r["mul1_b"], "nc"), kr.check("mul2", e2, r["mul2"], r["mul2_b"], "nc")
        # (g) one flipped comparison moves every kept element of that mask by 1 / count: each of them fails on its own
        _, bad, _ = _drop_emulate(c, B, comp, branch, kind, flip=(U - 1, C - 1))
        wrong = (bad.double() - r["mul1"]).abs() > r["mul1_b"]
        assert int(wrong.sum()) == int(((r["mul1"][B:] != 0) | (bad[B:] != 0)).sum()) and not bool(wrong[:B].any())
    # modes 0 / 1 and the all-zero fallback
    c = kr.channel_drop_inputs(3, 16)
    r0 = kr.channel_drop_ref(c["u1"], c["u2"], 3, "dropout2d")
    rz = kr.channel_drop_ref(c["u1"], c["u2"], 3, "scores", pool_partial=c["part"], npix=c["npix"], grad_sim=torch.zeros(16))
    assert rz["mode"] == "dropout2d" and torch.equal(r0["mul1"], rz["mul1"]) and torch.equal(r0["mul2"], rz["mul2"])
    assert torch.equal(r0["mul1"][3:], (c["u1"] < 0.5).double() * 2) and bool((r0["mul1"][:3] == 1).all())
    r1 = kr.channel_drop_ref(c["u1"], c["u2"], 3, "comp_binomial")
    assert torch.equal(r1["mul1"][3:] + r1["mul2"][3:], torch.full((3, 16), 2.0, dtype=torch.float64))
    # an empty mask is named, as 0 / 0 is NaN in the definition
    re = kr.channel_drop_ref(torch.ones(3, 16), c["u2"], 3, "scores", pool_partial=c["part"], npix=c["npix"], grad_sim=c["gs"])
    assert re["nan1"] and not re["nan2"]
    with np.errstate(invalid="ignore"):
        assert bool(torch.isnan(ofd.drop_based_on_prob(re["probs"], False, torch.ones(3, 16).double(), c["u2"].double())[0]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fold_restatement_equals_autograd_emulation_and_fault_h(dtype):
    g = gen(35)
    B, U, C, ld, coff = 4, 2, 16, 32, 8
    gfull = rq(torch.randn(B + U, 3, 5, ld, generator=g), dtype)
    mul = torch.cat((torch.ones(B, C), (torch.rand(U, C, generator=g) > 0.4).float() * 1.7))
    ref, b = kr.fold_ref(gfull, coff, C, mul, B, U, dtype)
    f = torch.zeros(B, C, 3, 5, dtype=torch.float64, requires_grad=True)
    cot = gfull[..., coff:coff + C].permute(0, 3, 1, 2).double()
    (torch.cat((f, mul[B:].double().view(U, C, 1, 1) * f[B - U:])) * cot).sum().backward()
    assert close(ref, f.grad.permute(0, 2, 3, 1))
    gs = gfull[..., coff:coff + C]
    emu = gs[:B].clone()
    emu[B - U:] = (emu[B - U:].double() + gs[B:].double() * mul[B:].double().view(U, 1, 1, C)).float()      # the kernel's fmaf: one rounding
    kr.check("fold", emu.to(dtype), ref, b, "nhwc")
    assert float(b[:B - U].max()) == 0.0
    bad = gs[:B].clone()
    bad[B - U:] += gs[B:] * mul[B - 1:B + U - 1].view(U, 1, 1, C)           # (h) mul of sample u - 1
    assert fails("fold", bad.to(dtype), ref, b)
    ref0, b0 = kr.fold_ref(gfull, coff, C, None, B, 0, dtype)
    assert torch.equal(ref0, gs[:B].double()) and float(b0.max()) == 0.0


def test_layout_restatements_and_fault_i():
    g = gen(36)
    x = torch.randn(2, 3, 4, 5, generator=g)
    x[0, 0, 0, :4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -20])     # bf16 ties (to even: 1.0, 1.015625, -1.0) and just above one
    out0 = torch.full((2, 1, 4, 5, 32), float("nan"), dtype=torch.bfloat16)
    ref = kr.planar_to_cl_ref(x, out0, out_coff=8, cpad=8)
    assert ref[0, 0, 0, :4, 8].tolist() == [1.0, 1.015625, -1.0, 1.0078125]
    assert torch.equal(ref[..., 8:11].float(), x.permute(0, 2, 3, 1).unsqueeze(1).bfloat16().float()) and bool((ref[..., 11:16] == 0).all())
    assert bool(torch.isnan(ref[..., :8]).all()) and bool(torch.isnan(ref[..., 16:]).all())
    def emulate(width):
        """planar_to_cl8_kernel's walk: per (sample, pixel) `width` channels from out_coff on, the first C converted, the rest zero."""
        o = out0.clone().reshape(2, 20, 32)
        xf = x.reshape(2, 3, 20)
        for n in range(2):
            for pp in range(20):
                for c in range(width):
                    o[n, pp, 8 + c] = xf[n, c, pp].bfloat16() if c < 3 else 0.0
        return o.reshape(out0.shape)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(emulate(8)), bits(ref))
    bad = bits(emulate(9)) != bits(ref)                     # (i) the zero pad written one channel too far: every pixel's channel 16, nothing else
    assert int(bad.sum()) == 2 * 20 and bool(bad[..., 16].all())
    for C, ld, coff, cpad in ((1, 1, 0, 0), (3, 12, 4, 5)):  # no pad; a pad and a slice the vector path cannot take
        o0 = torch.full((2, 1, 4, 5, ld), float("nan"))
        r = kr.planar_to_cl_ref(x[:, :C], o0, coff, cpad)
        w = max(C, cpad)
        want = F.pad(x[:, :C].permute(0, 2, 3, 1).unsqueeze(1), (0, w - C))
        assert torch.equal(r[..., coff:coff + w], want) and int(torch.isnan(r).sum()) == 40 * (ld - w)
    v, dv = kr.lazy_f32(x)                                  # cl_to_planar of a plain source: the values themselves, exactly
    assert torch.equal(v, x.double()) and float(dv.max()) == 0.0


# ---- emulated inference kernels, faults (a) and (b), and the near-tie shares of the GPU inputs -------------------------------------
def _emulate_window(logits, origins, score0, cnt0, skip=None):
    s, c = score0.clone(), cnt0.clone()
    pw, ph, pd = logits.shape[2:]
    sm = torch.softmax(logits, 1)
    for k, (x, y, z) in enumerate(origins):
        s[:, x:x + pw, y:y + ph, z:z + pd] += sm[k]
        c[x:x + pw, y:y + ph, z:z + pd] += 1
    if skip is not None:
        k, (x, y, z) = skip
        ox, oy, oz = origins[k]
        s[:, x, y, z] -= sm[k][:, x - ox, y - oy, z - oz]
    return s, c


def test_emulated_inference_kernels_pass_and_faults_a_b_fail():
    for C in (1, 2, 4, 8):
        for mode in kr.ENSEMBLE_SCALES:
            a, b = kr.ensemble_inputs(C, (1.0, 8.0, 30.0))
            r = kr.ensemble_ref(a, b, mode)
            emu = {"model1": torch.softmax(a, 1), "model2": torch.softmax(b, 1), "logit_ensemble": torch.softmax((a + b) / 2.0, 1),
                   "prob_ensemble": (torch.softmax(a, 1) + torch.softmax(b, 1)) / 2.0}[mode]
            kr.check("ensemble " + mode, emu, r["p"], r["e_p"])
            ok = ~r["near"]
            assert torch.equal(emu.argmax(1)[ok], r["label"][ok])
    lg, s0, c0 = kr.window_inputs(8, **kr.WINDOW_CASE)
    calls = kr.WINDOW_CASE["calls"]
    acc = kr.window_accumulate_ref(lg[0], calls[0], s0, c0)
    s, c = _emulate_window(lg[0], calls[0], s0, c0)
    kr.check("window score", s, acc["score"], acc["score_b"], "cxyz")
    assert torch.equal(c.double(), acc["cnt"]) and torch.equal(s[:, ~acc["covered"]], s0[:, ~acc["covered"]])
    bad, _ = _emulate_window(lg[0], calls[0], s0, c0, skip=(2, (10, 8, 5)))     # (a) the last patch of the batch missing from one voxel
    assert fails("window score", bad, acc["score"], acc["score_b"])
    assert np.allclose(bad.numpy(), acc["score"].numpy(), atol=1.0) and not np.allclose(bad.numpy(), acc["score"].numpy(), atol=1e-6)
    fin = kr.window_finalize_ref(s, c)
    live = ~fin["empty"]
    q = torch.where(live, s / c, torch.zeros(()))
    kr.check("window fin", q, fin["score"], fin["score_b"], "cxyz")
    qb = torch.where(live, s / c.roll(1, 2), torch.zeros(()))                  # (b) the count of the neighbouring voxel
    assert fails("window fin", torch.where(torch.isfinite(qb), qb, torch.zeros(())), fin["score"], fin["score_b"])


def test_near_tie_shares_of_the_inference_inputs():
    """the conditions of tests/test_eval_plumbing_kernels_gpu.py, from the reference alone: the share of pixels left out of the label comparison."""
    for C in (2, 4, 8):
        for mode, scales in kr.ENSEMBLE_SCALES.items():
            r = kr.ensemble_ref(*kr.ensemble_inputs(C, scales), mode)
            assert float(r["near"].double().mean()) <= kr.NEAR_TIE_CAP and int(r["near"].sum()) == 0, (C, mode)
            top = r["p"].topk(2, dim=1).values
            assert bool(top[0, 0, 0, 0] == top[0, 1, 0, 0])                   # the exact tie stays in the comparison
    N, sp = kr.ENSEMBLE_TWO_TRIPS                           # the second-grid-stride-trip inputs, whose labels the GPU test compares as well
    for mode, scales in kr.ENSEMBLE_SCALES.items():
        r = kr.ensemble_ref(*kr.ensemble_inputs(2, scales, N=N, sp=sp), mode)
        assert float(r["near"].double().mean()) <= kr.NEAR_TIE_CAP, (mode, int(r["near"].sum()))
    # what scales (1, 8, 30) do to prob_ensemble: two saturated heads that disagree put two classes at 0.5 +- one ulp
    r = kr.ensemble_ref(*kr.ensemble_inputs(4, (1.0, 8.0, 30.0)), "prob_ensemble")
    assert float(r["near"].double().mean()) > 0.01
    for C in (2, 8):
        lg, s0, c0 = kr.window_inputs(C, **kr.WINDOW_CASE)
        s, c = s0.double(), c0.double()
        for l, o in zip(lg, kr.WINDOW_CASE["calls"]):
            acc = kr.window_accumulate_ref(l, o, s, c)
            s, c = acc["score"], acc["cnt"]
        fin = kr.window_finalize_ref(s, c)
        assert float(fin["near"].double().mean()) <= kr.NEAR_TIE_CAP and bool(fin["empty"].any()) and not bool(acc["covered"].all())
    for kind in ("sigmoid", "gauss"):
        for U, C in kr.DROP_SHAPES:
            c = kr.channel_drop_inputs(U, C, prob_kind=kind)
            r = kr.channel_drop_ref(c["u1"], c["u2"], U, "scores", pool_partial=c["part"], npix=c["npix"], grad_sim=c["gs"], prob_kind=kind)
            assert int(r["near1"].sum()) + int(r["near2"].sum()) == 0 and c["moved"] <= 1 + U * C // 1000
