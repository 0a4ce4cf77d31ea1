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
