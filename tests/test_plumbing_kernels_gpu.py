"""The kernels of csrc/loss.hip, csrc/aux.hip and csrc/ccl.hip per element against the fp64 restatements and bounds of
tests/kernel_ref.py (or exactly, where the result is an integer, a mask or a copy), at the smallest shapes that reach each path: a
ragged last wave, the scalar and the quads path of the KL kernel, the second grid-stride trip, the slot caps of l2_normalize and
sgd_step, the tail / unaligned / fixed-geometry branches of keep_mask, the C = 2 instances.  Run with -s for one line per check
(worst err / bound)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import ops
from oracle import train_step as ots
from tests import kernel_ref as kr

DEV = torch.device("cuda", 0)


def gen(s):
    return torch.Generator().manual_seed(s)


def report(name, worst):
    print("  %-44s worst err/bound %.3f" % (name, worst))
    return worst


def chk(name, got, ref, bnd, dims="ncdhw"):
    return report(name, kr.check(name, got.cpu(), ref, bnd, dims))


def exact(name, got, ref):
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = got != ref
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s" % (name, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
    print("  %-44s exact (%d elements)" % (name, got.numel()))


def offset_view(t, elems=1):
    """a device copy of t that starts `elems` elements into its buffer (an allocation is 256-byte aligned: the view is not 16-byte aligned)."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=DEV)
    v = buf[elems:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


# ---- losses and pseudo_block --------------------------------------------------------------------------------------------------------
LOSS_SHAPES, loss_inputs = kr.LOSS_SHAPES, kr.loss_inputs


def _dev(t, offset=False):
    return None if t is None else (offset_view(t) if offset else t.to(DEV))


def run_mix(tag, c, *, mask="mask", tb="tb", w=(0.5, 1.0), k=(0.0, 0.0), gscale=1.0, gscale_dev=None, accumulate=False, offset=False):
    lg, ta = c["l1"], c["ta"]
    m = {"mask": c["mask"], None: None, "ones": torch.ones_like(c["mask"]), "zeros": torch.zeros_like(c["mask"])}[mask]
    tbv = c["tb"] if tb == "tb" else None
    ld, tad, tbd, md = _dev(lg, offset), _dev(ta), _dev(tbv), _dev(m)
    loss, acc = ops.mix_loss_fwd(ld, tad, tbd, md, w[0], w[1], k_dice=k[0], k_ce=k[1])
    prior = torch.randn(lg.shape, generator=gen(5)) * 0.01 if accumulate else None
    dl = prior.to(DEV) if accumulate else torch.full(lg.shape, float("nan"), device=DEV)
    gd = None if gscale_dev is None else torch.tensor([gscale_dev], dtype=torch.float32, device=DEV)
    ops.mix_loss_bwd(ld, tad, tbd, md, w[0], w[1], acc, dl, gscale=gscale, accumulate=accumulate, k_dice=k[0], k_ce=k[1], gscale_dev=gd)
    r = kr.mix_loss_ref(lg, ta, tbv, m, w[0], w[1], k_dice=k[0], k_ce=k[1], gscale=gscale,
                        gscale_dev=None if gscale_dev is None else float(torch.tensor(gscale_dev, dtype=torch.float32)), prior=prior)
    NA = 2 + 3 * c["C"]
    chk(tag + " acc", acc[:2 * NA].view(2, NA), r["acc"], r["acc_b"], "ka")
    chk(tag + " loss", loss, r["loss"], r["loss_b"], "k")
    chk(tag + " dlogits", dl, r["dlogits"], r["dlogits_b"])
    assert bool(torch.isfinite(dl).all())


def run_pseudo(tag, c, offset=False):
    r = kr.pseudo_ref(c["l1"], c["l2"])
    s1, s2, a1, a2, kn = ops.pseudo_block(_dev(c["l1"], offset), _dev(c["l2"]))
    near = r["near"]
    share = float(near.double().mean())
    print("  %-44s near-tie share %.2e (cap %.0e)" % (tag, share, kr.NEAR_TIE_CAP))
    assert share <= kr.NEAR_TIE_CAP
    chk(tag + " soft1", s1, r["soft1"], r["soft1_b"])
    chk(tag + " soft2", s2, r["soft2"], r["soft2_b"])
    ok = ~near
    for name, got in (("arg1", a1), ("arg2", a2)):
        got = got.cpu()
        assert got.dtype == torch.int64 and bool((got[ok] == r[name][ok]).all()), (tag, name, int((got[ok] != r[name][ok]).sum()))
    kn = kn.cpu().double()
    chk(tag + " knowledge", torch.where(ok, kn, r["knowledge"]), r["knowledge"], r["knowledge_b"], "ndhw")
    # no-soft variant: the same labels and knowledge
    _, _, b1, b2, kn2 = ops.pseudo_block(_dev(c["l1"], offset), _dev(c["l2"]), want_soft=False)
    assert torch.equal(b1, a1) and torch.equal(b2, a2) and torch.equal(kn2.cpu().double(), kn)


def run_dist(tag, c, mode, *, offset=False, heads=(True, True), with_loss=True, gscale=0.7, gscale_dev=None):
    lg, tg = (c["l1"], c["l2"]), (c["t1"], c["t2"])
    prior = 0.25
    lossd = torch.full((1,), prior, device=DEV) if with_loss else None
    gd = None if gscale_dev is None else torch.tensor([gscale_dev], dtype=torch.float32, device=DEV)
    outs = [torch.full(lg[0].shape, float("nan"), device=DEV) if h else None for h in heads]
    ops.kl_fwd_bwd((_dev(lg[0], offset), _dev(lg[1])), (_dev(tg[0]), _dev(tg[1])), lossd, tuple(outs), gscale=gscale, gscale_dev=gd, mode=mode)
    r = kr.kl_ref(lg, tg, mode, gscale=gscale, gscale_dev=None if gscale_dev is None else float(torch.tensor(gscale_dev, dtype=torch.float32)), prior=prior)
    if with_loss:
        chk("%s %s loss" % (tag, mode), lossd, r["loss"], r["loss_b"], "k")
    for h in range(2):
        if heads[h]:
            chk("%s %s g%d" % (tag, mode, h), outs[h], r["g"][h], r["g_b"][h])


@pytest.mark.parametrize("name", list(LOSS_SHAPES))
def test_losses_and_pseudo_block(name):
    c = loss_inputs(name)
    offs = [False, True] if name == "3d_c2_offset" else [False]        # aligned: the quads path; offset: the scalar one.  Both must pass
    for off in offs:
        tag = name + ("+4B" if off else "")
        run_mix(tag, c, offset=off)
        run_pseudo(tag, c, offset=off)
        run_dist(tag, c, "kl", offset=off)
        run_dist(tag, c, "dice", offset=off)
    torch.cuda.synchronize()


def test_loss_options():
    c = loss_inputs("2d_ragged")
    run_mix("no mask", c, mask=None)
    run_mix("no target_b", c, tb=None)
    run_mix("mask ones (part b empty)", c, mask="ones")
    run_mix("mask zeros (part a empty)", c, mask="zeros")
    run_mix("accumulate", c, accumulate=True, gscale=0.3)
    run_mix("gscale_dev", c, gscale=2.0, gscale_dev=0.37)
    run_mix("k_dice k_ce", c, k=(0.3, 1.7), w=(0.7, 0.3))
    run_mix("k_dice only", c, k=(1.0, 0.0))
    run_dist("head 0 only", c, "kl", heads=(True, False))
    run_dist("head 1 only", c, "kl", heads=(False, True))
    run_dist("no loss", c, "kl", with_loss=False)
    run_dist("gscale_dev", c, "kl", gscale=2.0, gscale_dev=0.37)
    run_dist("head 1 only", c, "dice", heads=(False, True))
    run_dist("gscale_dev", c, "dice", gscale=2.0, gscale_dev=0.37)
    torch.cuda.synchronize()


# ---- VAT helpers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 777, 6149, 256 * 2048 + 777])
def test_l2_normalize(P):
    x = torch.randn(3, P, generator=gen(P))
    x[1] = 0.0                                             # an all-zero sample: exact zeros
    out = torch.full((3, P), float("nan"), device=DEV)
    ops.l2_normalize(x.to(DEV), out)
    ref, b = kr.l2_normalize_ref(x)
    chk("l2_normalize P=%d" % P, out, ref, b, "np")
    assert bool((out[1] == 0).all())


def test_perturb():
    g = gen(31)
    for n in (1, 3, 255, 257, 1003, 70001):
        x, d = torch.rand(n, generator=g), torch.randn(n, generator=g)
        d[::7] = 0.0
        d[3::11] = -0.0
        m = (torch.rand(n, generator=g) > 0.5).float()
        for mask, sign, alpha in ((None, False, 10.0), (m, False, 6.0), (None, True, 0.5), (m, True, 0.013)):
            o = torch.full((n,), float("nan"), device=DEV)
            ops.perturb(x.to(DEV), d.to(DEV), o, alpha, mask=None if mask is None else mask.to(DEV), sign=sign)
            ref, b = kr.perturb_ref(x, d, alpha, mask, sign)
            w = kr.check("perturb", o.cpu(), ref, b, "i")
            if sign:                                       # sgn(+-0) = 0: the input comes back bit for bit
                assert torch.equal(o.cpu()[d == 0], x[d == 0])
        report("perturb n=%d (last variant)" % n, w)


@pytest.mark.parametrize("n", [1, 3, 1003, 2 ** 21 + 1203])
def test_sgd_step(n):
    g = gen(n)
    lr = torch.tensor([0.013], device=DEV)
    for grad2, gscale, zero in ((False, 1.0, False), (True, 1.0, True), (False, 0.25, True), (True, 1.0 / 3.0, False)):
        p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
        g2 = torch.randn(n, generator=g) if grad2 else None
        pd, gd, md, g2d = p.to(DEV), gr.to(DEV), m.to(DEV), None if g2 is None else g2.to(DEV)
        ops.sgd_step(pd, gd, md, lr, 0.9, 1e-4, grad_scale=gscale, zero_grad=zero, grad2=g2d)
        p2, e_p, m2, e_m = kr.sgd_ref(p, gr, m, 0.013, 0.9, 1e-4, gscale, g2)
        wp, wm = kr.check("sgd param", pd.cpu(), p2, e_p, "i"), kr.check("sgd mom", md.cpu(), m2, e_m, "i")
        for t, src in ((gd, gr), (g2d, g2)):
            if t is not None:
                assert torch.equal(t.cpu(), torch.zeros(n) if zero else src)
        report("sgd n=%d grad2=%d gs=%.2f zero=%d" % (n, grad2, gscale, zero), max(wp, wm))


@pytest.mark.parametrize("K", [9, 144, 2305])
@pytest.mark.parametrize("C", [1, 6, 16])
def test_grad_sim(C, K):
    g = gen(C * 10000 + K)
    gl, gu = torch.randn(C, K, generator=g), torch.randn(C, K, generator=g)
    gu[0] = gl[0] * 0.5 + 0.1 * gu[0]                      # one strongly aligned row
    if C > 1:
        gl[C - 1] = 0.0                                    # a zero row: sim = 0
    for ema in (0.0, 0.9):
        s0 = torch.randn(C, generator=g)
        sd = s0.to(DEV)
        ops.grad_sim(gl.to(DEV), gu.to(DEV), sd, ema=ema)
        ref, b = kr.grad_sim_ref(gl, gu, s0, ema)
        chk("grad_sim C=%d K=%d ema=%.1f" % (C, K, ema), sd, ref, b, "c")
        if C > 1 and ema == 0.0:
            assert float(sd[C - 1]) == 0.0


# ---- RNG family -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 65539, 2 ** 20 + 21])
def test_rng_family(n):
    w = 0.0
    for sdv in (None, 0, 5):
        sd = None if sdv is None else torch.tensor([sdv], dtype=torch.int64, device=DEV)
        for p in (0.0, 0.3, 1.0):
            ref = kr.keep_mask_ref(77, n, p, sdv)
            for off in (0, 1):
                buf = torch.full((n + 1 + 16,), 7, dtype=torch.uint8, device=DEV)
                keep = buf[off:off + n]
                ops.keep_mask(keep, 77, p, seed_dev=sd)
                got = buf.cpu()
                assert torch.equal(got[off:off + n], ref), ("keep", n, sdv, p, off, int((got[off:off + n] != ref).sum()))
                assert bool((got[:off] == 7).all()) and bool((got[off + n:] == 7).all()), ("keep wrote outside", n, off)
            mul = torch.full((n,), float("nan"), device=DEV)
            ops.chan_mask(mul, 77, p, seed_dev=sd)
            assert torch.equal(mul.cpu(), kr.chan_mask_ref(77, n, p, sdv)), ("chan", n, sdv, p)
        for lo, hi in ((0.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)):
            out = torch.full((n,), float("nan"), device=DEV)
            ops.rand_uniform(out, 123, lo, hi, seed_dev=sd)
            ref, b = kr.rand_uniform_ref(123, n, lo, hi, sdv)
            w = max(w, kr.check("rand_uniform", out.cpu(), ref, b, "i"))
            assert float(out.min()) >= lo and float(out.max()) < hi
    print("  rng n=%d: keep_mask / chan_mask exact (3 seeds x 3 p, aligned and +1 byte), rand_uniform worst err/bound %.3f" % (n, w))
    if n > 1000:                                           # a present seed word 0 draws the stream of an absent one; 5 draws another
        assert not torch.equal(kr.keep_mask_ref(77, n, 0.3, 0), kr.keep_mask_ref(77, n, 0.3, 5))


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------
BOXES_2D = {"interior": (5, 9, 24, 33), "far corner": (13, 17, 24, 33), "zero size": (4, 6, 0, 0), "zero height": (4, 6, 0, 10),
            "whole": (0, 0, 37, 50), "one pixel": (36, 49, 1, 1)}
BOXES_3D = {"interior": (1, 2, 3, 3, 6, 8), "far corner": (2, 3, 5, 3, 6, 8), "zero size": (1, 1, 1, 0, 0, 0), "whole": (0, 0, 0, 5, 9, 13)}


@pytest.mark.parametrize("dims", [2, 3])
def test_boxes(dims):
    g = gen(40 + dims)
    N, shape, boxes = (3, (37, 50), BOXES_2D) if dims == 2 else (2, (5, 9, 13), BOXES_3D)
    a, b = torch.rand(N, 1, *shape, generator=g), torch.rand(N, 1, *shape, generator=g)
    ai, bi = torch.randint(-5, 2 ** 40, (N, *shape), generator=g), torch.randint(-5, 2 ** 40, (N, *shape), generator=g)
    for name, box in boxes.items():
        bd = torch.tensor(box, dtype=torch.int32, device=DEV)
        o = torch.full(a.shape, float("nan"), device=DEV)
        ops.box_mix(a.to(DEV), b.to(DEV), o, bd)
        exact("box_mix f32 %dD %s" % (dims, name), o, kr.box_mix_ref(a, b, box))
        oi = torch.full(ai.shape, -77, dtype=torch.int64, device=DEV)
        ops.box_mix(ai.to(DEV), bi.to(DEV), oi, bd)
        exact("box_mix i64 %dD %s" % (dims, name), oi, kr.box_mix_ref(ai, bi, box))
        lm = torch.full((N, *shape), -77, dtype=torch.int64, device=DEV)
        ops.box_mask(lm, bd)
        exact("box_mask %dD %s" % (dims, name), lm, kr.box_mask_ref(N, shape, box))


# ---- largest connected component ------------------------------------------------------------------------------------------------------
spiral, serpentine = kr.spiral, kr.serpentine


def lcc_cases_2d():
    H, W, g = 67, 131, gen(50)
    cases = {}
    cases["spiral"] = spiral(H, W, cut=0.4)                # cut once: two long arms of different size; the larger must be kept whole
    cases["serpentine"] = serpentine(H, W)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cb = ((yy + xx) % 2 == 0).long()                       # one component through diagonals only
    cb[:, 64:66] = 0                                       # ... cut into two halves of different size
    cases["checkerboard"] = cb
    cases["interleaved"] = torch.where((yy + xx) % 2 == 0, 1, 2) * ((yy // 9 + xx // 11) % 3 != 0).long()
    cases["noise"] = (torch.rand(H, W, generator=g) < 0.5).long() * torch.randint(1, 4, (H, W), generator=g)
    odd = torch.randint(0, 4, (H, W), generator=g)
    odd[torch.rand(H, W, generator=g) < 0.1] = 4           # = num_classes
    odd[torch.rand(H, W, generator=g) < 0.1] = 7           # = num_classes + 3
    odd[torch.rand(H, W, generator=g) < 0.1] = -1
    cases["labels out of range"] = odd
    tie = torch.zeros(H, W, dtype=torch.int64)             # equal sizes: the component met first in raster order
    tie[10:14, 100:105] = 2; tie[12:16, 20:25] = 2; tie[50:52, 3:13] = 2
    tie[30, 5:70] = 1; tie[31, 66:131] = 3; tie[33, 0:65] = 3
    cases["tie"] = tie
    return cases


def staircase(D, H, W):
    """voxels linked through corners only: (z, y, x) -> (z + 1, y + 1, x + 1) (26-connectivity)."""
    v = torch.zeros(D, H, W, dtype=torch.int64)
    for i in range(min(D, H, W)):
        v[i, i, i] = 1
    for i in range(min(D, H - 3, W - 9) - 2):              # a shorter second one
        v[i, i + 3, i + 9] = 1
    return v


def helix(D, H, W):
    v = torch.zeros(D, H, W, dtype=torch.int64)
    for s in range(400):
        a = s * 0.05
        z, y, x = min(D - 1, int(s * D / 400)), int(round(H / 2 - 0.5 + (H / 2 - 1) * np.sin(a))), int(round(W / 2 - 0.5 + (W / 2 - 1) * np.cos(a)))
        v[z, y, x] = 1
    return v


def lcc_cases_3d():
    D, H, W, g = 7, 11, 21, gen(51)
    tie = torch.zeros(D, H, W, dtype=torch.int64)
    tie[4:6, 1:3, 1:3] = 1; tie[1:3, 7:9, 15:17] = 1       # two 2x2x2 cubes: the one in the lower plane wins
    return {"staircase": staircase(D, H, W), "helix": helix(D, H, W),
            "noise": (torch.rand(D, H, W, generator=g) < 0.15).long() * torch.randint(1, 3, (D, H, W), generator=g), "tie": tie}


def run_lcc(name, lab, ncls):
    ref = ots.largest_cc(torch.where((lab > 0) & (lab < ncls), lab, torch.zeros_like(lab)), ncls)
    ld = lab.to(DEV)
    got, again = ops.largest_cc(ld, ncls), ops.largest_cc(ld, ncls)
    assert torch.equal(got, again), name + ": two runs differ"
    exact("largest_cc " + name, got, ref)
    assert int(ref.sum()) > 0


def test_largest_cc_2d():
    cases = lcc_cases_2d()
    # the cut spiral / checkerboard are two components each (scipy agrees with the construction): the test would not notice a missing union otherwise
    from scipy import ndimage
    assert ndimage.label(cases["spiral"].numpy(), structure=np.ones((3, 3)))[1] == 2
    assert ndimage.label(cases["serpentine"].numpy(), structure=np.ones((3, 3)))[1] == 1
    assert ndimage.label(cases["checkerboard"].numpy(), structure=np.ones((3, 3)))[1] == 2
    for name, im in cases.items():
        run_lcc("2D " + name, torch.stack([im, im.flip(0), im.flip(1)]), 4)
    g = gen(52)
    many = torch.randint(0, 4, (65, 8, 9), generator=g)    # N * num_classes = 260 > 256: the global-atomic branch of lcc_best_kernel
    run_lcc("2D N=65", many, 4)


def test_largest_cc_3d():
    for name, v in lcc_cases_3d().items():
        run_lcc("3D " + name, torch.stack([v, v.flip(2)]), 3)


# ---- diff mask --------------------------------------------------------------------------------------------------------------------------
def diff_case(shape, seed, ties=None):
    g = gen(seed)
    N = shape[0]
    H, W = (shape[1], shape[2]) if len(shape) == 3 else (shape[1] * shape[2], shape[3])
    kn = kr.exact_knowledge(N, H, W, 4, g, ties=ties).reshape(shape)
    p1 = torch.randint(0, 4, shape, generator=g)
    p2 = torch.where(torch.rand(shape, generator=g) < 0.02, (p1 + 1) % 4, p1)
    return p1, p2, kn


def run_diff(name, shape, topk, seed, ties=None):
    p1, p2, kn = diff_case(shape, seed, ties)
    M = kn[0].numel() // 16
    k = kr.diff_mask_k(topk, M)
    ref = kr.diff_mask_ref(p1, p2, kn, 4, k)
    assert torch.equal(ref, ots.create_mask_v1(p1, p2, kn, 4, topk))            # the exact construction: fp32 and fp64 pooling agree
    got = ops.diff_mask(p1.to(DEV), p2.to(DEV), kn.to(DEV), 4, topk)
    sel = ref.reshape(shape[0], -1).sum(1)
    exact("diff_mask %s topk=%g (k=%d of %d)" % (name, topk, k, M), got, ref)
    return k, sel


@pytest.mark.parametrize("shape,topk", [((3, 40, 40), 0.1), ((3, 40, 40), 0.29), ((3, 40, 40), 1e-6), ((3, 40, 40), 1.0),
                                        ((2, 60, 96), 0.35), ((2, 60, 96), 0.7), ((2, 6, 20, 24), 0.1), ((2, 6, 20, 24), 0.29)])
def test_diff_mask(shape, topk):
    k, _ = run_diff("x".join(map(str, shape)), shape, topk, 60 + len(shape))
    M = int(np.prod(shape[1:])) // 16
    assert k == max(int(topk * M), 1)
    if (topk, M) in ((0.29, 100), (0.35, 360), (0.7, 360)):                        # the counts a float product gets wrong (one too many)
        assert int(np.float32(topk) * np.float32(M)) == k + 1


def test_diff_mask_ties_at_the_threshold():
    """three further cells carry the k-th largest value: `>= threshold` selects all of them (k + 3 cells)."""
    shape, topk = (3, 40, 40), 0.29
    p1, p2, kn = diff_case(shape, 70, ties=(28, 3))
    ref = kr.diff_mask_ref(p1, p1, kn, 4, 28)
    assert bool((ref.reshape(3, -1).sum(1) == (28 + 3) * 16).all())
    exact("diff_mask ties (no disagreement)", ops.diff_mask(p1.to(DEV), p1.to(DEV), kn.to(DEV), 4, topk), ref)
    run_diff("ties", shape, topk, 70, ties=(28, 3))
