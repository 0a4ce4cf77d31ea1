"""The evaluation kernels (ensemble_argmax, window_accumulate / _finalize), the channel-drop kernels (sample_channel_sum, channel_drop,
fold_perturbed), bn_finalize / bn_eval_affine, channel_sum, the layout converters and chap_pack_multi per element against the fp64
restatements and bounds of tests/kernel_ref.py (or bit for bit, where the result is a copy, a mask, a count or a label), at the smallest
shapes that reach each path: C = 1 and C = 8 of the inference softmax, logits far into the underflow of its exp, uncovered voxels, a
second grid-stride trip, every slot count of bn_finalize's lane loop, block-row counts below / across / above the slot cap of the channel
sums, channel slices with canaries beside them, U * C at the documented limit of channel_drop (last in the file).  Outputs the caller
allocates are poisoned with NaN before the call.  Run with -s for one line per check (worst err / bound)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib, ops
from tests import kernel_ref as kr

DEV = torch.device("cuda", 0)
NAN = float("nan")
LOSS_BLOCKS = 2048                                         # the block cap of loss_blocks (csrc/loss.hip) and of chap_fold_perturbed's grid (csrc/chandrop.hip): not exported
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def gen(s):
    return torch.Generator().manual_seed(s)


def report(name, worst):
    print("  %-52s worst err/bound %.3f" % (name, worst))
    return worst


def chk(name, got, ref, bnd, dims="ncdhw"):
    return report(name, kr.check(name, got, ref, bnd, dims))


def same_bits(name, got, ref):
    """bit for bit, NaN canaries included."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    iv = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[got.element_size()]
    bad = got.contiguous().view(iv).cpu() != ref.contiguous().view(iv).cpu()
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s" % (name, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
    print("  %-52s exact (%d elements)" % (name, got.numel()))


def labels_match(name, got, r):
    near = r["near"]
    share = float(near.double().mean())
    assert share <= kr.NEAR_TIE_CAP, (name, "near ties", int(near.sum()), near.numel())
    ok = ~near
    bad = (got.long()[ok] != r["label"].to(got.device)[ok])
    assert not bool(bad.any()), "%s: %d labels differ" % (name, int(bad.sum()))
    print("  %-52s labels equal; near-tie share %.2e" % (name, share))


# ---- inference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", list(kr.ENSEMBLE_SCALES))
def test_ensemble_argmax(mode, C):
    """5 x (37 * 41) pixels (ragged).  The probabilities are checked at the scales (1, 8, 30) (|z - max| up to ~100: beyond the underflow of the exp) in
    every mode; the labels at the mode's own scales (kr.ENSEMBLE_SCALES; tests/test_kernel_ref_cpu.py asserts their near-tie share)."""
    for scales in {(1.0, 8.0, 30.0), kr.ENSEMBLE_SCALES[mode]}:
        a, b = kr.ensemble_inputs(C, scales)
        r = kr.ensemble_ref(a, b, mode)
        label, p = ops.ensemble_argmax(a.to(DEV), b.to(DEV), mode, want_prob=True)
        chk("ensemble %s C=%d scales %s" % (mode, C, scales), p.cpu(), r["p"], r["e_p"])
        if scales == kr.ENSEMBLE_SCALES[mode]:
            labels_match("ensemble %s C=%d" % (mode, C), label.cpu(), r)
        assert int(label[0, 0, 0]) == 0                    # an exact tie of all classes: the first index
        label2, _ = ops.ensemble_argmax(a.to(DEV), b.to(DEV), mode)      # without the probabilities
        assert torch.equal(label, label2)


@pytest.mark.parametrize("mode", list(kr.ENSEMBLE_SCALES))
def test_ensemble_argmax_second_grid_stride_trip(mode):
    N, sp = kr.ENSEMBLE_TWO_TRIPS                          # 526 683 pixels > the block cap * 256 threads
    assert N * sp[0] * sp[1] > LOSS_BLOCKS * 256
    a, b = (t.to(DEV) for t in kr.ensemble_inputs(2, kr.ENSEMBLE_SCALES[mode], N=N, sp=sp))
    r = kr.ensemble_ref(a, b, mode)                        # fp64 on the device
    label, p = ops.ensemble_argmax(a, b, mode, want_prob=True)
    chk("ensemble %s two trips" % mode, p, r["p"], r["e_p"])
    labels_match("ensemble %s two trips" % mode, label, r)


def _window_run(C, vol, patch, calls, seed=5):
    logits, s0, c0 = kr.window_inputs(C, vol, patch, calls, seed)
    big = s0[0].numel() > 100000
    dev = DEV if big else torch.device("cpu")              # the restatement runs on the device for the large volume
    tag = "window C=%d vol=%s" % (C, "x".join(map(str, vol)))
    outs = []
    for rep in range(2):
        score, cnt = s0.to(DEV), c0.to(DEV)
        for lg, org in zip(logits, calls):
            before_s, before_c = score.clone(), cnt.clone()
            ops.window_accumulate(lg.to(DEV), torch.tensor(org, dtype=torch.int32, device=DEV), score, cnt)
            if rep == 0:
                r = kr.window_accumulate_ref(lg.to(dev), org, before_s.to(dev), before_c.to(dev))
                chk(tag + " score", score.to(dev), r["score"], r["score_b"], "cxyz")
                same_bits(tag + " cnt", cnt.to(dev), r["cnt"].float())
                unc = ~r["covered"]
                assert torch.equal(score.to(dev)[:, unc], before_s.to(dev)[:, unc])
        acc_s, acc_c = score.clone(), cnt.clone()
        label = ops.window_finalize(score, cnt)
        outs.append((acc_s, acc_c, score.clone(), label))
    for t0, t1 in zip(*outs):                              # no atomics: a second run gives the same bits (NaN included)
        same_bits(tag + " run twice", t1, t0)
    acc_s, acc_c, fin_s, label = (t.to(dev) for t in outs[0])
    r = kr.window_finalize_ref(acc_s, acc_c)
    empty = r["empty"]
    chk(tag + " finalize", torch.where(empty.unsqueeze(0), torch.zeros_like(fin_s), fin_s), r["score"], r["score_b"], "cxyz")
    assert bool(torch.isnan(fin_s[:, empty]).all()) and not bool(label[empty].any())      # 0 / 0: NaN scores, label 0
    labels_match(tag, label, r)
    return r


@pytest.mark.parametrize("C", [1, 2, 8])
def test_window_accumulate_finalize(C):
    r = _window_run(C, **kr.WINDOW_CASE)
    assert bool(r["empty"].any())                          # an uncovered voxel with nothing in it exists
    _window_run(C, (12, 10, 8), (12, 10, 8), (((0, 0, 0),), ((0, 0, 0), (0, 0, 0))), seed=6)      # the patch is the volume


def test_window_second_grid_stride_trip():
    vol = (82, 80, 81)
    assert vol[0] * vol[1] * vol[2] > LOSS_BLOCKS * 256
    r = _window_run(2, vol, (40, 48, 40), (((42, 32, 41), (0, 0, 0)), ((20, 10, 30),)), seed=7)
    assert bool(r["empty"].any())


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------
def _bn_buffer(C, nsub, nslots, g, count_one=False):
    """header word, then [slot][S | Q][Clog], NaN in every slot not in use.  Values are multiples of 2^-6; channel 0 has Q / n < (S / n)^2."""
    Clog = C * nsub
    buf = torch.full((ops.stats_size(Clog),), NAN)
    body = buf[_lib.STATS_HDR:].view(_lib.STATS_MAX_SLOTS, 2, Clog)
    r = lambda *s: torch.randint(-256, 256, s, generator=g).float() / 64
    body[:nslots, 0] = r(nslots, Clog) * 4
    body[:nslots, 1] = r(nslots, Clog).abs() * 64 + 40
    if count_one:
        body[0, 0] = r(Clog)
        body[0, 1] = body[0, 0] ** 2                       # one value: Q = S^2 exactly
        count = 1
    else:
        count = 64 * nslots * nsub
        body[:nslots, 0].view(nslots, nsub, C)[:, :, 0] = 8.0
        body[:nslots, 1].view(nslots, nsub, C)[:, :, 0] = 0.5
    buf[:1].view(torch.int32).fill_(nslots)
    buf[1:_lib.STATS_HDR] = 0
    return buf, body, count


def _bn_run(tag, C, nsub, nslots, g, *, shift, want_mean, running, momentum, count_one=False):
    buf, body, count = _bn_buffer(C, nsub, nslots, g, count_one)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    sh = torch.randn(C, generator=g) * 0.5 if shift else None
    rm, rv = (torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5) if running else (None, None)
    d = lambda t: None if t is None else t.to(DEV)
    outs = {k: torch.full((C + 3,), NAN, device=DEV) for k in ("scale", "shift", "mean", "invstd")}      # three canaries past the end of each
    rmd, rvd = d(rm), d(rv)
    nbt = torch.full((1,), 5, dtype=torch.int64, device=DEV) if running else None
    ops.bn_finalize(buf.to(DEV), d(gam), d(bet), rmd, rvd, nbt, count, 1e-5, momentum, outs["scale"], outs["shift"],
                    mean=outs["mean"] if want_mean else None, invstd=outs["invstd"] if want_mean else None, stats_shift=d(sh), clog=C * nsub)
    ref = kr.bn_finalize_ref(body, nslots, C, C * nsub, count, sh, gam, bet, rm, rv, momentum, 1e-5)
    worst = 0.0
    for k, t in outs.items():
        if k in ("mean", "invstd") and not want_mean:
            assert bool(torch.isnan(t).all())
            continue
        worst = max(worst, kr.check("%s %s" % (tag, k), t[:C].cpu(), ref[k][0], ref[k][1], "c"))
        assert bool(torch.isnan(t[C:]).all()), (tag, k, "canary")
    if running and momentum > 0:
        worst = max(worst, kr.check(tag + " running_mean", rmd.cpu(), *ref["running_mean"], "c"), kr.check(tag + " running_var", rvd.cpu(), *ref["running_var"], "c"))
        assert int(nbt) == 6
    elif running:                                          # momentum == 0: nothing of the running state moves
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv) and int(nbt) == 5
    if not count_one:
        assert abs(float(ref["invstd"][0][0]) * kr._fp32_scalar(1e-5) ** 0.5 - 1.0) < 1e-12              # channel 0: Q / n < (S / n)^2, the clamp at 0
    return worst


@pytest.mark.parametrize("nslots", [1, 63, 64, 65, 1024])
def test_bn_finalize_slots_sublattices_and_state(nslots):
    g = gen(40 + nslots)
    worst, i = 0.0, 0
    for C in (6, 16, 256):
        for nsub in (1, 4, 8):
            kw = [dict(shift=True, want_mean=True, running=True, momentum=0.1), dict(shift=False, want_mean=False, running=False, momentum=0.1),
                  dict(shift=True, want_mean=True, running=True, momentum=0.0), dict(shift=False, want_mean=True, running=True, momentum=1.0)][i % 4]
            i += 1
            worst = max(worst, _bn_run("bn_finalize C=%d x%d slots=%d" % (C, nsub, nslots), C, nsub, nslots, g, **kw))
    report("bn_finalize nslots=%d (9 shapes)" % nslots, worst)


def test_bn_finalize_count_one():
    g = gen(39)
    for C, nsub in ((6, 1), (16, 4)):
        report("bn_finalize count=1 C=%d x%d" % (C, nsub), _bn_run("bn_finalize count=1", C, nsub, 1, g, shift=True, want_mean=True, running=True, momentum=0.1, count_one=True))


@pytest.mark.parametrize("C", [1, 63, 64, 65, 256])
def test_bn_eval_affine(C):
    g = gen(50 + C)
    gam, bet, rm = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) * 2
    rv[0] = 0.0
    rv[C // 2] = 1e6
    if C > 2:
        rv[C - 1] = 0.0
    scale, shift = torch.full((C + 3,), NAN, device=DEV), torch.full((C + 3,), NAN, device=DEV)
    ops.bn_eval_affine(gam.to(DEV), bet.to(DEV), rm.to(DEV), rv.to(DEV), 1e-5, scale, shift)
    (sc, e_sc), (sh, e_sh) = kr.bn_eval_ref(gam, bet, rm, rv, 1e-5)
    chk("bn_eval scale C=%d" % C, scale[:C].cpu(), sc, e_sc, "c"), chk("bn_eval shift C=%d" % C, shift[:C].cpu(), sh, e_sh, "c")
    assert bool(torch.isnan(scale[C:]).all()) and bool(torch.isnan(shift[C:]).all())


# ---- lazy sources ---------------------------------------------------------------------------------------------------------------------
def make_lazy(dtype, N, sp3, C, g, *, lazy=True, coff=0, ld=None, keep=True):
    """a Lazy over raw [N, *sp3, ld] whose channels outside [coff, coff + C) hold 1e30 (a kernel that reads beside its slice shows); affine + leaky (+ keep)
    + chan_mul when `lazy`."""
    ld = ld or C
    raw = torch.full((N, *sp3, ld), 1e30)
    raw[..., coff:coff + C] = torch.randn(N, *sp3, C, generator=g)
    raw = raw.to(dtype).to(DEV)
    if not lazy:
        return ops.Lazy(raw, C=C, coff=coff)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    kp = (torch.rand(N, *sp3, C, generator=g) > 0.3).to(torch.uint8).to(DEV) if keep else None
    cm = ((torch.rand(N, C, generator=g) > 0.3).float() * 1.5).to(DEV)
    return ops.Lazy(raw, sc, sh, True, 0.01, kp, 1.25, cm, C=C, coff=coff)


def lazy_ref(lz, dev=None):
    """kr.lazy_f32 of a Lazy: (v, dv) [N, C, D, H, W] fp64 on `dev` (default: the CPU)."""
    dev = dev or torch.device("cpu")
    t = lambda x: None if x is None else x.to(dev)
    x = t(lz.raw)[..., lz.coff:lz.coff + lz.C].permute(0, 4, 1, 2, 3)
    keep = None if lz.keep is None else t(lz.keep).permute(0, 4, 1, 2, 3)
    return kr.lazy_f32(x, scale=t(lz.scale), shift=t(lz.shift), act=lz.act, slope=lz.slope, keep=keep, keep_scale=lz.keep_scale, chan_mul=t(lz.chan_mul))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 16, 64, 512])
def test_channel_sum(C, dtype):
    dt = DT[dtype]
    rows = 256 // (C // 8)                                 # pixels a block sums per trip
    g = gen(60 + C)
    cases = [("fewer pixels than a block's rows", 1, (1, 1, max(rows - 1, 1) if rows > 1 else 1), False, 0, C),
             ("ragged, lazy, sample boundaries inside a block", 3, (1, 37, 23), True, 0, C),
             ("a channel slice, lazy", 3, (1, 9, 7), True, 8, C + 16),
             ("above the slot cap", 1, (1, 1, _lib.CHANSUM_SLOTS * rows + 77), False, 8, C + 16)]
    for name, N, sp3, lazy, coff, ld in cases:
        lz = make_lazy(dt, N, sp3, C, g, lazy=lazy, coff=coff, ld=ld)
        prior = torch.randn(C, generator=g)
        outs = []
        for rep in range(2):
            out = torch.full((C + 3,), NAN, device=DEV)
            out[:C] = prior.to(DEV)
            ops.channel_sum(lz, out)
            outs.append(out)
        same_bits("channel_sum twice", outs[1], outs[0])
        ref, b = kr.channel_sum_ref(lazy_ref(lz), prior)
        chk("channel_sum C=%d %s: %s" % (C, dtype, name), outs[0][:C].cpu(), ref, b, "c")
        assert bool(torch.isnan(outs[0][C:]).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 32, 256, 2048])
def test_sample_channel_sum(C, dtype):
    dt = DT[dtype]
    g = gen(70 + C)
    for nchunk, N, sp3, lazy in ((1, 2, (1, 9, 7), True), (7, 3, (1, 20, 12), True), (32, 3, (1, 1, 5), False), (32, 2, (1, 33, 29), True)):
        if C == 2048:
            sp3 = (1, 1, min(sp3[2], 11))
        lz = make_lazy(dt, N, sp3, C, g, lazy=lazy)         # lazy: affine + leaky, keep and chan_mul
        part = ops.sample_channel_sum(lz, nchunk=nchunk)
        assert tuple(part.shape) == (N, nchunk, C)
        r = kr.sample_channel_sum_ref(lazy_ref(lz))
        tot = part.double().sum(1).cpu()
        P = sp3[0] * sp3[1] * sp3[2]
        tag = "sample_channel_sum C=%d %s nchunk=%d P=%d" % (C, dtype, nchunk, P)
        chk(tag + " sum", tot, r["sum"], r["sum_b"], "nc"), chk(tag + " mean", tot / P, r["mean"], r["mean_b"], "nc")
        assert torch.equal(part, ops.sample_channel_sum(lz, nchunk=nchunk))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fold_perturbed(dtype):
    dt = DT[dtype]
    g = gen(80)
    B, C, coff = 4, 24, 8
    for U in (0, B // 2, B):
        for with_mul in (True, False):
            gfull = torch.full((B + U, 1, 5, 7, C + 16), 1e30)      # 35 pixels * 3 groups of 8 channels * 4 samples: ragged against 256
            gfull[..., coff:coff + C] = torch.randn(B + U, 1, 5, 7, C, generator=g)
            gfull = gfull.to(dt)
            mul = torch.cat((torch.full((B, C), NAN), (torch.rand(U, C, generator=g) > 0.4).float() * 1.7)) if with_mul else None
            out = ops.fold_perturbed(gfull.to(DEV), coff, C, None if mul is None else mul.to(DEV), B, U)
            ref, b = kr.fold_ref(gfull, coff, C, mul, B, U, dt)
            assert out.dtype == dt and tuple(out.shape) == (B, 1, 5, 7, C)
            chk("fold %s U=%d mul=%s" % (dtype, U, with_mul), out.cpu(), ref, b, "ndhwc")
            same_bits("fold copies", out[:B - U], gfull[:B - U, ..., coff:coff + C].contiguous().to(DEV))


def test_fold_perturbed_second_grid_stride_trip():
    B, U, C, sp3 = 2, 1, 8, (1, 437, 600)                  # 2 * 262 200 units of 8 channels > the block cap * 256
    assert B * sp3[1] * sp3[2] * (C // 8) > LOSS_BLOCKS * 256
    g = torch.Generator(device=DEV).manual_seed(81)
    gfull = torch.randn(B + U, *sp3, C + 16, generator=g, device=DEV).bfloat16()
    mul = torch.rand(B + U, C, generator=g, device=DEV) * 2
    out = ops.fold_perturbed(gfull, 8, C, mul, B, U)
    ref, b = kr.fold_ref(gfull, 8, C, mul, B, U, torch.bfloat16)
    chk("fold two trips", out, ref, b, "ndhwc")


# ---- layout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_planar_to_cl(dtype):
    dt = DT[dtype]
    g = gen(90)
    #        C  ld  coff cpad   (scalar path: the vector path needs max(C, cpad), ld and coff all multiples of 8)
    cases = [(1, 1, 0, 0), (3, 3, 0, 0), (3, 12, 4, 5), (1, 16, 0, 16), (4, 8, 0, 8), (3, 8, 0, 8), (3, 32, 8, 8), (16, 32, 8, 0)]
    for C, ld, coff, cpad in cases:
        x = torch.randn(2, C, 3, 9, 7, generator=g)
        x[0, 0, 0, 0, :4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -20])      # bf16 ties (to even) and just above one
        x[1, C - 1, 2, 8, :2] = torch.tensor([3.0e38, -3.4e38])              # the second rounds to -inf in bf16
        out0 = torch.full((2, 3, 9, 7, ld), NAN, dtype=dt)
        out = out0.to(DEV)
        ops.planar_to_cl(x.to(DEV), out, out_coff=coff, cpad=cpad)
        same_bits("planar_to_cl %s C=%d ld=%d coff=%d cpad=%d" % (dtype, C, ld, coff, cpad), out, kr.planar_to_cl_ref(x, out0, coff, cpad))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [2, 4, 16])
def test_cl_to_planar(C, dtype):
    dt = DT[dtype]
    g = gen(95 + C)
    for lazy, coff, ld in ((False, 0, C), (True, 0, C), (False, 8, C + 16), (True, 8, C + 16)):
        lz = make_lazy(dt, 3, (3, 5, 7), C, g, lazy=lazy, coff=coff, ld=ld)
        n = 3 * C * 105
        buf = torch.full((n + 5,), NAN, device=DEV)
        out = buf[:n].view(3, C, 3, 5, 7)
        ops.cl_to_planar(lz, out)
        v, dv = lazy_ref(lz)                               # the output is the lazy value itself
        tag = "cl_to_planar %s C=%d lazy=%s coff=%d" % (dtype, C, lazy, coff)
        if lazy:
            chk(tag, out.cpu(), v, dv)
        else:
            same_bits(tag, out, v.float().to(DEV))
        assert bool(torch.isnan(buf[n:]).all())


# ---- chap_pack_multi: every weight of a step in one launch == chap_pack_weights one by one ----------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("net", ["dualdecoder2d", "vnet"])
def test_pack_multi_equals_pack_weights(net, dtype):
    from chap_amd import engine
    if net == "dualdecoder2d":
        from chap_amd.networks import DualDecoder
        m = DualDecoder(1, 4, {"decoder_type": "mcnet"}).to(DEV)
    else:
        from chap_amd.networks import net_factory_3d
        m = net_factory_3d("vnet", 1, 2, "train", DEV)
    dt = DT[dtype]
    ex = m._exec
    sd = ex._sd()
    tab = ex._build_pack_table(dt, sd)
    for buf in tab["bufs"].values():
        buf.fill_(0xA5)
    _lib.pack_multi(tab["table"].data_ptr(), tab["n"], tab["max_total"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    seen = set()
    for op in ex.prog.ops:
        for kind in ex._pack_kinds(op):
            w = sd[op.w]
            cin, cout = (w.shape[0], w.shape[1]) if op.kind == "deconv" else (w.shape[1], w.shape[0])
            one = ops.pack_weights(w, kind, dt, cin, cout, engine._taps(op, ex.prog.dims))
            got = tab["bufs"][(op.w, kind)]
            assert got.numel() == one.numel() and torch.equal(got, one), (op.w, kind, dtype)
            seen.add((op.kind, kind))
    assert len(tab["bufs"]) == tab["n"] and len(seen) >= 4
    print("  pack_multi %s %s: %d entries byte-identical, (op, pack kind) pairs %s" % (net, dtype, tab["n"], sorted(seen)))


# ---- channel_drop (last: its final case launches at the documented limit U * C = 16384) ---------------------------------------------------
def _drop_check(tag, U, C, B, mode, kind="sigmoid", comp=False, branch=0, zero_scores=False, all_dropped=False):
    c = kr.channel_drop_inputs(U, C, prob_kind=kind, comp=comp, branch=branch)
    if zero_scores:
        c["gs"] = torch.zeros(C)
    if all_dropped:
        c["u1"] = torch.ones(U, C)                         # u < q never holds: an empty first mask
    buf1, buf2 = torch.full((B + U + 1, C), NAN, device=DEV), torch.full((B + U + 1, C), NAN, device=DEV)      # one canary row past the end
    probs = torch.full((U + 1, C), NAN, device=DEV)
    kw = {}
    if mode == "scores":
        kw = dict(pool_partial=c["part"].to(DEV), npix=c["npix"], grad_sim=c["gs"].to(DEV), comp=comp, branch=branch, prob_kind=kind, probs_out=probs[:U])
    ops.channel_drop(buf1[:B + U], buf2[:B + U], c["u1"].to(DEV), c["u2"].to(DEV), B, mode, **kw)
    r = kr.channel_drop_ref(c["u1"], c["u2"], B, mode, **{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in kw.items() if k != "probs_out"})
    assert bool(torch.isnan(buf1[B + U:]).all()) and bool(torch.isnan(buf2[B + U:]).all()) and bool(torch.isnan(probs[U:]).all())
    if r["mode"] != "scores":
        assert bool(torch.isnan(probs).all())
    return kr.channel_drop_check(tag, r, B, buf1[:B + U].cpu(), buf2[:B + U].cpu(), probs[:U].cpu())


@pytest.mark.parametrize("U,C", kr.DROP_SHAPES)
def test_channel_drop(U, C):
    worst = 0.0
    for B in (U, 2 * U):
        for mode in ("dropout2d", "comp_binomial"):
            worst = max(worst, _drop_check("channel_drop %s U=%d C=%d B=%d" % (mode, U, C, B), U, C, B, mode))
        for kind in ("sigmoid", "gauss"):
            for comp, branch in ((False, 0), (True, 0), (True, 1)):
                tag = "channel_drop scores %s comp=%d branch=%d U=%d C=%d B=%d" % (kind, comp, branch, U, C, B)
                worst = max(worst, _drop_check(tag, U, C, B, "scores", kind, comp, branch))
    worst = max(worst, _drop_check("channel_drop zero scores U=%d C=%d" % (U, C), U, C, U, "scores", zero_scores=True))
    worst = max(worst, _drop_check("channel_drop empty mask U=%d C=%d" % (U, C), U, C, U, "scores", all_dropped=True))
    report("channel_drop U=%d C=%d (18 configurations)" % (U, C), worst)
