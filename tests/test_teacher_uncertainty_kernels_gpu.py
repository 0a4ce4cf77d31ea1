"""chap_teacher_uncertainty and chap_teacher_consistency_masked per element against the fp64 restatements and bounds of tests/uncertainty_ref.py,
at every class count 2..8 and T = 1, 2, 3, 8 noisy passes.  Shapes: 4 x C x 17 x 19 (P % 4 = 3: the one-pixel path, ragged last wave),
4 x C x 16 x 20 on aligned tensors (the four-pixel path, the mask as 32-bit words), the same shape with one fp32 tensor a float into its buffer
and with the mask a byte into its buffer (both: the one-pixel path again) and, at C = 2 and 8 with T = 2, 3 x C x 420 x 420 (a second grid-stride
trip).  Thresholds 0.75 ln C and 0.9 ln C.  Both entries are called through their parameter structs on buffers whose every byte is 0xff
beforehand (NaN as fp32, -1 as int64, 255 as a mask byte): behind every output, in the workspace rows a launch does not use, in `loss` and
`count`.  Threshold 0 is not "count = 0" on these inputs -- a saturated pixel has H = -log(1 + 1e-6) < 0, inside its own rounding band of
0 -- so the uncertainty kernel's empty mask is taken at threshold -1 and count = 0 reaches the masked kernel with an all-zero mask.  Run with -s for one JSON line per case
(profiles/teacher_uncertainty_kernels.jsonl holds those lines)."""
import functools
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from tests import kernel_ref as kr
from tests import teacher_ref as tr
from tests import uncertainty_ref as ur

DEV = torch.device("cuda", 0)
GUARD = 256             # bytes


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, dtype=torch.float32, fill=None, offset=0):
    """(view of `shape` starting `offset` elements into a fresh buffer, the GUARD bytes right behind it, the bytes in front); every byte 0xff unless filled."""
    item = torch.empty((), dtype=dtype).element_size()
    n = int(torch.Size(shape).numel()) * item
    buf = torch.full((offset * item + n + GUARD,), 255, dtype=torch.uint8, device=DEV)
    v = buf[offset * item:offset * item + n].view(dtype).view(shape)
    if fill is not None:
        v.copy_(fill)
    return v, buf[offset * item + n:], buf[:offset * item]


def untouched(name, *guards):
    for g in guards:
        assert bool((g.contiguous().view(torch.uint8) == 255).all()), "%s: a guard byte next to it was written" % name


def blocks_of(N, P, quads):
    units = N * P // 4 if quads else N * P
    return min((units + 255) // 256, L.LOSS_SLOTS)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=4)
def case_inputs(C, shape, T):
    return ur.inputs(C, shape, T)


def launch_unc(x, thr, *, offset=0, mask_offset=0, entropy=True, thr_dev=False, quads=None):
    """One call through the struct -> dict(mask, count, H (or None), ws, nb)."""
    N, C, T, P = x["N"], x["C"], x["T"], x["P"]
    shape = x["t"][0][0].shape
    ins = [[guarded(shape, fill=z) for z in pair] for pair in x["t"]]
    ins[T - 1][1] = guarded(shape, fill=x["t"][T - 1][1], offset=offset)         # the misaligned case: the last pass's second head one float in
    sp = (N,) + tuple(shape[2:])
    mask, mask_g, mask_f = guarded(sp, torch.uint8, offset=mask_offset)
    H = guarded(sp) if entropy else None
    count, count_g, _ = guarded((1,), torch.int64)
    ws, ws_g, _ = guarded((1 + L.LOSS_SLOTS,), torch.int64)
    td = torch.tensor([thr], dtype=torch.float32, device=DEV) if thr_dev else None
    p = L.TeacherUncertaintyParams()
    for k in range(T):
        for h in range(2):
            p.teacher[k][h] = ins[k][h][0].data_ptr()
    aligned = P % 4 == 0 and all(t[0].data_ptr() % 16 == 0 for pair in ins for t in pair) and mask.data_ptr() % 4 == 0
    assert aligned == quads, "the case must reach the %s path" % ("four-pixel" if quads else "one-pixel")
    p.mask, p.entropy, p.count, p.ws = mask.data_ptr(), (H[0].data_ptr() if entropy else None), count.data_ptr(), ws.data_ptr()
    p.threshold, p.threshold_dev = (-7.0 if thr_dev else thr), (td.data_ptr() if thr_dev else None)      # the host value is ignored beside the device word
    p.T, p.N, p.C, p.P = T, N, C, P
    L.call("chap_teacher_uncertainty", p, _stream())
    torch.cuda.synchronize()
    nb = blocks_of(N, P, quads)
    untouched("mask", mask_g, mask_f)
    untouched("count", count_g)
    untouched("ws", ws_g, ws[1 + nb:])                                  # the rows behind the launch's blocks stay as they were
    assert int(ws[0]) == int(count) == int(ws[1:1 + nb].sum()) and bool((ws[1:1 + nb] >= 0).all())
    if entropy:
        untouched("entropy", H[1])
    for pair, src in zip(ins, x["t"]):
        for t, z in zip(pair, src):
            untouched("input", t[1], t[2])
            assert torch.equal(t[0].cpu(), z), "an input was written"
    return dict(mask=mask.clone(), count=count.clone(), H=H[0].clone() if entropy else None, ws=ws.clone(), nb=nb)


def launch_masked(x, mask, count, *, offset=0, mask_offset=0, want=(True, True), accumulate=False, gscale=1.0, gscale_dev=None, quads=None, prior_seed=5):
    """One call through the struct -> dict(loss, g [2] (None where dlogits was NULL), prior [2], ws, nb)."""
    N, C, P = x["N"], x["C"], x["P"]
    shape = x["s"][0].shape
    srcs = x["s"] + x["t"][0]
    ins = [guarded(shape, fill=t) for t in srcs]
    ins[0] = guarded(shape, fill=srcs[0], offset=offset)
    m = guarded(mask.shape, torch.uint8, fill=mask, offset=mask_offset)
    cnt = torch.tensor([count], dtype=torch.int64, device=DEV)
    gen = torch.Generator().manual_seed(prior_seed)
    prior = [0.01 * torch.randn(shape, generator=gen) if accumulate else None for _ in range(2)]
    outs = [guarded(shape, fill=prior[h]) if want[h] else None for h in range(2)]
    loss, loss_g, _ = guarded((1,))
    ws, ws_g, _ = guarded((1 + L.LOSS_SLOTS, 2))
    gd = None if gscale_dev is None else torch.tensor([gscale_dev], dtype=torch.float32, device=DEV)
    p = L.TeacherConsistencyMaskedParams()
    for h in range(2):
        p.logits[h], p.teacher[h] = ins[h][0].data_ptr(), ins[2 + h][0].data_ptr()
        p.dlogits[h] = outs[h][0].data_ptr() if want[h] else None
    aligned = P % 4 == 0 and all(t[0].data_ptr() % 16 == 0 for t in ins + [o for o in outs if o is not None]) and m[0].data_ptr() % 4 == 0
    assert aligned == quads, "the case must reach the %s path" % ("four-pixel" if quads else "one-pixel")
    p.mask, p.count = m[0].data_ptr(), cnt.data_ptr()
    p.loss, p.ws, p.gscale, p.gscale_dev, p.accumulate = loss.data_ptr(), ws.data_ptr(), gscale, (None if gd is None else gd.data_ptr()), int(accumulate)
    p.N, p.C, p.P = N, C, P
    L.call("chap_teacher_consistency_masked", p, _stream())
    torch.cuda.synchronize()
    nb = blocks_of(N, P, quads)
    untouched("loss", loss_g)
    untouched("ws", ws_g, ws[1 + nb:])
    assert bool(torch.isfinite(ws[:1 + nb]).all()), "a used workspace row was left unwritten"
    untouched("mask", m[1], m[2])
    assert torch.equal(m[0].cpu(), mask) and int(cnt) == count
    for t, src in zip(ins, srcs):
        untouched("input", t[1], t[2])
        assert torch.equal(t[0].cpu(), src), "an input was written"
    for o in outs:
        if o is not None:
            untouched("dlogits", o[1])
    return dict(loss=loss.clone(), g=[None if o is None else o[0].clone() for o in outs], prior=prior, ws=ws.clone(), nb=nb)


class Worst:
    def __init__(self, case, C, T):
        self.case, self.C, self.T, self.w, self.und = case, C, T, {}, 0.0

    def chk(self, what, name, got, ref, bnd, dims="ncdhw"):
        r = kr.check("%s %s" % (self.case, name), got.cpu(), ref, bnd, dims)
        print("  %-56s worst err/bound %.3f" % ("%s %s" % (self.case, name), r))
        self.w[what] = max(self.w.get(what, 0.0), r)

    def masked(self, name, out, r, mask):
        self.chk("loss", name + " loss", out["loss"], r["loss"], r["loss_b"], "i")
        off = (mask == 0).unsqueeze(1)
        for h in range(2):
            if out["g"][h] is not None:
                self.chk("grad", "%s g%d" % (name, h), out["g"][h], r["g"][h], r["g_b"][h])
                # masked-out elements: the prior's bits, or +0
                want = torch.zeros_like(out["g"][h]).cpu() if out["prior"][h] is None else out["prior"][h]
                sel = off.expand_as(want)
                assert torch.equal(bits(out["g"][h].cpu())[sel], bits(want)[sel]), "%s g%d: a masked-out element changed" % (name, h)

    def log(self):
        print(json.dumps({"case": self.case, "C": self.C, "T": self.T, "undecided_share": round(self.und, 6),
                          "worst_ratio": {k: round(v, 4) for k, v in self.w.items()}}))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def cases():
    out = []
    for C in ur.CLASSES:
        for T in ur.PASSES:
            out.append(("c%d_t%d_scalar" % (C, T), C, T, ur.SCALAR, 0, 0))
            out.append(("c%d_t%d_quads" % (C, T), C, T, ur.QUADS, 0, 0))
    for C in (2, 5, 8):
        out.append(("c%d_t2_float_misaligned" % C, C, 2, ur.QUADS, 1, 0))
        out.append(("c%d_t2_mask_misaligned" % C, C, 2, ur.QUADS, 0, 1))
    for C in ur.TWO_TRIPS_CLASSES:
        out.append(("c%d_t2_two_trips" % C, C, 2, ur.TWO_TRIPS, 0, 0))
    return out


@pytest.mark.parametrize("name,C,T,shape,offset,mask_offset", cases(), ids=[c[0] for c in cases()])
def test_uncertainty_and_masked_term_per_element(name, C, T, shape, offset, mask_offset):
    x = case_inputs(C, shape, T)
    N, P = x["N"], x["P"]
    quads = P % 4 == 0 and offset == 0 and mask_offset == 0
    big = shape == ur.TWO_TRIPS
    kw = dict(offset=offset, mask_offset=mask_offset, quads=quads)
    W = Worst(name, C, T)
    if big:
        assert N * P // 4 > L.LOSS_SLOTS * 256              # the second trip
    # ---- the uncertainty kernel at both thresholds: entropy, the mask outside the band, the count
    refs = {}
    for frac in ur.FRACTIONS:
        thr = ur.threshold(frac, C)
        r = refs[frac] = ur.uncertainty_ref(x["t"], thr)
        a = launch_unc(x, thr, **kw)
        assert a["nb"] == blocks_of(N, P, quads) and a["nb"] >= 2 and (a["nb"] == L.LOSS_SLOTS) == big
        W.chk("entropy", "H at %.2f ln C" % frac, a["H"], r["H"], r["H_b"], "nhw")
        W.und = max(W.und, ur.check_mask("%s mask at %.2f ln C" % (name, frac), a["mask"], a["count"], r))
        assert 0 < int(a["count"]) < N * P
        # the device threshold word, no entropy output, a second launch: identical bits
        b = launch_unc(x, thr, entropy=False, thr_dev=True, **kw)
        assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["count"], b["count"]) and torch.equal(a["ws"][:1 + a["nb"]], b["ws"][:1 + b["nb"]])
    never = launch_unc(x, -1.0, **kw)
    assert int(never["count"]) == 0 and not bool(never["mask"].any())
    # ---- the masked term on the restatement's own mask (0.9 ln C)
    mref = refs[0.9]["mask"].to(torch.uint8)
    cnt = int(mref.sum())
    a = launch_masked(x, mref, cnt, **kw)
    r = ur.masked_ref(x["s"], x["t"][0], mref, cnt)
    W.masked("write", a, r, mref)
    b = launch_masked(x, mref, cnt, **kw)
    assert torch.equal(bits(a["loss"]), bits(b["loss"])) and all(torch.equal(bits(u), bits(v)) for u, v in zip(a["g"], b["g"]))
    assert torch.equal(bits(a["ws"][:1 + a["nb"]]), bits(b["ws"][:1 + b["nb"]]))
    if not big:
        c = launch_masked(x, mref, cnt, accumulate=True, gscale=0.3, gscale_dev=0.37, **kw)
        rc = ur.masked_ref(x["s"], x["t"][0], mref, cnt, gscale=0.3, gscale_dev=_f32(0.37), prior=c["prior"])
        W.masked("accumulate+gscale_dev", c, rc, mref)
        assert torch.equal(bits(c["loss"]), bits(a["loss"]))
        for want in ((False, True), (True, False)):
            d = launch_masked(x, mref, cnt, want=want, **kw)
            assert torch.equal(bits(d["loss"]), bits(a["loss"]))
            for h in range(2):
                assert (d["g"][h] is None) == (not want[h])
                if want[h]:
                    assert torch.equal(bits(d["g"][h]), bits(a["g"][h]))
        # count = 0: loss 0, gradient +0 (write) or the prior (accumulate); no NaN
        zero = torch.zeros_like(mref)
        for acc in (False, True):
            e = launch_masked(x, zero, 0, accumulate=acc, **kw)
            assert float(e["loss"]) == 0.0 and bits(e["loss"]).item() == 0
            for h in range(2):
                want = torch.zeros_like(e["g"][h]).cpu() if not acc else e["prior"][h]
                assert torch.equal(bits(e["g"][h].cpu()), bits(want))
        # an all-ones mask with count = N P is chap_teacher_consistency, within the sum of the two bounds
        ones = torch.ones_like(mref)
        f = launch_masked(x, ones, N * P, **kw)
        ro, rp = ur.masked_ref(x["s"], x["t"][0], ones, N * P), tr.teacher_ref(x["s"], x["t"][0])
        s, t = [v.to(DEV) for v in x["s"]], [v.to(DEV) for v in x["t"][0]]
        d = [torch.empty_like(v) for v in s]
        loss = torch.empty(1, device=DEV)
        ops.teacher_consistency(s, t, loss, d)
        torch.cuda.synchronize()
        W.chk("plain", "all-ones loss against chap_teacher_consistency", f["loss"], loss.cpu().double(), ro["loss_b"] + rp["loss_b"], "i")
        for h in range(2):
            W.chk("plain", "all-ones g%d against chap_teacher_consistency" % h, f["g"][h], d[h].cpu().double(), ro["g_b"][h] + rp["g_b"][h])
    W.log()


def test_refused_arguments_touch_nothing():
    shape = (4, 4, 16, 20)
    bufs = [guarded(shape) for _ in range(6)]
    mask, mask_g, _ = guarded((4, 16, 20), torch.uint8)
    count, count_g, _ = guarded((1,), torch.int64)
    ws, ws_g, _ = guarded((1 + L.LOSS_SLOTS,), torch.int64)
    loss, loss_g, _ = guarded((1,))
    wsf, wsf_g, _ = guarded((1 + L.LOSS_SLOTS, 2))

    def unc(**over):
        p = L.TeacherUncertaintyParams()
        for k in range(2):
            for h in range(2):
                p.teacher[k][h] = bufs[2 * k + h][0].data_ptr()
        p.mask, p.count, p.ws, p.threshold, p.T, p.N, p.C, p.P = mask.data_ptr(), count.data_ptr(), ws.data_ptr(), 0.5, 2, 4, 4, 320
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def msk(**over):
        p = L.TeacherConsistencyMaskedParams()
        for h in range(2):
            p.logits[h], p.teacher[h], p.dlogits[h] = bufs[h][0].data_ptr(), bufs[2 + h][0].data_ptr(), bufs[4 + h][0].data_ptr()
        p.mask, p.count, p.loss, p.ws, p.gscale, p.N, p.C, p.P = mask.data_ptr(), count.data_ptr(), loss.data_ptr(), wsf.data_ptr(), 1.0, 4, 4, 320
        for k, v in over.items():
            setattr(p, k, v)
        return p
    for entry, p, match in (("chap_teacher_uncertainty", unc(C=9), r"C=9 \(2\.\.8 built\)"), ("chap_teacher_uncertainty", unc(T=0), r"T=0 \(1\.\.8 built\)"),
                            ("chap_teacher_uncertainty", unc(T=3), "null teacher logits in pass 2 of T=3"), ("chap_teacher_uncertainty", unc(N=0), "N=0, P=320"),
                            ("chap_teacher_consistency_masked", msk(C=1), r"C=1 \(2\.\.8 built\)"), ("chap_teacher_consistency_masked", msk(count=None), "null"),
                            ("chap_teacher_consistency_masked", msk(N=1 << 16, P=1 << 16), "32-bit pixel index")):
        with pytest.raises(L.ChapError, match=match):
            L.call(entry, p, _stream())
    torch.cuda.synchronize()
    untouched("everything", mask, mask_g, count, count_g, ws, ws_g, loss, loss_g, wsf, wsf_g, *[b[0] for b in bufs], *[b[1] for b in bufs])


def test_ops_wrappers_are_the_struct_calls():
    C, T = 4, 3
    x = case_inputs(C, ur.QUADS, T)
    thr = ur.threshold(0.9, C)
    a = launch_unc(x, thr, quads=True)
    passes = [[z.to(DEV) for z in pair] for pair in x["t"]]
    mask, count, H = ops.teacher_uncertainty(passes, threshold=thr, want_entropy=True)
    mask2, count2 = ops.teacher_uncertainty(passes, threshold=-3.0, threshold_dev=torch.tensor([thr], device=DEV))
    torch.cuda.synchronize()
    assert mask.dtype == torch.uint8 and mask.shape == (4, 16, 20) and count.dtype == torch.int64 and count.shape == (1,)
    assert torch.equal(mask, a["mask"]) and torch.equal(count, a["count"]) and torch.equal(bits(H), bits(a["H"]))
    assert torch.equal(mask2, mask) and torch.equal(count2, count)
    b = launch_masked(x, mask.cpu(), int(count), quads=True, accumulate=True, gscale=0.3, gscale_dev=0.37)
    s = [v.to(DEV) for v in x["s"]]
    d = [v.to(DEV) for v in b["prior"]]
    loss = torch.full((1,), float("nan"), device=DEV)
    ops.teacher_consistency_masked(s, passes[0], mask, count, loss, d, gscale=0.3, gscale_dev=torch.tensor([0.37], device=DEV), accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(loss), bits(b["loss"])) and all(torch.equal(bits(u), bits(v)) for u, v in zip(d, b["g"]))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.teacher_uncertainty([passes[0], [passes[1][0], passes[1][1][:, :3]]])
    with pytest.raises(ValueError, match="need 1..8"):
        ops.teacher_uncertainty([])
    with pytest.raises(ValueError, match="mask must be contiguous uint8"):
        ops.teacher_consistency_masked(s, passes[0], mask[:, :8], count, loss)
    with pytest.raises(ValueError, match="count must be one int64"):
        ops.teacher_consistency_masked(s, passes[0], mask, count.float(), loss)
    with pytest.raises(ValueError, match="ws must hold"):
        ops.teacher_uncertainty(passes, ws=torch.empty(8, dtype=torch.int64, device=DEV))
