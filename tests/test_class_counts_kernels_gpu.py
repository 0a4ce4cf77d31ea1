"""chap_mix_loss_fwd / _bwd, chap_pseudo_block and chap_kl_fwd_bwd (kl and dice) at the class counts 3, 5, 6, 7, 8, per element against the fp64
restatements and bounds of tests/kernel_ref.py (exactly, where the result is a label), with the softmax chain term of
tests/class_count_cases.py.  Shapes: 4 x C x 17 x 19 (P % 4 = 3: the scalar KL path, two blocks, a ragged last wave), 4 x C x 16 x 20 on
16-byte-aligned tensors (the four-pixel KL path) and, at C = 3 and 8, 3 x C x 420 x 420 (more than 2048 * 256 pixels: a second grid-stride
trip in every kernel).  The entry points are called through their parameter structs on buffers with NaN / sentinel guards behind every
output and behind the used rows of the workspaces.  Run with -s for one line per check (worst err / bound) and one JSON line per case
(profiles/class_counts_kernels.jsonl holds those lines)."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from tests import class_count_cases as cc
from tests import kernel_ref as kr

DEV = torch.device("cuda", 0)
GUARD = 64
SENTINEL = -7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(n, dtype=torch.float32, fill=None):
    """(view of n elements, guard of GUARD elements right behind it); both NaN (floats) / SENTINEL (integers) unless `fill` is given for the view."""
    blank = float("nan") if dtype.is_floating_point else SENTINEL
    buf = torch.full((n + GUARD,), blank, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:n] = fill.reshape(-1).to(DEV)
    return buf[:n], buf[n:]


def untouched(name, g):
    ok = torch.isnan(g).all() if g.dtype.is_floating_point else (g == SENTINEL).all()
    assert bool(ok), "%s: the guard behind it was written" % name


class Worst:
    """the worst err / bound per kernel of one case; printed at the end."""

    def __init__(self, case, C):
        self.case, self.C, self.w = case, C, {}

    def chk(self, kernel, name, got, ref, bnd, dims="ncdhw"):
        r = kr.check("%s %s" % (self.case, name), got.cpu(), ref, bnd, dims)
        print("  %-52s worst err/bound %.3f" % ("%s %s" % (self.case, name), r))
        self.w[kernel] = max(self.w.get(kernel, 0.0), r)

    def log(self):
        rec = {"case": self.case, "C": self.C, "ew_u32": round(kr.EW / kr.U32), "worst_ratio": {k: round(v, 4) for k, v in self.w.items()}}
        print(json.dumps(rec))


def _blocks(total, cap):
    return min((total + 255) // 256, cap)


def run_mix(W, tag, c, *, mask=True, tb=True, w=(0.5, 1.0), k=(0.0, 0.0), gscale=1.0, gscale_dev=None, accumulate=False):
    C, lg = c["C"], c["l1"]
    N, P = lg.shape[0], lg[0, 0].numel()
    NA = 2 + 3 * C
    nb = _blocks(N * P, L.LOSS_SLOTS)
    ld, tad = lg.to(DEV), c["ta"].to(DEV)
    tbd = c["tb"].to(DEV) if tb else None
    md = c["mask"].to(DEV) if mask else None
    acc, acc_g = guarded((1 + nb) * 2 * NA)                 # the rows this launch uses; rows nb + 1 .. of a full workspace are the guard
    loss, loss_g = guarded(3)
    prior = torch.randn(lg.shape, generator=torch.Generator().manual_seed(5)) * 0.01 if accumulate else None
    dl, dl_g = guarded(lg.numel(), fill=prior)
    gd = None if gscale_dev is None else torch.tensor([gscale_dev], dtype=torch.float32, device=DEV)
    p = L.MixLossParams()
    p.logits, p.target_a, p.target_b, p.mask = ld.data_ptr(), tad.data_ptr(), (tbd.data_ptr() if tb else None), (md.data_ptr() if mask else None)
    p.w_a, p.w_b, p.acc, p.loss, p.dlogits = w[0], w[1], acc.data_ptr(), loss.data_ptr(), dl.data_ptr()
    p.gscale, p.accumulate, p.gscale_dev = gscale, int(accumulate), (None if gd is None else gd.data_ptr())
    p.N, p.C, p.P, p.smooth, p.k_dice, p.k_ce = N, C, P, 1e-10, k[0], k[1]
    L.call("chap_mix_loss_fwd", p, _stream())
    L.call("chap_mix_loss_bwd", p, _stream())
    torch.cuda.synchronize()
    r = kr.mix_loss_ref(lg, c["ta"], c["tb"] if tb else None, c["mask"] if mask else None, w[0], w[1], k_dice=k[0], k_ce=k[1], gscale=gscale,
                        gscale_dev=None if gscale_dev is None else float(torch.tensor(gscale_dev, dtype=torch.float32)), prior=prior)
    assert bool(torch.isfinite(acc).all()), tag + ": a used workspace row was left unwritten"
    W.chk("mix_loss_fwd", tag + " acc", acc[:2 * NA].view(2, NA), r["acc"], r["acc_b"], "ka")
    W.chk("mix_loss_fwd", tag + " loss", loss, r["loss"], r["loss_b"], "k")
    W.chk("mix_loss_bwd", tag + " dlogits", dl.view(lg.shape), r["dlogits"], r["dlogits_b"])
    for name, g in (("acc", acc_g), ("loss", loss_g), ("dlogits", dl_g)):
        untouched(tag + " " + name, g)


def run_pseudo(W, tag, c, want_soft=True):
    C, l1, l2 = c["C"], c["l1"], c["l2"]
    N, P = l1.shape[0], l1[0, 0].numel()
    r = kr.pseudo_ref(l1, l2)
    share = float(r["near"].double().mean())
    print("  %-52s near-tie share %.2e (cap %.0e)" % (tag, share, kr.NEAR_TIE_CAP))
    assert share <= kr.NEAR_TIE_CAP
    a, b = l1.to(DEV), l2.to(DEV)
    (s1, s1g), (s2, s2g) = guarded(l1.numel()), guarded(l1.numel())
    (a1, a1g), (a2, a2g) = guarded(N * P, torch.int64), guarded(N * P, torch.int64)
    kn, kng = guarded(N * P)
    p = L.PseudoParams()
    p.logits1, p.logits2 = a.data_ptr(), b.data_ptr()
    if want_soft:
        p.soft1, p.soft2 = s1.data_ptr(), s2.data_ptr()
    p.arg1, p.arg2, p.knowledge = a1.data_ptr(), a2.data_ptr(), kn.data_ptr()
    p.N, p.C, p.P = N, C, P
    L.call("chap_pseudo_block", p, _stream())
    torch.cuda.synchronize()
    ok = ~r["near"]
    if want_soft:
        W.chk("pseudo_block", tag + " soft1", s1.view(l1.shape), r["soft1"], r["soft1_b"])
        W.chk("pseudo_block", tag + " soft2", s2.view(l1.shape), r["soft2"], r["soft2_b"])
    else:
        assert bool(torch.isnan(s1).all()) and bool(torch.isnan(s2).all())
    for name, got in (("arg1", a1), ("arg2", a2)):          # labels: bit for bit wherever fp64 decides the maximum (planted exact ties included)
        got = got.cpu().view(r[name].shape)
        bad = (got != r[name]) & ok
        assert not bool(bad.any()), "%s %s: %d labels differ" % (tag, name, int(bad.sum()))
        assert int(got.min()) >= 0 and int(got.max()) < C
    W.chk("pseudo_block", tag + " knowledge", torch.where(ok, kn.cpu().view(ok.shape).double(), r["knowledge"]), r["knowledge"], r["knowledge_b"], "ndhw")
    for name, g in (("soft1", s1g), ("soft2", s2g), ("arg1", a1g), ("arg2", a2g), ("knowledge", kng)):
        untouched(tag + " " + name, g)
    return a1, a2, kn


def run_dist(W, tag, c, mode, *, quads, gscale=0.7, gscale_dev=None):
    C = c["C"]
    lg, tg = (c["l1"], c["l2"]), (c["t1"], c["t2"])
    N, P = lg[0].shape[0], lg[0][0, 0].numel()
    RL = 2 * (3 * C + 1)
    nb = _blocks(N * P, L.LOSS_SLOTS)
    prior = 0.25
    loss, loss_g = guarded(1, fill=torch.tensor([prior]))
    ws, ws_g = guarded((1 + nb) * RL)
    ld, td = [t.to(DEV) for t in lg], [t.to(DEV) for t in tg]
    outs = [guarded(lg[0].numel()) for _ in range(2)]
    gd = None if gscale_dev is None else torch.tensor([gscale_dev], dtype=torch.float32, device=DEV)
    p = L.KlParams()
    for h in range(2):
        p.logits[h], p.target[h], p.dlogits[h] = ld[h].data_ptr(), td[h].data_ptr(), outs[h][0].data_ptr()
    aligned = all(t.data_ptr() % 16 == 0 for t in ld + td + [o[0] for o in outs]) and P % 4 == 0
    assert aligned == quads, (tag, "the case must reach the %s path" % ("four-pixel" if quads else "scalar"))
    p.loss, p.gscale, p.gscale_dev = loss.data_ptr(), gscale, (None if gd is None else gd.data_ptr())
    p.N, p.C, p.P, p.mode, p.ws = N, C, P, {"kl": 0, "dice": 1}[mode], ws.data_ptr()
    L.call("chap_kl_fwd_bwd", p, _stream())
    torch.cuda.synchronize()
    r = kr.kl_ref(lg, tg, mode, gscale=gscale, gscale_dev=None if gscale_dev is None else float(torch.tensor(gscale_dev, dtype=torch.float32)), prior=prior)
    kern = "kl_fwd_bwd(%s)" % mode
    W.chk(kern, "%s %s loss" % (tag, mode), loss, r["loss"], r["loss_b"], "k")
    for h in range(2):
        W.chk(kern, "%s %s g%d" % (tag, mode, h), outs[h][0].view(lg[0].shape), r["g"][h], r["g_b"][h])
        untouched("%s %s g%d" % (tag, mode, h), outs[h][1])
    used = ws.view(1 + nb, RL)
    assert bool(torch.isfinite(used[:, 0]).all()) and (mode == "kl" or bool(torch.isfinite(used).all())), tag + ": a used workspace row was left unwritten"
    untouched("%s %s loss" % (tag, mode), loss_g), untouched("%s %s ws" % (tag, mode), ws_g)


@pytest.mark.parametrize("name,C,shape", cc.cases(), ids=[c[0] for c in cc.cases()])
def test_loss_kernels_at_the_new_class_counts(name, C, shape, monkeypatch):
    cc.chain_term(monkeypatch, C)
    c = cc.inputs(C, shape)
    W = Worst(name, C)
    quads = shape == cc.QUADS
    big = shape == cc.TWO_TRIPS
    assert int((c["ta"] == C).sum()) > 0 and int((c["ta"] == 255).sum()) > 0
    run_mix(W, "mask+tb", c)
    if not big:                                             # the options, at the small shapes
        run_mix(W, "no mask, no target_b, fp_loss (0,1)", c, mask=False, tb=False, w=(1.0, 0.0), k=(0.0, 1.0), gscale_dev=0.37)
        run_mix(W, "no mask", c, mask=False, w=(1.0, 0.5))
        run_mix(W, "accumulate+gscale_dev", c, accumulate=True, gscale=0.3, gscale_dev=0.37, k=(0.3, 1.7), w=(0.7, 0.3))
    a1, a2, kn = run_pseudo(W, "pseudo", c)
    if not big:
        b1, b2, kn2 = run_pseudo(W, "pseudo no soft", c, want_soft=False)
        assert torch.equal(a1, b1) and torch.equal(a2, b2) and torch.equal(kn, kn2)
    run_dist(W, "dist", c, "kl", quads=quads or big)
    run_dist(W, "dist", c, "dice", quads=quads or big)
    if not big:
        run_dist(W, "dist gscale_dev", c, "kl", quads=quads, gscale=2.0, gscale_dev=0.37)
        run_dist(W, "dist gscale_dev", c, "dice", quads=quads, gscale=2.0, gscale_dev=0.37)
    W.log()


@pytest.mark.parametrize("C", [5, 8])
def test_scalar_and_four_pixel_kl_paths_agree_bit_for_bit(C):
    """the same pixels through both paths of kl_kernel (aligned, and one float into its buffer): the per-pixel arithmetic is the same code, so
    the gradients are bit-identical; the loss differs only by the order of the per-thread sums and is covered by the bound above."""
    c = cc.inputs(C, cc.QUADS)
    N, P = c["l1"].shape[0], c["l1"][0, 0].numel()
    res = []
    for off in (0, 1):
        buf = torch.empty(c["l1"].numel() + 1, device=DEV)
        l1 = buf[off:off + c["l1"].numel()].view(c["l1"].shape)
        l1.copy_(c["l1"])
        assert (l1.data_ptr() % 16 == 0) == (off == 0)
        l2, t1, t2 = c["l2"].to(DEV), c["t1"].to(DEV), c["t2"].to(DEV)
        g = [torch.full(c["l1"].shape, float("nan"), device=DEV) for _ in range(2)]
        p = L.KlParams()
        for h, (lg, t) in enumerate(((l1, t1), (l2, t2))):
            p.logits[h], p.target[h], p.dlogits[h] = lg.data_ptr(), t.data_ptr(), g[h].data_ptr()
        p.gscale, p.N, p.C, p.P, p.mode = 0.7, N, C, P, 0
        L.call("chap_kl_fwd_bwd", p, _stream())
        torch.cuda.synchronize()
        res.append(g)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
