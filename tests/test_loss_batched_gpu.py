"""chap_mix_loss_multi_fwd / _bwd (up to four mix_loss terms in one launch per kernel) against the single-term entries, bit for bit:
loss[3], row 0 of the accumulator workspace and dlogits.  Each term keeps the block count, the grid-stride step and the partial-row
index of its own single-term launch, so the comparison is torch.equal, not a tolerance.  Shapes: a ragged last block (17 x 19), terms of
different N (blocks past a term's count leave), N * P > 512 * 256 (a second trip of the accumulate kernel, every partial row in use) and
N * P > 2048 * 256 (a second trip of the backward kernel); NULL mask / target_b, accumulate onto a non-zero buffer, a device-side gradient
scale and (k_dice, k_ce) weights vary over the terms.  One case checks the multi-term path per element against the fp64 restatement with
the bounds of the single-term tests (tests/kernel_ref.py).  Run with -s for one line per check."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import ops
from tests import kernel_ref as kr

DEV = torch.device("cuda", 0)
NS = (2, 3, 2, 3)


def make_terms(C, sp, ns, seed=0):
    """CPU description of len(ns) independent terms: term 1 has no mask, term 2 no target_b, term 0 accumulates onto a non-zero
    buffer, the last term carries a device-side scale, term 3 its own (k_dice, k_ce)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * len(ns) + seed + sp[0])
    weights = ((0.5, 1.0), (1.0, 0.5), (0.0, 1.0), (0.7, 0.3))
    terms = []
    for t, n in enumerate(ns):
        d = dict(logits=torch.randn(n, C, *sp, generator=g) * 2, target_a=torch.randint(0, C, (n, *sp), generator=g),
                 target_b=None if t == 2 else torch.randint(0, C, (n, *sp), generator=g),
                 mask=None if t == 1 else (torch.rand(n, *sp, generator=g) > 0.4).long(),
                 w_a=weights[t][0], w_b=weights[t][1], gscale=(1.0, 0.25, 1.0, 2.0)[t], accumulate=(t == 0),
                 gscale_dev=0.449 if t == len(ns) - 1 else None, k=(0.3, 1.7) if t == 3 else (0.0, 0.0))
        d["prior"] = torch.randn(n, C, *sp, generator=g) * 0.01 if d["accumulate"] else None
        terms.append(d)
    return terms


def to_dev(d):
    f = lambda v: v.to(DEV) if isinstance(v, torch.Tensor) else v
    e = {k: f(v) for k, v in d.items()}
    e["gd"] = None if d["gscale_dev"] is None else torch.tensor([d["gscale_dev"]], dtype=torch.float32, device=DEV)
    return e


def fresh_dlogits(d):
    return d["prior"].clone() if d["accumulate"] else torch.full(d["logits"].shape, float("nan"), device=DEV)


def run_single(devs):
    res = []
    for d in devs:
        loss, acc = ops.mix_loss_fwd(d["logits"], d["target_a"], d["target_b"], d["mask"], d["w_a"], d["w_b"], k_dice=d["k"][0], k_ce=d["k"][1])
        dl = fresh_dlogits(d)
        ops.mix_loss_bwd(d["logits"], d["target_a"], d["target_b"], d["mask"], d["w_a"], d["w_b"], acc, dl, gscale=d["gscale"],
                         accumulate=d["accumulate"], k_dice=d["k"][0], k_ce=d["k"][1], gscale_dev=d["gd"])
        res.append((loss, acc, dl))
    return res


def run_multi(devs):
    base = [dict(logits=d["logits"], target_a=d["target_a"], target_b=d["target_b"], mask=d["mask"], w_a=d["w_a"], w_b=d["w_b"],
                 k_dice=d["k"][0], k_ce=d["k"][1]) for d in devs]
    fwd = ops.mix_loss_multi_fwd(base)
    dls = [fresh_dlogits(d) for d in devs]
    ops.mix_loss_multi_bwd([dict(b, acc=acc, dlogits=dl, gscale=d["gscale"], accumulate=d["accumulate"], gscale_dev=d["gd"])
                            for b, (_, acc), dl, d in zip(base, fwd, dls, devs)])
    return [(loss, acc, dl) for (loss, acc), dl in zip(fwd, dls)]


def compare(tag, C, terms):
    devs = [to_dev(d) for d in terms]
    want, got = run_single(devs), run_multi(devs)
    torch.cuda.synchronize()
    row0 = 2 * (2 + 3 * C)
    for t, ((l0, a0, d0), (l1, a1, d1)) in enumerate(zip(want, got)):
        assert bool(torch.isfinite(d0).all()), (tag, t)
        assert torch.equal(l0, l1), (tag, t, "loss", l0.tolist(), l1.tolist())
        assert torch.equal(a0[:row0], a1[:row0]), (tag, t, "acc row 0")
        bad = d0 != d1
        assert not bool(bad.any()), "%s term %d: %d of %d dlogits differ" % (tag, t, int(bad.sum()), bad.numel())
    print("  %-40s %d terms bitwise equal" % (tag, len(terms)))
    return devs, got


@pytest.mark.parametrize("nterms", [1, 3, 4])
@pytest.mark.parametrize("C", [4, 2])
def test_multi_term_equals_single_term_calls_ragged(C, nterms):
    compare("C=%d nterms=%d 17x19" % (C, nterms), C, make_terms(C, (17, 19), NS[:nterms]))


def test_second_trip_of_the_accumulate_kernel_and_unequal_block_counts():
    """N = 3, P = 210 x 210: 132 300 pixels > 512 * 256, every partial row in use and a second grid-stride trip for some threads; the
    other terms (N = 2, 1) have fewer blocks than the grid is wide."""
    compare("C=4 210x210 N=(3,2,1)", 4, make_terms(4, (210, 210), (3, 2, 1)))


def test_second_trip_of_the_backward_kernel():
    """N = 3, P = 420 x 420: 529 200 pixels > 2048 * 256."""
    compare("C=2 420x420 N=(3,1)", 2, make_terms(2, (420, 420), (3, 1)))


def test_multi_term_path_per_element_against_fp64():
    """The multi-term kernels themselves (not through the single-term ones) against kr.mix_loss_ref, with its bounds."""
    C = 4
    terms = make_terms(C, (17, 19), NS)
    got = run_multi([to_dev(d) for d in terms])
    torch.cuda.synchronize()
    NA = 2 + 3 * C
    for t, (d, (loss, acc, dl)) in enumerate(zip(terms, got)):
        r = kr.mix_loss_ref(d["logits"], d["target_a"], d["target_b"], d["mask"], d["w_a"], d["w_b"], k_dice=d["k"][0], k_ce=d["k"][1], gscale=d["gscale"],
                            gscale_dev=None if d["gscale_dev"] is None else float(torch.tensor(d["gscale_dev"], dtype=torch.float32)), prior=d["prior"])
        worst = [kr.check("term %d acc" % t, acc[:2 * NA].view(2, NA).cpu(), r["acc"], r["acc_b"], "ka"),
                 kr.check("term %d loss" % t, loss.cpu(), r["loss"], r["loss_b"], "k"),
                 kr.check("term %d dlogits" % t, dl.cpu(), r["dlogits"], r["dlogits_b"])]
        print("  term %d worst err/bound acc %.3f loss %.3f dlogits %.3f" % ((t,) + tuple(worst)))


def test_multi_term_argument_errors():
    from chap_amd import _lib
    devs = [to_dev(d) for d in make_terms(4, (17, 19), (2, 2))]
    base = [dict(logits=d["logits"], target_a=d["target_a"], target_b=d["target_b"], mask=d["mask"], w_a=1.0, w_b=0.5) for d in devs]
    other = dict(base[1], logits=torch.zeros(2, 4, 17, 18, device=DEV))
    with pytest.raises(_lib.ChapError, match="common"):
        ops.mix_loss_multi_fwd([base[0], other])
    with pytest.raises(ValueError):
        ops.mix_loss_multi_fwd(base * 3)
