"""Training with 2 to 8 classes, the part that needs no GPU: the argument checks of the loss entry points at the class counts csrc/loss.hip
now builds, the oracle's iteration at those counts, tests/kernel_ref.py's restatements of the loss kernels against fp64 autograd at C = 3
and C = 8 (an fp32 emulation of each kernel passes their check, three planted faults fail it), the near-tie share of every input of
tests/test_class_counts_kernels_gpu.py, and the range check of the two train() entries."""
import pytest
import torch
import torch.nn.functional as F

from chap_amd import _lib
from chap_amd.synthetic import synthetic_batch_3d
from oracle import init as oinit
from oracle import train_step as ots
from tests import class_count_cases as cc
from tests import kernel_ref as kr
from tests.iteration_parity import compare, inject_2d, inject_3d, run_oracle

NEW = cc.CLASSES


# ---- argument checks: nothing is launched -------------------------------------------------------------------------------------------
def _mix(C, N=1 << 16, P=1 << 16):
    p = _lib.MixLossParams()
    p.logits, p.target_a, p.acc, p.loss, p.dlogits = 256, 256, 256, 256, 256       # never dereferenced: every call below fails its checks
    p.N, p.C, p.P = N, C, P
    return p


def _pseudo(C, N=1 << 16, P=1 << 16):
    p = _lib.PseudoParams()
    p.logits1, p.logits2 = 256, 256
    p.N, p.C, p.P = N, C, P
    return p


def _kl(C, N=1 << 16, P=1 << 16, ws=256):
    p = _lib.KlParams()
    for h in range(2):
        p.logits[h], p.target[h] = 256, 256
    p.N, p.C, p.P, p.mode, p.ws = N, C, P, 0, ws
    return p


ENTRIES = (("chap_mix_loss_fwd", _mix), ("chap_mix_loss_bwd", _mix), ("chap_pseudo_block", _pseudo), ("chap_kl_fwd_bwd", _kl))


@pytest.mark.parametrize("C", NEW)
def test_new_class_counts_pass_the_class_check(C):
    """the checks run null, then C, then the 32-bit pixel index: a built C with 2^32 pixels is refused for its size, not for its C."""
    for entry, make in ENTRIES:
        with pytest.raises(_lib.ChapError, match="32-bit"):
            _lib.call(entry, make(C), 0)
    with pytest.raises(_lib.ChapError, match="ws is required"):                     # kl: mode and ws are checked in front of the pixel index
        p = _kl(C, ws=None)
        p.loss = 256
        _lib.call("chap_kl_fwd_bwd", p, 0)


@pytest.mark.parametrize("C", [1, 9, 0, 16])
def test_class_counts_outside_2_to_8_are_refused_by_name(C):
    for entry, make in ENTRIES:
        with pytest.raises(_lib.ChapError, match=r"C=%d \(" % C):
            _lib.call(entry, make(C, N=2, P=323), 0)


def test_null_comes_before_the_class_check():
    for entry, make in ENTRIES:
        p = make(9)
        if isinstance(p, _lib.KlParams):
            p.logits[0] = None
        elif isinstance(p, _lib.PseudoParams):
            p.logits1 = None
        else:
            p.logits = None
        with pytest.raises(_lib.ChapError, match="null argument"):
            _lib.call(entry, p, 0)


@pytest.mark.parametrize("entry", ["chap_mix_loss_multi_fwd", "chap_mix_loss_multi_bwd"])
def test_multi_term_entries_keep_their_two_class_counts(entry):
    for C in (3, 5, 8):
        m = _lib.MixLossMultiParams()
        m.nterms = 1
        m.term[0] = _mix(C, N=2, P=323)
        with pytest.raises(_lib.ChapError, match=r"C=%d \(2 or 4 built\)" % C):
            _lib.call(entry, m, 0)


def test_train_entries_refuse_other_class_counts_up_front(tmp_path):
    from chap_amd import train_ours_2D, train_ours_3D
    for mod in (train_ours_2D, train_ours_3D):
        for nc in (1, 9, 16, 0):
            target = tmp_path / ("%s_%d" % (mod.__name__.rsplit(".", 1)[-1], nc))
            with pytest.raises(ValueError, match="2 to 8 classes"):
                mod.train(dict(num_classes=nc, max_iterations=1), str(target))
            assert not target.exists()                      # refused before anything is written or allocated


# ---- synthetic volumes ---------------------------------------------------------------------------------------------------------------
def test_synthetic_batch_3d_default_is_unchanged_and_classes_nest():
    v2, l2 = synthetic_batch_3d(1338, 2, 2, 16, 32, 16)
    va, la = synthetic_batch_3d(1338, 2, 2, 16, 32, 16, n_classes=2)
    assert torch.equal(v2, va) and torch.equal(l2, la) and set(l2.unique().tolist()) == {0, 1}
    assert int(l2.sum()) == 349                             # the foreground voxels of this batch before the argument existed
    # the definition of the two-class generator, restated: foreground = the main blob above one half.  The images do not depend on n_classes
    v3, l3 = synthetic_batch_3d(1338, 2, 2, 16, 32, 16, n_classes=3)
    assert torch.equal(v3, v2) and set(l3.unique().tolist()) == {0, 1, 2}
    assert bool(((l3 == 2) <= (l2 == 1)).all()) and bool(((l2 == 1) <= (l3 >= 1)).all())       # thresholds 5/12 < 1/2 < 7/12: nested regions
    assert ots.synthetic_batch_3d is synthetic_batch_3d


# ---- the oracle runs the iteration at the new counts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 5, 8])
def test_oracle_iteration_2d(C):
    B, lbs, H, W = 8, 4, 64, 64
    U = B - lbs
    args = dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=C)
    state = oinit.dual_decoder_2d_state(611, n_class=C)
    vol, lab = ots.synthetic_batch(1441, lbs, U, H, W, C)
    assert set(lab.unique().tolist()) == set(range(C))
    inj = inject_2d(U, lbs // 2 + U // 2, H, W, 1)
    o32 = run_oracle(state, vol, lab, (9, 4), 4500, args, inj, 2, torch.float32)
    o64 = run_oracle(state, vol, lab, (9, 4), 4500, args, inj, 2, torch.float64)
    assert o32["losses"].shape == (4, 3) and bool(torch.isfinite(o64["losses"]).all()) and float(o64["losses"].min()) > 0
    d = compare(o32, o64, state)
    print("oracle 2D C=%d: fp32 vs fp64 loss %.2e vat %.2e update %.2e" % (C, d["loss"], d["vat"], d["upd_rel_l2"]))
    assert d["loss"] < 2e-5                                 # rounding level (tests/iteration_parity.py's floor); measured 1.0e-7 .. 1.3e-7


def test_oracle_iteration_3d_three_classes():
    B, lbs, sp = 4, 2, (16, 32, 16)
    U = B - lbs
    args = dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=3)
    state = oinit.dual_decoder_3d_state(402, n_class=3)
    vol, lab = ots.synthetic_batch_3d(1338, lbs, U, *sp, n_classes=3)
    assert set(lab.unique().tolist()) == {0, 1, 2}
    inj = inject_3d(U, lbs // 2 + U // 2, sp, 1)
    o32 = run_oracle(state, vol, lab, (2, 5, 3), 4500, args, inj, 3, torch.float32)
    o64 = run_oracle(state, vol, lab, (2, 5, 3), 4500, args, inj, 3, torch.float64)
    d = compare(o32, o64, state)
    print("oracle 3D C=3: fp32 vs fp64 loss %.2e vat %.2e update %.2e" % (d["loss"], d["vat"], d["upd_rel_l2"]))
    # 5e-4: the absolute loss bound tests/test_iteration_conditioning_gpu.py holds the small 3D iteration to -- at 16 x 32 x 16 a handful of arg-max
    # pseudo labels differ between ANY two evaluations (here fp32 and fp64 of the same oracle: 2.7e-4), so the 2D rounding floor does not apply
    assert bool(torch.isfinite(o64["losses"]).all()) and float(o64["losses"].min()) > 0 and d["loss"] < 5e-4


# ---- the restatements at the new counts --------------------------------------------------------------------------------------------------
def close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def _in_range(c):
    """the case with its out-of-range labels folded back into [0, C): what the oracle's cross_entropy accepts."""
    C = c["C"]
    return dict(c, ta=c["ta"] % C, tb=c["tb"] % C)


def _autograd_mix(z, ta, tb, m, wa, wb, kd=0.5, kc=0.5, smooth=1e-10):
    """mix_loss in autograd form with one-hot targets by comparison: a label outside [0, C) is an all-zero one-hot (no Dice target, CE term
    lse - 0), as in the kernel."""
    C = z.shape[1]
    p = torch.softmax(z, 1)
    lse = torch.logsumexp(z, 1)
    red = [0] + list(range(2, z.dim()))
    parts = []
    for t, mk, w in ((ta, m, wa), (tb, 1.0 - m, wb)):
        oh = torch.stack([(t == c) for c in range(C)], 1).to(z.dtype)
        ce = ((lse - (oh * z).sum(1)) * mk).sum() / (mk.sum() + 1e-16)
        mk1 = mk.unsqueeze(1)
        I, Z, Y = (p * oh * mk1).sum(red), (p * p * mk1).sum(red), (oh * mk1).sum(red)
        dice = (1.0 - (2.0 * I + smooth) / (Z + Y + smooth)).sum() / C
        parts.append(w * (kd * dice + kc * ce))
    return parts[0], parts[1], parts[0] + parts[1]


@pytest.mark.parametrize("C", [3, 8])
def test_restatements_equal_fp64_autograd(C):
    c = cc.inputs(C, cc.SCALAR)
    m = c["mask"].double()
    # mix_loss with ignored labels (C and 255) against the autograd form, and with in-range labels against the oracle's mix_loss
    lo = c["l1"].double().requires_grad_(True)
    la, lb, tot = _autograd_mix(lo, c["ta"], c["tb"], m, 0.5, 1.0)
    (tot * 0.25).backward()
    r = kr.mix_loss_ref(c["l1"], c["ta"], c["tb"], c["mask"], 0.5, 1.0, gscale=0.25)
    assert close(r["loss"], torch.stack([la, lb, tot])) and close(r["dlogits"], lo.grad)
    assert int((c["ta"] == C).sum()) > 0 and int((c["ta"] == 255).sum()) > 0 and float(r["acc"][0, 1 + 2 * C:1 + 3 * C].sum()) < float(r["acc"][0, -1])
    ci = _in_range(c)
    lo = c["l1"].double().requires_grad_(True)
    li, lp, tot = ots.mix_loss(lo, ci["ta"], ci["tb"], m, l_weight=1.0, u_weight=0.5)
    tot.backward()
    r = kr.mix_loss_ref(c["l1"], ci["ta"], ci["tb"], c["mask"], 1.0, 0.5)
    assert close(r["loss"], torch.stack([li, lp, tot])) and close(r["dlogits"], lo.grad)
    # (k_dice, k_ce) = (0, 1), no mask, no target_b: the fp_loss branch's mean cross-entropy
    lo = c["l1"].double().requires_grad_(True)
    ce = F.cross_entropy(lo, ci["ta"])
    ce.backward()
    r = kr.mix_loss_ref(c["l1"], ci["ta"], None, None, 1.0, 0.0, k_dice=0.0, k_ce=1.0)
    assert close(r["loss"][2], ce) and close(r["dlogits"], lo.grad)
    # pseudo block
    pr = kr.pseudo_ref(c["l1"], c["l2"])
    s1, s2, a1, a2, kn = ots.pseudo_block(c["l1"].double(), c["l2"].double())
    assert close(pr["soft1"], s1) and close(pr["soft2"], s2) and close(pr["knowledge"], kn)
    assert torch.equal(pr["arg1"], a1) and torch.equal(pr["arg2"], a2)
    # the two distances
    for mode, fn in (("kl", ots.kl_two_heads), ("dice", ots.dice_two_heads)):
        la, lb = c["l1"].double().requires_grad_(True), c["l2"].double().requires_grad_(True)
        d = fn((la, lb), (c["t1"].double(), c["t2"].double()))
        (d * 0.75).backward()
        r = kr.kl_ref((c["l1"], c["l2"]), (c["t1"], c["t2"]), mode, gscale=0.75, prior=0.25)
        assert abs(float(r["loss"]) - 0.25 - float(d.detach())) < 1e-12
        tol = 1e-12 if mode == "dice" else 4 * kr.U32      # KL: gs/total (p - t) is the derivative for targets that sum to 1; these do to fp32 rounding
        assert (r["g"][0] - la.grad).abs().max() <= tol * la.grad.abs().max() and (r["g"][1] - lb.grad).abs().max() <= tol * lb.grad.abs().max()


# ---- an fp32 emulation of each kernel, and three planted faults ------------------------------------------------------------------------
def _emulate_mix(c, w=(0.5, 1.0), drop_last_class=False, div4=False):
    """chap_mix_loss_fwd / _bwd in fp32 torch arithmetic: one partial row per 256 pixels summed back to front, fp64 total of the rows.
    drop_last_class: the Dice sums of the loss and of the gradient stop at class C - 2.  div4: the Dice mean divides by 4, not by C."""
    lg, C = c["l1"], c["C"]
    N, P = lg.shape[0], lg[0, 0].numel()
    z = lg.reshape(N, C, P)
    p = torch.softmax(z, 1)
    lse = torch.logsumexp(z, 1)
    mk = [c["mask"].reshape(N, P).float(), 1.0 - c["mask"].reshape(N, P).float()]
    ts = [torch.stack([(t.reshape(N, P) == k) for k in range(C)], 1).float() for t in (c["ta"], c["tb"])]
    rows = []
    for k in range(2):
        cols = [(lse - (ts[k] * z).sum(1)) * mk[k]] + [p[:, i] * ts[k][:, i] * mk[k] for i in range(C)] + [p[:, i] * p[:, i] * mk[k] for i in range(C)] \
            + [ts[k][:, i] * mk[k] for i in range(C)] + [mk[k]]
        rows.append(torch.stack([v.reshape(-1) for v in cols], 1))
    per_px = torch.cat(rows, 1)
    pad = (-per_px.shape[0]) % 256
    blocks = F.pad(per_px, (0, 0, 0, pad)).reshape(-1, 256, per_px.shape[1]).flip(1).sum(1)
    acc = blocks.double().sum(0).float().reshape(2, -1)
    s, kd, kc = torch.tensor(1e-10), 0.5, 0.5
    div = 4 if div4 else C
    live = torch.ones(C)
    if drop_last_class:
        live[C - 1] = 0.0
    part, dz, dp = [], torch.zeros_like(p), torch.zeros_like(p)
    for k in range(2):
        a = acc[k]
        I, Z, Y = a[1:1 + C], a[1 + C:1 + 2 * C], a[1 + 2 * C:1 + 3 * C]
        den = Z + Y + s
        dice = ((1.0 - (2.0 * I + s) / den) * live).sum() / div * w[k]
        ce = w[k] * a[0] / (a[-1] + 1e-16)
        part.append(kd * dice + kc * ce)
        kce = w[k] * mk[k] / (a[-1] + 1e-16)
        dz = dz + kce.unsqueeze(1) * (p - ts[k])
        dp = dp + (w[k] / div) * mk[k].unsqueeze(1) * live.view(1, C, 1) * (-2.0 * ts[k] / den.view(1, C, 1) + ((2.0 * I + s) * 2.0 / (den * den)).view(1, C, 1) * p)
    dl = kc * dz + kd * p * (dp - (dp * p).sum(1, keepdim=True))
    return acc, torch.stack([part[0], part[1], part[0] + part[1]]), dl.reshape(lg.shape)


def _emulate_argmax(p, last_wins=False):
    if not last_wins:
        return p.argmax(1)
    return p.shape[1] - 1 - p.flip(1).argmax(1)


def fails(name, got, ref, bnd, dims="ncdhw"):
    try:
        kr.check(name, got, ref, bnd, dims)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("C", [3, 8])
def test_emulated_kernels_pass_and_three_planted_faults_fail(C, monkeypatch):
    cc.chain_term(monkeypatch, C)
    c = cc.inputs(C, cc.SCALAR)
    r = kr.mix_loss_ref(c["l1"], c["ta"], c["tb"], c["mask"], 0.5, 1.0)
    acc, loss, dl = _emulate_mix(c)
    kr.check("acc", acc, r["acc"], r["acc_b"], "ka"), kr.check("loss", loss, r["loss"], r["loss_b"], "k"), kr.check("dlogits", dl, r["dlogits"], r["dlogits_b"])
    pr = kr.pseudo_ref(c["l1"], c["l2"])
    s1, s2, a1, a2, kn = ots.pseudo_block(c["l1"], c["l2"])
    ok = ~pr["near"]
    kr.check("soft1", s1, pr["soft1"], pr["soft1_b"]), kr.check("soft2", s2, pr["soft2"], pr["soft2_b"])
    kr.check("knowledge", torch.where(ok, kn.double(), pr["knowledge"]), pr["knowledge"], pr["knowledge_b"], "ndhw")
    assert torch.equal(_emulate_argmax(s1)[ok], pr["arg1"][ok]) and torch.equal(_emulate_argmax(s2)[ok], pr["arg2"][ok])
    for mode, fn in (("kl", ots.kl_two_heads), ("dice", ots.dice_two_heads)):
        la, lb = c["l1"].clone().requires_grad_(True), c["l2"].clone().requires_grad_(True)
        d = fn((la, lb), (c["t1"], c["t2"]))
        (d * 0.7).backward()
        k_ = kr.kl_ref((c["l1"], c["l2"]), (c["t1"], c["t2"]), mode, gscale=0.7, prior=0.25)
        kr.check("dist loss", (d.detach() + 0.25).reshape(1), k_["loss"], k_["loss_b"], "k")
        kr.check("dist g0", la.grad, k_["g"][0], k_["g_b"][0]), kr.check("dist g1", lb.grad, k_["g"][1], k_["g_b"][1])
        if mode == "dice":                                  # fault 2 on the distance: the class mean taken over 4
            bad, gbad = (d.detach() * C / 4 + 0.25).reshape(1), la.grad * C / 4
            assert fails("dist loss /4", bad, k_["loss"], k_["loss_b"], "k") and fails("dist g0 /4", gbad, k_["g"][0], k_["g_b"][0])
    # fault 1: class C - 1 dropped from the Dice sum
    _, loss1, dl1 = _emulate_mix(c, drop_last_class=True)
    assert fails("fault 1 loss", loss1, r["loss"], r["loss_b"], "k") and fails("fault 1 dlogits", dl1, r["dlogits"], r["dlogits_b"])
    # fault 2: the division by 4 where C belongs
    _, loss2, dl2 = _emulate_mix(c, div4=True)
    assert fails("fault 2 loss", loss2, r["loss"], r["loss_b"], "k") and fails("fault 2 dlogits", dl2, r["dlogits"], r["dlogits_b"])
    # fault 3: the last maximum wins the arg-max -- wrong exactly on the planted ties, which the comparison keeps
    top = pr["soft1"].topk(2, dim=1).values
    assert int(((top[:, 0] == top[:, 1]) & ok).sum()) >= 20
    assert not torch.equal(_emulate_argmax(s1, last_wins=True)[ok], pr["arg1"][ok])
    assert not torch.equal(_emulate_argmax(s2, last_wins=True)[ok], pr["arg2"][ok])


def test_chain_term_counts_the_softmax_chain():
    """C + 4 roundings (argument, expf, C - 1 adds, reciprocal, product), never below kernel_ref's 8: unchanged up to C = 4."""
    assert [round(cc.ew(C) / kr.U32) for C in (2, 3, 4, 5, 6, 7, 8)] == [8, 8, 8, 9, 10, 11, 12] and kr.EW == 8 * kr.U32


# ---- near ties of every GPU input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,shape", cc.cases(), ids=[c[0] for c in cc.cases()])
def test_near_tie_share_of_the_gpu_inputs(name, C, shape, monkeypatch):
    cc.chain_term(monkeypatch, C)
    c = cc.inputs(C, shape)
    r = kr.pseudo_ref(c["l1"], c["l2"])
    share = float(r["near"].double().mean())
    print("near-tie share %s: %.2e (%d pixels)" % (name, share, int(r["near"].sum())))
    assert share <= kr.NEAR_TIE_CAP
    top = r["soft1"].topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) >= 20       # the planted exact ties are present and are compared
    if C >= 6:                                              # ... and some of them sit between classes 4 and 5
        assert int(((r["arg1"] == 4) & (top[:, 0] == top[:, 1])).sum()) >= 10
