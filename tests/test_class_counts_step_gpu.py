"""Networks, training steps and the public train() entries at class counts other than the two benchmarked ones (2D: 4, 3D: 2).

Networks against the oracle (fp32: eval logits within the project's 1e-4, training-mode gradients by the three-way criterion of
tests/test_net2d_gpu.py::test_dualdecoder_train_injected; bf16: the 2D heads and the 3D head route within the bf16 bounds of the existing
network tests).  One iteration three ways with the criterion, factors and floors of tests/iteration_parity.py; captured replay == eager bit
for bit; the dropout (fp_loss + GradSim) branch and AblationStep at C = 3; the captured C = 3 iteration free of unordered cross-stream
conflicts (with three classes pass B issues the four single-term loss calls instead of the batched launch); train() of both entries."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd.networks import DualDecoder, DualDecoder3d
from chap_amd.train import AblationStep, ChapStep
from oracle import init as oinit
from oracle import nets as onets
from oracle import train_step as ots
from tests.iteration_parity import (assert_as_close_to_fp64_as_the_fp32_oracle, compare, gm_over, inject_2d, inject_3d, run_oracle, to_dev)
from tests.test_net2d_gpu import cl_masks, cosine, relerr

DEV = "cuda"
SEEDS = 3


def make_net(dims, C):
    if dims == 3:
        return DualDecoder3d(n_channels=1, n_classes=C, normalization="batchnorm", has_dropout=True)
    return DualDecoder(1, C, {"decoder_type": "mcnet"})


# ---- networks ----------------------------------------------------------------------------------------------------------------------------
def oracle_net(dims, state, x, cots, dtype, train, drop):
    sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    for k, v in sd.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    fn = onets.dual_decoder_3d if dims == 3 else onets.dual_decoder_2d
    o = fn(sd, xr, train=train, drop=drop)
    sum((a * c.to(dtype)).sum() for a, c in zip(o, cots)).backward()
    return [a.detach() for a in o], xr.grad, {k: v.grad for k, v in sd.items() if v.requires_grad}


def hip_net(dims, C, state, x, cots, dtype, train, drop):
    m = make_net(dims, C).to(DEV)
    m.load_state_dict(state, strict=True)
    m.set_compute_dtype(dtype)
    m.train() if train else m.eval()
    xd = x.detach().clone().to(DEV).requires_grad_(True)
    kw = {}
    if drop is not None:
        kw["drop_masks"] = cl_masks(drop) if dims == 2 else {k: (v.float() * 2.0).to(DEV) for k, v in drop.items()}
    outs = m(xd, **kw)
    m.zero_grad()
    torch.autograd.backward(outs, [c.to(DEV) for c in cots])
    torch.cuda.synchronize()
    return outs, xd.grad, {k: p.grad for k, p in m.named_parameters()}


NET_CASES = [(2, 3, (2, 1, 64, 64)), (2, 8, (2, 1, 64, 64)), (3, 3, (1, 1, 16, 32, 16))]


def net_inputs(dims, C, shape, golden_dir):
    """State, input and cotangents of a network case.  2D: the input (2 x 1 x 64 x 64) and the state seed of tests/golden/dualdecoder2d_64.npz, the
    fixture the bounds of tests/test_net2d_gpu.py were set on, with heads of C classes; 3D: a uniform input of the case's shape."""
    g = torch.Generator().manual_seed(31 + C)
    if dims == 2:
        gold = np.load(os.path.join(golden_dir, "dualdecoder2d_64.npz"), allow_pickle=False)
        state, x = oinit.dual_decoder_2d_state(int(gold["state_seed"]), n_class=C), torch.from_numpy(gold["x"])
        assert tuple(x.shape) == shape
    else:
        state, x = oinit.dual_decoder_3d_state(811 + C, n_class=C), torch.rand(shape, generator=g)
    cots = [torch.randn((shape[0], C) + shape[2:], generator=g) for _ in range(2)]
    return state, x, cots
PICKS = {2: ["decoder1.out_conv.weight", "decoder2.out_conv.weight", "decoder1.out_conv.bias", "encoder.in_conv.conv_conv.0.weight",
             "encoder.down4.maxpool_conv.1.conv_conv.4.weight", "decoder2.up4.conv.conv_conv.4.weight"],
         3: ["decoder1.out_conv.weight", "decoder2.out_conv.weight", "decoder1.out_conv.bias", "encoder.block_one.conv.0.weight",
             "decoder1.block_nine.conv.0.weight", "decoder2.block_six_up.conv.0.weight"]}


@pytest.mark.parametrize("dims,C,shape", NET_CASES, ids=["2d_c3", "2d_c8", "3d_c3"])
def test_network_matches_the_oracle_fp32(golden_dir, dims, C, shape):
    state, x, cots = net_inputs(dims, C, shape, golden_dir)
    # eval: logits within 1e-4
    ref, _, _ = oracle_net(dims, state, x, cots, torch.float32, False, None)
    outs, _, _ = hip_net(dims, C, state, x, cots, torch.float32, False, None)
    for a, b in zip(outs, ref):
        assert a.shape == b.shape and relerr(a, b) < 1e-4, (relerr(a, b),)
    # train mode, injected dropout: the distance to fp64 against the fp32 oracle's own distance to fp64
    drop = oinit.drop_masks_3d(5, shape[0]) if dims == 3 else oinit.drop_masks_2d(5, shape[0], shape[2], shape[3])
    o32, dx32, g32 = oracle_net(dims, state, x, cots, torch.float32, True, drop)
    o64, dx64, g64 = oracle_net(dims, state, x, cots, torch.float64, True, drop)
    outs, dx, grads = hip_net(dims, C, state, x, cots, torch.float32, True, drop)
    for a, b, c in zip(outs, o32, o64):                    # training-mode BatchNorm over a few values per channel: logits by the same criterion, 1e-4 as the floor
        print("C=%d %dD train logits: HIP %.3g, fp32 oracle %.3g" % (C, dims, relerr(a, c), relerr(b, c)))
        assert relerr(a, c) < max(4 * relerr(b, c), 1e-4), (relerr(a, c), relerr(b, c))
    ref_err = relerr(dx32, dx64)
    print("C=%d %dD dx: HIP %.3g, fp32 oracle %.3g" % (C, dims, relerr(dx, dx64), ref_err))
    assert relerr(dx, dx64) < max(4 * ref_err, 2e-2)
    for n in PICKS[dims]:
        ref_e, e = relerr(g32[n], g64[n]), relerr(grads[n], g64[n])
        print("C=%d %dD %s: HIP %.3g, fp32 oracle %.3g" % (C, dims, n, e, ref_e))
        assert e < max(4 * ref_e, 2e-2), (n, e, ref_e)


@pytest.mark.parametrize("dims,C,shape,tol", [(2, 3, (2, 1, 64, 64), 4e-2), (2, 8, (2, 1, 64, 64), 4e-2),
                                              (3, 3, (1, 1, 16, 32, 16), 5e-2), (3, 8, (1, 1, 16, 32, 16), 5e-2)], ids=["2d_c3", "2d_c8", "3d_c3", "3d_c8"])
def test_network_heads_bf16(golden_dir, dims, C, shape, tol):
    """bf16 compute: the 2D 3 x 3 heads and the 3D 1 x 1 x 1 head route (Cout <= 8) at 3 and 8 output channels; eval logits within the bounds
    of tests/test_net2d_gpu.py::test_dualdecoder_eval (4e-2) and tests/test_net3d_gpu.py::test_dualdecoder3d_eval (5e-2), input gradient by direction."""
    state, x, cots = net_inputs(dims, C, shape, golden_dir)
    ref, dxr, _ = oracle_net(dims, state, x, cots, torch.float32, False, None)
    outs, dx, _ = hip_net(dims, C, state, x, cots, torch.bfloat16, False, None)
    for a, b in zip(outs, ref):
        print("C=%d %dD bf16 logits %.3g" % (C, dims, relerr(a, b)))
        assert a.shape == b.shape and relerr(a, b) < tol
    assert cosine(dx, dxr) > 0.9


# ---- one iteration -------------------------------------------------------------------------------------------------------------------------
def run_hip(state, vol, lab, box, it0, args, inj, dims, C, graph=False):
    """tests/iteration_parity.py::run_hip with a class-count argument."""
    m = make_net(dims, C).to(DEV).train()
    m.load_state_dict(state, strict=True)
    step = ChapStep(m, args)
    step.iter_num = it0
    vd, ld, injd = vol.to(DEV), lab.to(DEV), to_dev(inj, dims)
    if graph:
        step.capture(vd, ld, warmup=1, inject=injd)
        out = step.replay(vd, ld, box_yx=box)
    else:
        out = step.step(vd, ld, box_yx=box, inject=injd)
    torch.cuda.synchronize()
    losses = torch.stack([l.detach().double().cpu() for l in out["mix_losses"]])
    return dict(losses=losses, vat=out["vat_loss"].detach().double().cpu().reshape(1), after={k: v.detach().double().cpu() for k, v in m.state_dict().items()},
                mom=step.opt.mom.clone())


def three_way(name, dims, C, state, vol, lab, box, it0, args, inj):
    o32 = run_oracle(state, vol, lab, box, it0, args, inj, dims, torch.float32)
    o64 = run_oracle(state, vol, lab, box, it0, args, inj, dims, torch.float64)
    hip = run_hip(state, vol, lab, box, it0, args, inj, dims, C)
    res = {"case": name, "hip_o32": compare(hip, o32, state), "o32_o64": compare(o32, o64, state), "hip_o64": compare(hip, o64, state)}
    print(json.dumps(res))
    return res


def case_2d(C, s=0, **extra):
    B, lbs, H, W = 8, 4, 64, 64
    U = B - lbs
    args = dict(dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=C), **extra)
    state = oinit.dual_decoder_2d_state(611, n_class=C)
    vol, lab = ots.synthetic_batch(1441 + s, lbs, U, H, W, C)
    return state, vol, lab, (9 + s, 4 + 2 * s), args, inject_2d(U, lbs // 2 + U // 2, H, W, 1, seed=50 * s)


def case_3d(C, s=0):
    B, lbs, sp = 4, 2, (16, 32, 16)
    U = B - lbs
    args = dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=C)
    state = oinit.dual_decoder_3d_state(402, n_class=C)
    vol, lab = ots.synthetic_batch_3d(1338 + s, lbs, U, *sp, n_classes=C)
    return state, vol, lab, (2, 5 - s, 3), args, inject_3d(U, lbs // 2 + U // 2, sp, 1, seed=50 * s)


@pytest.mark.parametrize("C,losstype", [(3, "kl"), (3, "dice"), (8, "kl")])
def test_2d_iteration_is_as_close_to_fp64_as_the_fp32_oracle(C, losstype):
    runs = []
    for s in range(SEEDS):
        state, vol, lab, box, args, inj = case_2d(C, s, adv_losstype=losstype)
        runs.append(three_way("2d_64_c%d_%s_s%d" % (C, losstype, s), 2, C, state, vol, lab, box, 4500, args, inj))
        assert runs[-1]["hip_o32"]["loss"] < 2e-4           # the absolute bound of tests/test_iteration_conditioning_gpu.py in 2D
    assert_as_close_to_fp64_as_the_fp32_oracle(gm_over(runs))


def test_3d_iteration_three_classes_is_as_close_to_fp64_as_the_fp32_oracle():
    runs = []
    for s in range(SEEDS):
        state, vol, lab, box, args, inj = case_3d(3, s)
        runs.append(three_way("3d_16x32x16_c3_k1_s%d" % s, 3, 3, state, vol, lab, box, 4500, args, inj))
        assert runs[-1]["hip_o32"]["loss"] < 5e-4           # ... and in 3D
    assert_as_close_to_fp64_as_the_fp32_oracle(gm_over(runs))


def _same(a, b):
    assert torch.equal(a["losses"], b["losses"]) and torch.equal(a["vat"], b["vat"]) and torch.equal(a["mom"], b["mom"])
    assert [k for k in a["after"] if not torch.equal(a["after"][k], b["after"][k])] == []


@pytest.mark.parametrize("dims", [2, 3])
def test_three_class_replay_equals_eager_bit_for_bit(dims):
    state, vol, lab, box, args, inj = case_2d(3) if dims == 2 else case_3d(3)
    eager = run_hip(state, vol, lab, box, 4500, args, inj, dims, 3)
    again = run_hip(state, vol, lab, box, 4500, args, inj, dims, 3)
    graph = run_hip(state, vol, lab, box, 4500, args, inj, dims, 3, graph=True)
    _same(eager, again)                                     # two eager steps from the same state
    _same(eager, graph)                                     # the captured iteration, replayed
    assert bool(torch.isfinite(eager["losses"]).all()) and float(eager["losses"].min()) > 0


def update_agreement(sd, state, after):
    """tests/test_train_step_gpu.py::update_agreement."""
    num = den = 0.0
    cos_min, cos_key = 1.0, None
    for k, v in sd.items():
        if not v.is_floating_point() or k.endswith(("running_mean", "running_var")):
            continue
        ug = (after[k].cpu().double() - state[k].double()).flatten()
        uo = (v.detach().double() - state[k].double()).flatten()
        num += float(((ug - uo) ** 2).sum())
        den += float((uo ** 2).sum())
        if k.endswith(("conv_conv.0.bias", "conv_conv.4.bias")) or float(uo.norm()) == 0:
            continue
        c = float((ug * uo).sum() / (ug.norm() * uo.norm() + 1e-300))
        if c < cos_min:
            cos_min, cos_key = c, k
    return (num / den) ** 0.5, cos_min, cos_key


def _oracle_state(state):
    sd = {k: v.clone() for k, v in state.items()}
    for k, v in sd.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    return sd, {k: torch.zeros_like(v) for k, v in sd.items() if v.requires_grad}


def test_three_class_iteration_with_channel_dropout_matches_oracle():
    """tests/test_train_step_gpu.py::test_iteration_with_channel_dropout_matches_oracle at three classes: the fp_loss term (mean cross-entropy, the
    (k_dice, k_ce) = (0, 1) call of the loss kernels) and GradSim's split backward, eager against the oracle and replay against eager."""
    from oracle import filter_dropout as ofd
    C, B, lbs, H, W = 3, 8, 4, 64, 64
    U = B - lbs
    args = dict(labeled_bs=lbs, batch_size=B, vat_iters=1, dropout=True, adv_noise=False, num_classes=C)
    state = oinit.dual_decoder_2d_state(505, n_class=C)
    vol, lab = ots.synthetic_batch(2468, lbs, U, H, W, C)
    _, scores, uniforms = ofd.fd_inputs(B=U)
    inj_cpu = {"drop_A": oinit.drop_masks_2d(1, U, H, W), "drop_B": oinit.drop_masks_2d(2, lbs // 2 + U // 2, H, W),
               "drop_FP": oinit.drop_masks_2d(6, U, H, W), "fp_uniforms": uniforms, "sim_score": scores}
    box, it0 = (5, 9), 3000
    sd, moms = _oracle_state(state)
    ref = ots.iteration(sd, moms, vol, lab, box, iter_num=it0, lr=0.01, args=args, inject=inj_cpu)
    m = make_net(2, C).to(DEV).train()
    m.load_state_dict(state, strict=True)
    step = ChapStep(m, args)
    step.iter_num = it0
    inj = {k: (cl_masks(v) if k.startswith("drop") else v) for k, v in inj_cpu.items()}
    out = step.step(vol.to(DEV), lab.to(DEV), box_yx=box, inject=inj)
    torch.cuda.synchronize()
    for got, want in zip(out["fp_losses"], ref["fp_losses"]):
        assert relerr(got.cpu(), want.reshape(1)) < 2e-4
    for got, want in zip(out["mix_losses"], ref["losses"]):
        assert relerr(got.cpu(), torch.stack([w.detach() for w in want])) < 2e-4
    after = m.state_dict()
    rel_l2, cos_min, cos_key = update_agreement(sd, state, after)
    print("C=3 dropout: update rel L2 %.3g, cos_min %.5f (%s)" % (rel_l2, cos_min, cos_key))
    assert rel_l2 < 0.03, rel_l2
    assert cos_min > 0.995, (cos_min, cos_key)
    m2 = make_net(2, C).to(DEV).train()
    m2.load_state_dict(state, strict=True)
    step2 = ChapStep(m2, args)
    step2.iter_num = it0
    inj2 = dict(inj, fp_uniforms=[(a.to(DEV), b.to(DEV)) for a, b in uniforms], sim_score=[sc.to(DEV) for sc in scores])
    step2.capture(vol.to(DEV), lab.to(DEV), warmup=1, inject=inj2)
    step2.replay(vol.to(DEV), lab.to(DEV), box_yx=box)
    torch.cuda.synchronize()
    after2 = m2.state_dict()
    assert [k for k in after if not torch.equal(after[k], after2[k])] == []
    # the scores produced by GradSim (no injected sim_score): the split backward through the single-term loss calls, eager == replay
    res = []
    inj3 = {k: v for k, v in inj2.items() if k != "sim_score"}
    for graph in (False, True):
        m3 = make_net(2, C).to(DEV).train()
        m3.load_state_dict(state, strict=True)
        step3 = ChapStep(m3, args)
        step3.iter_num = it0
        if graph:
            step3.capture(vol.to(DEV), lab.to(DEV), warmup=1, inject=inj3)
            step3.replay(vol.to(DEV), lab.to(DEV), box_yx=box)
        else:
            step3.step(vol.to(DEV), lab.to(DEV), box_yx=box, inject=inj3)
        torch.cuda.synchronize()
        res.append(({k: v.clone() for k, v in m3.state_dict().items()}, [s.clone() for s in step3.gradsim.get_sim()]))
    assert [k for k in res[0][0] if not torch.equal(res[0][0][k], res[1][0][k])] == []
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1])) and any(float(s.abs().max()) > 0 for s in res[0][1])


def test_three_class_ablation_iteration_matches_oracle():
    """tests/test_train_step_gpu.py::test_ablation_iteration_matches_oracle at three classes, with its bounds."""
    C, B, lbs, H, W = 3, 8, 4, 64, 64
    U = B - lbs
    args = dict(labeled_bs=lbs, batch_size=B, vat_iters=1, w_adv=0.7, num_classes=C)
    state = oinit.dual_decoder_2d_state(404, n_class=C)
    vol, lab = ots.synthetic_batch(4321, lbs, U, H, W, C)
    inj_cpu = {"drop_F": oinit.drop_masks_2d(11, B, H, W), "drop_V0": oinit.drop_masks_2d(13, U, H, W), "drop_VF": oinit.drop_masks_2d(14, U, H, W),
               "d0": torch.rand(U, 1, H, W, generator=torch.Generator().manual_seed(15)) - 0.5}
    it0 = 3000
    sd, moms = _oracle_state(state)
    ref = ots.ablation_iteration(sd, moms, vol, lab, iter_num=it0, lr=0.01, args=args, inject=inj_cpu)
    inj = {k: (cl_masks(v) if k.startswith("drop") else v.to(DEV)) for k, v in inj_cpu.items()}
    afters = []
    for graph in (False, True):
        m = make_net(2, C).to(DEV).train()
        m.load_state_dict(state, strict=True)
        step = AblationStep(m, args)
        step.iter_num = it0
        if graph:
            step.capture(vol.to(DEV), lab.to(DEV), warmup=1, inject=inj)
            out = step.replay(vol.to(DEV), lab.to(DEV))
        else:
            out = step.step(vol.to(DEV), lab.to(DEV), inject=inj)
        torch.cuda.synchronize()
        afters.append({k: v.clone() for k, v in m.state_dict().items()})
        if not graph:
            for got, want in zip(out["sup_losses"] + out["cps_losses"], ref["sup"] + ref["cps"]):
                assert relerr(got.cpu(), want.reshape(1)) < 2e-4
            assert relerr(out["vat_loss"].cpu(), ref["vat_loss"].reshape(1)) < 5e-3
            rel_l2, cos_min, cos_key = update_agreement(sd, state, afters[0])
            print("C=3 ablation: update rel L2 %.3g, cos_min %.5f (%s)" % (rel_l2, cos_min, cos_key))
            assert rel_l2 < 0.03, rel_l2
            assert cos_min > 0.995, (cos_min, cos_key)
    assert [k for k in afters[0] if not torch.equal(afters[0][k], afters[1][k])] == []


# ---- the schedule: which launches pass B issues changes with the class count ------------------------------------------------------------
def test_captured_three_class_iteration_has_no_unordered_conflict():
    from tests import issue_trace, launch_order
    state, vol, lab, box, args, inj = case_2d(3)
    m = make_net(2, 3).to(DEV).train()
    m.load_state_dict(state, strict=True)
    step = ChapStep(m, dict(args, vat_iters=2))
    step.iter_num = 4500
    injd = to_dev(inject_2d(4, 4, 64, 64, 2), 2)
    rec = issue_trace.RichRecorder(True, issue_trace._Allocations(True), pack_entries=issue_trace._pack_entries_of(m))
    with rec.recording():
        step.capture(vol.to(DEV), lab.to(DEV), warmup=1, inject=injd)
    torch.cuda.synchronize()
    plain, rich = rec.text(), rec.rich_text()
    names = [ln.split()[1] for ln in plain.splitlines() if ln.startswith("L ")]
    assert names.count("chap_mix_loss_fwd") == 4 and names.count("chap_mix_loss_bwd") == 4           # the single-term calls ...
    assert "chap_mix_loss_multi_fwd" not in names and "chap_mix_loss_multi_bwd" not in names
    assert names.count("chap_bcp_mix") == 1 and names.count("chap_largest_cc") == 1                  # ... while largest-CC and the BCP mixing stay batched
    an = launch_order.Analysis(rich)
    found, c = an.findings(), an.counts()
    print("2d_captured_c3: %d launches, %d streams, %d conflicting pairs all ordered but %d" % (c["launches"], c["streams"], c["ordered_conflicts"], len(found)))
    assert c["launches"] == len(names) > 0 and c["ordered_conflicts"] > 0
    bare = [ln for ln in rich.splitlines() if ln.startswith("L ") and not ln.partition(" | ")[2].strip()]
    assert bare == [] and found == [], "%d unordered conflicts, the first:\n%s" % (len(found), "\n".join(f["text"] for f in found[:10]))


# ---- the public entries ---------------------------------------------------------------------------------------------------------------------
def dice_per_class(pred, gt, n_classes):
    out = []
    for c in range(1, n_classes):
        p, g = (pred == c), (gt == c)
        den = p.sum() + g.sum()
        out.append(2.0 * (p & g).sum() / den if den > 0 else 1.0)
    return np.array(out, dtype=np.float64)


def test_train_2d_three_classes_and_checkpoint_parity(tmp_path):
    """train_ours_2D.train on its synthetic data at three classes; the saved checkpoint evaluated by the HIP path and by the oracle (the
    criterion of tests/test_training_parity_gpu.py::test_trained_model_dice_matches_oracle_inference)."""
    from chap_amd.train_ours_2D import train
    C, H, W = 3, 64, 64
    snap = str(tmp_path / "run")
    model = train(dict(model="dualdecoder", decoder_type="mcnet", num_classes=C, batch_size=8, labeled_bs=4, image_size=[H, W],
                       max_iterations=300, val_interval=150, base_lr=0.05, gpu=0, seed=1337), snap)
    files = sorted(os.listdir(snap))
    assert "latest.pth" in files and "log.txt" in files
    assert ("dualdecoder_best_model.pth" in files) == ("val.csv" in files)
    log = open(os.path.join(snap, "log.txt")).read()
    assert "model1_mean_dice" in log
    bcp = [float(ln.split("bcp loss : ")[1].split()[0]) for ln in log.splitlines() if "bcp loss" in ln]
    assert len(bcp) == 6 and np.isfinite(bcp).all(), bcp
    ck = torch.load(os.path.join(snap, "latest.pth"), map_location="cpu")
    assert list(ck.keys()) == list(oinit.dual_decoder_2d_state(1, n_class=C).keys()) and ck["decoder1.out_conv.weight"].shape[0] == C
    fresh = make_net(2, C).to(DEV).eval()
    fresh.load_state_dict(ck, strict=True)
    val, gt = ots.synthetic_batch(4242, 6, 0, H, W, C)
    preds = []
    with torch.no_grad():
        for i in range(val.shape[0]):
            o = fresh(val[i:i + 1].to(DEV))
            preds.append(torch.argmax(torch.softmax((o[0] + o[1]) / 2.0, dim=1), dim=1).cpu())
        p_hip = torch.cat(preds).numpy()
        o1, o2 = onets.dual_decoder_2d({k: v.clone() for k, v in ck.items()}, val, train=False)
        p_ref = torch.argmax(torch.softmax((o1 + o2) / 2.0, dim=1), dim=1).numpy()
    d_ref, d_hip = dice_per_class(p_ref, gt.numpy(), C), dice_per_class(p_hip, gt.numpy(), C)
    print("C=3 trained checkpoint: Dice oracle %s HIP %s, labels equal %.5f" % (d_ref, d_hip, (p_ref == p_hip).mean()))
    assert np.abs(d_ref - d_hip).max() <= 1e-3, (d_ref, d_hip)
    assert (p_ref == p_hip).mean() > 0.999
    assert set(np.unique(p_hip).tolist()) <= set(range(C)) and len(np.unique(p_ref)) > 1      # labels of a three-class model, and not the trivial one


def test_train_3d_three_classes(tmp_path, monkeypatch):
    from chap_amd import train_ours_3D as T3
    losses = []

    class Recording(ChapStep):
        def replay(self, *a, **k):
            out = super().replay(*a, **k)
            losses.append([float(l[2]) for l in out["mix_losses"]] + [float(out["vat_loss"])])
            return out

    monkeypatch.setattr(T3, "ChapStep", Recording)
    snap = str(tmp_path / "run")
    model = T3.train(dict(patch_size=[16, 32, 16], num_classes=3, batch_size=4, labeled_bs=2, max_iterations=6, val_interval=3, stride_xy=8, stride_z=8, seed=3), snap)
    assert {"latest.pth", "log.txt"} <= set(os.listdir(snap))
    assert len(losses) == 6 and np.isfinite(np.array(losses)).all() and min(l[0] for l in losses) > 0
    assert "iteration 6 : dice_score : " in open(os.path.join(snap, "log.txt")).read()
    ck = torch.load(os.path.join(snap, "latest.pth"), map_location="cpu")
    assert list(ck.keys()) == list(oinit.dual_decoder_3d_state(1, n_class=3).keys()) and ck["decoder1.out_conv.weight"].shape[0] == 3
    assert all(torch.isfinite(p).all() for p in model.parameters())
