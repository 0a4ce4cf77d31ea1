"""Residual V-Net blocks (has_residual=True) through the nn.Module boundary on the GPU: eval logits against the imported reference's
(tests/golden/vnet_residual_32.npz), train mode with injected Dropout3d masks against the fp64 restatement tests/vnet_residual_ref.py run
on the CPU here, one state dict in both architectures, and the training iteration eager against captured.  The bounds are those
tests/test_net3d_gpu.py applies to the plain nets: fp32 logits 1e-4 relative (max norm), bf16 5e-2 and 0.99 arg-max agreement, gradients
against the fp64 run within max(4 x the fp32 restatement's own distance from it, 2e-2), running statistics 1e-4."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd.networks import DualDecoder3d, VNet
from oracle import init as oinit
from tests import vnet_residual_ref as rref
from tests.test_net2d_gpu import relerr, run_case
from tests.test_net3d_gpu import chan_masks

DEV = "cuda"
SUB = (slice(None), slice(None), slice(None, None, 2), slice(None, None, 2), slice(None, None, 2))
COT_SEED, MASK_SEED = 37, 43
PICKS = ("encoder.block_two.conv.3.weight",        # a last-stage conv (BatchNorm without ReLU behind it)
         "encoder.block_one.conv.0.weight",        # the first conv: its block's input is the image itself
         "decoder1.block_six.conv.0.weight")       # reads up + x4; x4 collects five gradient contributions (the grad_sum fold)
KW = dict(n_channels=1, n_classes=2, normalization="batchnorm")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "vnet_residual_32.npz"), allow_pickle=False)


def _model(cls, state, **kw):
    m = cls(has_residual=True, **dict(KW, **kw)).to(DEV)
    m.load_state_dict(state, strict=True)
    return m


@pytest.fixture(scope="module")
def eval32(fixture):
    """fp32 eval logits of both nets on the fixture's input (shared by the fp32 and the bf16 test)."""
    x = torch.from_numpy(fixture["x"]).to(DEV)
    with torch.no_grad():
        d = _model(DualDecoder3d, oinit.dual_decoder_3d_state(int(fixture["state_seed"]))).eval()(x)
        v = _model(VNet, oinit.vnet_state(int(fixture["vnet_state_seed"]))).eval()(x)
    return d[0], d[1], v


def test_eval_fp32_against_the_reference(fixture, eval32):
    g = fixture
    assert relerr(eval32[0], g["eval_logits0"]) < 1e-4
    assert relerr(eval32[1], g["eval_logits1"]) < 1e-4
    assert relerr(eval32[2], g["vnet_eval_logits"]) < 1e-4


def test_eval_bf16_against_the_reference(fixture, eval32):
    g = fixture
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        b1, b2 = _model(DualDecoder3d, oinit.dual_decoder_3d_state(int(g["state_seed"]))).set_compute_dtype(torch.bfloat16).eval()(x)
        bv = _model(VNet, oinit.vnet_state(int(g["vnet_state_seed"]))).set_compute_dtype(torch.bfloat16).eval()(x)
    for got, key, f32 in ((b1, "eval_logits0", eval32[0]), (b2, "eval_logits1", eval32[1]), (bv, "vnet_eval_logits", eval32[2])):
        e, agree = relerr(got, g[key]), float((got.argmax(1) == f32.argmax(1)).float().mean())
        print("bf16 %s: relerr %.3g argmax agreement %.5f" % (key, e, agree))
        assert e < 5e-2, key
        assert agree > 0.99, key


def test_train_mode_without_dropout_against_the_reference(fixture):
    """Batch statistics, no dropout: the reference's train-mode logits (every second voxel per axis is stored) and the running statistics it
    leaves in a last-stage BatchNorm layer and an ordinary one."""
    g = fixture
    x = torch.from_numpy(g["x"]).to(DEV)
    m = _model(DualDecoder3d, oinit.dual_decoder_3d_state(int(g["state_seed"]))).train()
    v = _model(VNet, oinit.vnet_state(int(g["vnet_state_seed"]))).train()
    with torch.no_grad():
        t1, t2 = m(x)
        tv = v(x)
    assert relerr(t1[SUB], g["train_logits0_sub"]) < 1e-4 and relerr(t2[SUB], g["train_logits1_sub"]) < 1e-4
    assert relerr(tv[SUB], g["vnet_train_logits_sub"]) < 1e-4
    sd = m.state_dict()
    for k in g["bn_layers"]:
        assert relerr(sd[str(k) + ".running_mean"], g["after_rm_" + str(k)]) < 1e-4, k
        assert relerr(sd[str(k) + ".running_var"], g["after_rv_" + str(k)]) < 1e-4, k
    assert int(sd["encoder.block_two.conv.4.num_batches_tracked"]) == 1


def _restated(state, x, masks, dtype):
    """Train-mode forward + backward of the restatement against run_case's cotangents: logits, dx, picked gradients, the state after."""
    sd = rref.cast_state(state, dtype)
    for k in PICKS:
        sd[k].requires_grad_(True)
    xr = torch.from_numpy(x).to(dtype).requires_grad_(True)
    outs = rref.dual_decoder_3d(sd, xr, train=True, drop=masks, has_dropout=True)
    gen = torch.Generator().manual_seed(COT_SEED)
    cots = [torch.randn(o.shape, generator=gen).to(dtype) for o in outs]
    torch.autograd.backward(outs, cots)
    return dict(logits=[o.detach() for o in outs], dx=xr.grad, grads={k: sd[k].grad for k in PICKS}, sd=sd)


@pytest.fixture(scope="module")
def train_ref(fixture):
    state = oinit.dual_decoder_3d_state(int(fixture["state_seed"]))
    masks = oinit.drop_masks_3d(MASK_SEED, 2)
    return state, masks, _restated(state, fixture["x"], masks, torch.float64), _restated(state, fixture["x"], masks, torch.float32)


def test_train_mode_injected_masks_against_fp64(fixture, train_ref, monkeypatch):
    state, masks, r64, r32 = train_ref
    m = _model(DualDecoder3d, state, has_dropout=True).train()
    outs, dx = run_case(m, fixture["x"], COT_SEED, drop_masks=chan_masks(masks))
    for h in range(2):
        e = relerr(outs[h], r64["logits"][h])
        print("train logits head %d: relerr %.3g" % (h, e))
        assert e < 1e-4
    ref_err = relerr(r32["dx"], r64["dx"])
    e = relerr(dx, r64["dx"])
    print("dx: relerr %.3g (fp32 restatement %.3g)" % (e, ref_err))
    assert e < max(4 * ref_err, 2e-2)
    grads = dict(m.named_parameters())
    for k in PICKS:
        ref_e = relerr(r32["grads"][k], r64["grads"][k])
        e = relerr(grads[k].grad, r64["grads"][k])
        print("%s: relerr %.3g (fp32 restatement %.3g)" % (k, e, ref_e))
        assert e < max(4 * ref_e, 2e-2), k
    sd = m.state_dict()
    for k in fixture["bn_layers"]:
        assert relerr(sd[str(k) + ".running_mean"], r64["sd"][str(k) + ".running_mean"]) < 1e-4, k
        assert relerr(sd[str(k) + ".running_var"], r64["sd"][str(k) + ".running_var"]) < 1e-4, k
    # dx contains the gradient through block_one's residual add (chap_residual_bwd's dxin): the first conv's input gradient alone is another tensor
    from chap_amd import engine
    monkeypatch.setattr(engine.ops, "perturb", lambda *a, **k: None)
    m2 = _model(DualDecoder3d, state, has_dropout=True).train()
    _, dx_conv_only = run_case(m2, fixture["x"], COT_SEED, drop_masks=chan_masks(masks))
    print("dx without dxin: relerr %.3g" % relerr(dx_conv_only, r64["dx"]))
    assert float((dx - dx_conv_only).norm()) > 0


def test_frozen_pass_gives_dx_only(fixture):
    """frozen() + update_stats=False (the VAT passes): dL/dx, no parameter gradients, running statistics untouched; in-kernel Dropout3d masks."""
    m = _model(DualDecoder3d, oinit.dual_decoder_3d_state(int(fixture["state_seed"])), has_dropout=True).train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.from_numpy(fixture["x"]).to(DEV).requires_grad_(True)
    with m.frozen():
        a, b = m(x, update_stats=False)
        (a.sum() + b.sum()).backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    assert all(p.grad is None or p.grad.abs().sum() == 0 for p in m.parameters())
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_one_state_dict_two_architectures(fixture):
    state = oinit.dual_decoder_3d_state(int(fixture["state_seed"]))
    x = torch.from_numpy(fixture["x"]).to(DEV)
    outs = {}
    for flag in (True, False):
        m = DualDecoder3d(has_residual=flag, **KW).to(DEV)
        m.load_state_dict(state, strict=True)
        with torch.no_grad():
            outs[flag] = m.eval()(x)
        back = m.state_dict()
        assert list(back.keys()) == list(state.keys())
        assert all(torch.equal(back[k].cpu(), state[k]) for k in state)
    assert relerr(outs[True][0], outs[False][0]) > 0.1 and relerr(outs[True][1], outs[False][1]) > 0.1


def test_training_iteration_eager_equals_captured():
    """ChapStep on DualDecoder3d(has_residual=True, has_dropout=True), 2 labelled + 2 unlabelled samples at 32 x 32 x 16, VAT on: three eager steps
    (decoders on two streams, deferred decoder weight gradients) against capture + three replays (pass B and the early VAT pass run the
    decoders in lockstep: the residual adds of the two decoders are the lanes of grouped launches) -- losses and the flat parameter buffer bit
    for bit, losses finite.  The loss VALUES are tied to the oracle: the eager run's mix_losses of the first step against
    oracle.train_step.iteration driving the residual restatement (net=tests.vnet_residual_ref.dual_decoder_3d) in fp32 with the same injected
    randomness, within the 5e-4 (max norm, relative) of tests/test_iteration_conditioning_gpu.py's small 3D cases; the whole iteration is judged there
    (test_small_3d_residual_iteration_is_as_close_to_fp64_as_the_fp32_oracle)."""
    from chap_amd.train import ChapStep
    from oracle import train_step as ots
    from tests.iteration_parity import _rel, inject_3d, run_oracle, to_dev
    B, lbs, sp = 4, 2, (32, 32, 16)
    state = oinit.dual_decoder_3d_state(401)
    vol, lab = ots.synthetic_batch_3d(1337, lbs, B - lbs, *sp)
    inj_cpu = inject_3d(B - lbs, lbs // 2 + (B - lbs) // 2, sp, 1)
    inj = to_dev(inj_cpu, 3)
    box = (4, 5, 3)
    res = {}
    for mode in ("eager", "graph"):
        m = DualDecoder3d(has_residual=True, has_dropout=True, **KW).to(DEV).train()
        m.load_state_dict(state, strict=True)
        step = ChapStep(m, dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=2, adv_noise=True))
        step.iter_num = 4500
        start = m.flat_buffers()[0].clone()
        if mode == "graph":
            step.capture(vol.to(DEV), lab.to(DEV), warmup=1, inject=inj)
        losses = []
        for _ in range(3):
            out = step.step(vol.to(DEV), lab.to(DEV), box_yx=box, inject=inj) if mode == "eager" else step.replay(vol.to(DEV), lab.to(DEV), box_yx=box)
            losses.append([t.clone() for t in out["mix_losses"]] + [out["vat_loss"].clone()])
        torch.cuda.synchronize()
        res[mode] = (losses, m.flat_buffers()[0].clone())
        assert torch.isfinite(res[mode][1]).all() and not torch.equal(res[mode][1], start)          # the steps trained
    for a, b in zip(res["eager"][0], res["graph"][0]):
        for s, t in zip(a, b):
            assert torch.isfinite(s).all() and torch.equal(s, t), (s, t)
    assert torch.equal(res["eager"][1], res["graph"][1])
    # ... and the bit-for-bit pair has the oracle's values: the first step's mix losses against the fp32 oracle of the residual iteration
    args = dict(labeled_bs=lbs, batch_size=B, vat_iters=1, num_classes=2, adv_noise=True)
    o32 = run_oracle(state, vol, lab, box, 4500, args, inj_cpu, 3, torch.float32, residual=True)
    got = torch.stack([t.double().cpu() for t in res["eager"][0][0][:-1]])
    e = _rel(got, o32["losses"])
    print("first step's mix losses against the fp32 oracle: %.3g" % e)
    assert got.shape == o32["losses"].shape and e < 5e-4
