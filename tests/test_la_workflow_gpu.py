"""The 3D workflow end to end on the GPU (DESIGN.md "3D workflow"): chap_amd.test_3d_patch -- the device-side sliding window with a
recording stub network against the oracle's loop and the fp64 restatement of tests/la_ref.py, getLargestCC against scipy, test_all_case
against tests/metrics_restatement.py -- and chap_amd.train_ours_3D.train over a padded DeviceLoader."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import inference
from chap_amd import test_3d_patch as T
from tests import kernel_ref as kr
from tests import la_ref as LR
from tests import metrics_restatement as M

DEV = "cuda:0"
PATCH = (16, 32, 16)
CASES = [((21, 40, 13), (9, 4)), ((30, 45, 24), (8, 4))]


def _image(shape, seed=5):
    return np.random.default_rng(seed).random(shape, dtype=np.float32) + 0.5        # no zeros: the padding is recognisable


# ---------------------------------------------------------------------------------------------------- window pipeline
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("case", CASES)
def test_window_pipeline_with_a_recording_stub(case, C):
    shape, strides = case
    image = _image(shape)
    ref_patches = LR.oracle_patches(image, PATCH, *strides)
    if shape == (30, 45, 24):
        assert len(ref_patches) == 27
    results = {}
    for name, fn, nheads in (("first", T.test_single_case_first_output, 1), ("average", T.test_single_case_average_output, 2)):
        net = LR.StubNet(C).to(DEV)
        label, score = fn(net, image, *strides, PATCH, num_classes=C, batch=4, device=DEV)
        assert label.shape == shape and label.dtype == np.int64 and score.shape == (C,) + shape and score.dtype == np.float32
        # (a) the patches the network saw: the reference loop's, bitwise and in loop order, in batches of 4 (the last one shorter)
        sizes = [x.shape[0] for x, _ in net.calls]
        assert sizes == [min(4, len(ref_patches) - k0) for k0 in range(0, len(ref_patches), 4)]
        seen = torch.cat([x for x, _ in net.calls])
        want = torch.from_numpy(np.stack(ref_patches))[:, None]
        assert seen.shape == want.shape and torch.equal(seen.view(torch.int32), want.view(torch.int32))
        # (b) score and labels against the fp64 restatement fed the recorded fp32 logits, the bound carried across the launches
        r = LR.window_pipeline_ref(shape, PATCH, *strides, [outs[:nheads] for _, outs in net.calls], C)
        worst = kr.check("pipeline %s C=%d %s" % (name, C, shape), torch.from_numpy(score), r["score"], r["score_b"], "cxyz")
        share = float(r["near"].double().mean())
        print("  pipeline %-7s C=%d %s: worst err/bound %.3f, near-tie share %.2e" % (name, C, shape, worst, share))
        assert share <= LR.NEAR_TIE_CAP
        ok = ~r["near"]
        assert torch.equal(torch.from_numpy(label)[ok], r["label"][ok])
        results[name] = (label, score)
    assert not np.array_equal(results["first"][1], results["average"][1])              # the second head took part
    # a net with one output: average_output is first_output
    one = LR.StubNet(C, heads=1).to(DEV)
    label1, score1 = T.test_single_case_average_output(one, image, *strides, PATCH, num_classes=C, batch=4, device=DEV)
    assert np.array_equal(label1, results["first"][0]) and np.array_equal(score1.view(np.int32), results["first"][1].view(np.int32))
    # (c) first_output == the existing host-side window of chap_amd.inference on the same stub, labels and score bits
    old_label, old_score = inference.test_single_case(LR.StubNet(C).to(DEV), image, *strides, PATCH, num_classes=C, batch=4, device=DEV, return_score=True)
    assert np.array_equal(old_label, results["first"][0]) and np.array_equal(old_score.view(np.int32), results["first"][1].view(np.int32))


# ---------------------------------------------------------------------------------------------------- getLargestCC
def test_get_largest_cc():
    rng = np.random.default_rng(0)
    for n, density in enumerate((0.35, 0.35, 0.35, 0.1, 0.1)):       # 0.1: near the percolation threshold, many components of similar size
        seg = (rng.random((17, 19, 13)) < density) * rng.integers(1, 4, (17, 19, 13))
        got = T.getLargestCC(seg)
        assert got.dtype == seg.dtype and np.array_equal(got, LR.largest_cc_scipy(seg)), n
        assert (got > 0).any() and (density > 0.1 or (got > 0).sum() < (seg > 0).sum())
    # two components of equal size: the one met first in raster order
    seg = np.zeros((6, 7, 8), dtype=np.int64)
    seg[4:6, 0:2, 0:2] = 2
    seg[0:2, 4:6, 5:7] = 1
    got = T.getLargestCC(seg)
    assert np.array_equal(got, LR.largest_cc_scipy(seg)) and got[0, 4, 5] == 1 and not got[4:].any()
    # contact across a corner only joins (26-connectivity)
    seg = np.zeros((5, 5, 5), dtype=np.uint8)
    seg[0, 0, 0] = seg[1, 1, 1] = seg[2, 2, 2] = 1
    seg[4, 4, 0] = seg[4, 4, 1] = 1
    got = T.getLargestCC(seg)
    assert got.dtype == np.uint8 and np.array_equal(got, LR.largest_cc_scipy(seg)) and got.sum() == 3 and got[1, 1, 1] == 1
    # nothing to keep: returned unchanged (the public code asserts here)
    zero = np.zeros((4, 4, 4), dtype=np.int64)
    assert T.getLargestCC(zero) is zero
    t = torch.from_numpy(seg).to(DEV)
    assert torch.equal(T.getLargestCC(t).cpu(), torch.from_numpy(got))                  # a device tensor stays one


# ---------------------------------------------------------------------------------------------------- test_all_case
def _restated_labels(image, strides, average):
    """The label map of the restatement; a voxel it calls a near tie (none expected, at most NEAR_TIE_CAP) takes the device's label."""
    net = LR.StubNet(2).to(DEV)
    fn = T.test_single_case_average_output if average else T.test_single_case_first_output
    label, _ = fn(net, image, *strides, PATCH, num_classes=2, batch=4, device=DEV)
    r = LR.window_pipeline_ref(image.shape, PATCH, *strides, [outs[:2 if average else 1] for _, outs in net.calls], 2)
    assert float(r["near"].double().mean()) <= LR.NEAR_TIE_CAP
    return torch.where(r["near"], torch.from_numpy(label), r["label"]).numpy()


@pytest.mark.parametrize("nms", [0, 1])
@pytest.mark.parametrize("num_outputs", [1, 2])
def test_all_case_scores_like_the_restatement(num_outputs, nms, capsys):
    strides = (9, 4)
    shapes = [(21, 40, 13), (18, 30, 20), (24, 33, 16)]
    rng = np.random.default_rng(8)
    cases = []
    for n, s in enumerate(shapes):
        image = np.zeros(s, dtype=np.float32) if n == 1 else _image(s, 20 + n)           # case 1: all zeros -> an empty prediction
        gt = np.zeros(s, dtype=np.uint8)
        gt[3:3 + s[0] // 2, 5:5 + s[1] // 2, 2:2 + s[2] // 2] = 1
        gt[rng.random(s) < 0.05] = 1
        cases.append((image, gt))
    got = T.test_all_case("stub", num_outputs, LR.StubNet(2).to(DEV), cases, num_classes=2, patch_size=PATCH, stride_xy=strides[0], stride_z=strides[1],
                          save_result=False, metric_detail=1, nms=nms)
    rows = []
    for image, gt in cases:
        pred = _restated_labels(image, strides, num_outputs > 1)
        if nms:
            pred = LR.largest_cc_scipy(pred)
        rows.append((0.0, 0.0, 0.0, 0.0) if pred.sum() == 0 else (M.dc(pred, gt), M.jc(pred, gt), M.hd95(pred, gt), M.asd(pred, gt)))
    assert rows[1] == (0.0, 0.0, 0.0, 0.0) and all(r[0] > 0 for r in (rows[0], rows[2]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln[:2].isdigit()]
    assert len(lines) == 3                                       # metric_detail: one line per case
    per_case = np.array([[float(v) for v in ln.split(",")[1:]] for ln in lines])
    assert np.allclose(per_case, np.array(rows), rtol=0, atol=6e-6)                     # the printed %.5f figures
    want = (np.zeros(4) + np.asarray(rows[0]) + np.asarray(rows[1]) + np.asarray(rows[2])) / 3             # the mean over cases
    assert isinstance(got, np.ndarray) and got.shape == (4,)
    # dc, jc: integer counts, the same divisions -- the mean over cases too; hd95, asd: 1e-12 relative, as tests/test_metrics_gpu.py asserts
    assert got[0] == want[0] and got[1] == want[1]
    assert abs(got[2] - want[2]) <= 1e-12 * abs(want[2]) and abs(got[3] - want[3]) <= 1e-12 * abs(want[3])
    single = T.calculate_metric_percase(_restated_labels(cases[0][0], strides, num_outputs > 1), cases[0][1])
    if not nms:
        assert single[0] == rows[0][0] and single[1] == rows[0][1] and abs(single[2] - rows[0][2]) <= 1e-12 * rows[0][2]


def test_var_all_case_is_the_mean_foreground_dice():
    strides = (9, 4)
    cases = []
    for n, s in enumerate([(21, 40, 13), (18, 30, 20)]):
        gt = np.zeros(s, dtype=np.uint8)
        gt[2:12, 4:20, 1:9] = 1
        cases.append((_image(s, 30 + n) if n == 0 else np.zeros(s, dtype=np.float32), gt))
    got = T.var_all_case(LR.StubNet(2).to(DEV), cases, 2, PATCH, *strides)
    want = (M.dc(_restated_labels(cases[0][0], strides, False), cases[0][1]) + 0.0) / 2
    assert got == want and want > 0


# ---------------------------------------------------------------------------------------------------- training entry
def test_train_ours_3d_over_a_padded_loader(tmp_path, monkeypatch):
    """train() with a DeviceLoader(pad=True) over 8 synthetic volumes, one of them smaller than the patch: 12 iterations at
    (32, 32, 16), validation by the sliding window every 6."""
    from chap_amd import train_ours_3D as T3
    from chap_amd.data import DeviceLoader, VolumeStore
    from chap_amd.synthetic import synthetic_batch_3d
    from chap_amd.train import ChapStep
    from oracle import init as oinit
    losses, staged, initial = [], [], []

    class Recording(ChapStep):
        def __init__(self, model, *a, **k):
            initial.extend(p.detach().clone() for p in model.parameters())
            super().__init__(model, *a, **k)

        def replay(self, *a, **k):
            out = super().replay(*a, **k)
            losses.append([float(l[2]) for l in out["mix_losses"]] + [float(out["vat_loss"])])
            return out

        def stage_from(self, loader):
            staged.append(loader)
            return super().stage_from(loader)

    monkeypatch.setattr(T3, "ChapStep", Recording)
    v, l = synthetic_batch_3d(11, 10, 0, 40, 40, 24)
    crops = [(40, 40, 24), (36, 40, 20), (40, 34, 24), (33, 38, 17), (40, 40, 22), (38, 36, 24), (34, 40, 18), (28, 40, 12)]
    images = [v[i, 0, :c[0], :c[1], :c[2]].numpy().copy() for i, c in enumerate(crops)]
    labels = [l[i, :c[0], :c[1], :c[2]].numpy().astype(np.uint8) for i, c in enumerate(crops)]
    store = VolumeStore(images, labels, DEV)
    with pytest.raises(ValueError, match="smaller than the crop"):
        DeviceLoader(store, range(3), range(3, 8), 4, 2, (32, 32, 16), seed=7)
    loader = DeviceLoader(store, range(3), range(3, 8), 4, 2, (32, 32, 16), seed=7, pad=True)
    val = [(v[8, 0].numpy(), l[8].numpy()), (v[9, 0, :30, :36, :14].numpy().copy(), l[9, :30, :36, :14].numpy().copy())]
    snap = str(tmp_path / "run")
    model = T3.train(dict(patch_size=[32, 32, 16], batch_size=4, labeled_bs=2, max_iterations=12, val_interval=6, base_lr=0.05, gpu=0, seed=7,
                          stride_xy=16, stride_z=8, trainloader=loader, val_volumes=val), snap)
    assert len(losses) == 12 and np.isfinite(np.array(losses)).all()
    assert len(staged) == 11 and all(s is loader for s in staged)
    ck = torch.load(os.path.join(snap, "latest.pth"), map_location="cpu")
    state = oinit.dual_decoder_3d_state(1)
    assert list(ck.keys()) == list(state.keys()) and all(torch.isfinite(t.float()).all() for t in ck.values())
    log = open(os.path.join(snap, "log.txt")).read()
    assert "iteration 6 : dice_score : " in log and "iteration 12 : dice_score : " in log
    params = list(model.parameters())
    assert len(initial) == len(params) and any(not torch.equal(p, q) for p, q in zip(params, initial))   # the parameters changed ...
    assert all(torch.isfinite(p).all() for p in model.parameters())                                       # ... and are finite


def test_train_ours_3d_synthetic_fallback(tmp_path):
    """No loader, no data set, no validation volumes: the fixed-seed synthetic generator feeds the loop (host batches through stage())
    and the validation; three iterations at (32, 32, 16)."""
    from chap_amd import train_ours_3D as T3
    snap = str(tmp_path / "run")
    model = T3.train(dict(patch_size=[32, 32, 16], max_iterations=3, val_interval=3, stride_xy=16, stride_z=8, seed=3), snap)
    assert {"latest.pth", "log.txt"} <= set(os.listdir(snap))
    assert "iteration 3 : dice_score : " in open(os.path.join(snap, "log.txt")).read()
    assert all(torch.isfinite(p).all() for p in model.parameters())
