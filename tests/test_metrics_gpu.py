"""chap_metrics (chap_amd.metrics) against the scipy restatement of tests/metrics_restatement.py: border maps and squared distance
fields bit for bit, the seven medpy metrics, the empty-mask errors, per_class against the per-class calls, the inference callers."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import metrics_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _blobs(rng, shape, p=0.5, sigma=1.5):
    return ndimage.gaussian_filter(rng.random(shape), sigma) > np.quantile(ndimage.gaussian_filter(rng.random(shape), sigma), p)


def _run(a, b, spacing=None, classes=None):
    from chap_amd import metrics
    rec, (ba, bb, dist) = metrics._run(a, b, classes, spacing, binary=classes is None)
    return rec, ba.cpu().numpy(), bb.cpu().numpy(), dist.cpu().numpy()


def _border_cases():
    rng = np.random.default_rng(11)
    cases = [_blobs(rng, (37, 29)), _blobs(rng, (9, 23, 31)), _blobs(rng, (1, 40, 40)), _blobs(rng, (40, 40))]
    line = np.zeros((7, 9, 11), bool); line[3, 4, :] = True; line[:, 2, 5] = True          # 1-voxel-thick objects
    cases.append(line)
    faces = np.zeros((6, 7, 8), bool); faces[0] = True; faces[-1] = True; faces[:, 0] = True; faces[:, :, -1] = True
    cases.append(faces)                                                                    # objects on every face
    cases.append(np.ones((5, 6, 7), bool))                                                  # the full array
    one = np.zeros((5, 6, 7), bool); one[2, 3, 4] = True
    cases.append(one)                                                                       # a single voxel
    full2 = np.ones((13, 17), bool)
    cases.append(full2)
    return cases


def test_border_maps_bitwise():
    cases = _border_cases()
    for i, a in enumerate(cases):
        b = cases[(i + 1) % len(cases)]
        if b.shape != a.shape:
            b = np.roll(a, 1, axis=-1)
        rec, ba, bb, _ = _run(a, b)
        want_a = R.border(a).reshape(ba.shape).astype(np.uint8)
        want_b = R.border(b).reshape(bb.shape).astype(np.uint8)
        assert np.array_equal(ba, want_a), i
        assert np.array_equal(bb, want_b), i
        assert (rec["n_a"][0], rec["n_b"][0], rec["n_ab"][0]) == (a.sum(), b.sum(), (a & b).sum())
    sq = np.zeros((40, 40), bool); sq[10:30, 10:30] = True
    _, b2, _, _ = _run(sq, sq)
    _, b3, _, _ = _run(sq[None], sq[None])
    assert b2.sum() == 76 and b3.sum() == 400           # 2D: the ring; [1, 40, 40]: every voxel (3D footprint)


@pytest.mark.parametrize("shape,spacing", [((23, 31), None), ((6, 610, 19), None), ((5, 13, 640), None), ((11, 17, 29), None),
                                           ((7, 620, 21), (0.625, 0.625, 2.5)), ((9, 14, 33), (0.625, 0.625, 2.5)),
                                           ((31, 43), (0.7, 1.3))])
def test_distance_fields(shape, spacing):
    rng = np.random.default_rng(sum(shape))
    a = _blobs(rng, shape, 0.6, 2.0)
    b = _blobs(rng, shape, 0.4, 2.0)
    _, _, _, dist = _run(a, b, spacing)
    for d, feat in ((0, R.border(b)), (1, R.border(a))):
        want = ndimage.distance_transform_edt(~feat, sampling=spacing).reshape(dist.shape[2:])
        got = np.sqrt(dist[0, d])                 # the kernel keeps squared distances; scipy returns sqrt of its squared sum
        if spacing is None:
            assert np.array_equal(got, want), (shape, d, np.abs(got - want).max())
            assert np.array_equal(dist[0, d], np.round(dist[0, d]))          # integers: exact
        else:
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def _pairs():
    rng = np.random.default_rng(2024)
    out = []
    for i in range(24):
        shape = [(20, 24), (33, 27), (7, 19, 23), (12, 16, 10)][i % 4]
        sp = [None, (0.625, 0.625, 2.5)[-len(shape):], 1.5, None][i // 6 % 4]
        a = _blobs(rng, shape, 0.5 + 0.04 * (i % 5), 1.0 + 0.3 * (i % 3))
        b = _blobs(rng, shape, 0.55, 1.2)
        out.append((a, b, sp))
    # HD95 over n samples: 0.95 * (n - 1) integral (n - 1 a multiple of 20) and not
    for m in (20, 40, 21, 33):
        a = np.zeros((60, 60), bool); a[30, 30] = True
        b = np.zeros((60, 60), bool)
        for j in range(m - 1):
            b[2 * (j // 29) + 1, 2 * (j % 29) + 1] = True                   # isolated voxels: each its own border
        out.append((a, b, None))
    return out


def test_seven_metrics_match_restatement():
    from chap_amd import metrics
    integral = set()
    for a, b, sp in _pairs():
        n = len(R.sds(a, b, sp)) + len(R.sds(b, a, sp))
        integral.add(float(np.float64(n - 1) * 0.95).is_integer())
        for name, f in R.ALL.items():
            want = f(a, b) if name in ("dc", "jc", "ravd") else f(a, b, voxelspacing=sp)
            got = getattr(metrics.binary, name)(a, b) if name in ("dc", "jc", "ravd") else getattr(metrics.binary, name)(a, b, voxelspacing=sp)
            if name in ("dc", "jc", "ravd"):
                assert got == want, (name, got, want)
            else:
                assert abs(got - want) <= 1e-12 * abs(want), (name, sp, got, want)
            if sp is None and name in ("hd", "hd95"):
                assert got == want, (name, got, want)
    assert integral == {True, False}


def test_empty_masks():
    from chap_amd import metrics
    z = np.zeros((6, 7), bool)
    o = z.copy(); o[2, 3] = True
    assert metrics.dc(z, z) == 0.0 and metrics.dc(o, z) == 0.0
    with pytest.raises(ZeroDivisionError):
        metrics.jc(z, z)
    assert metrics.jc(o, z) == 0.0
    with pytest.raises(RuntimeError):
        metrics.ravd(o, z)
    assert metrics.ravd(z, o) == -1.0
    for f in (metrics.hd, metrics.hd95, metrics.asd, metrics.assd):
        for x, y in ((z, o), (o, z), (z, z)):
            with pytest.raises(RuntimeError):
                f(x, y)


def test_per_class_equals_binary_calls_and_is_reproducible():
    from chap_amd import metrics
    rng = np.random.default_rng(5)
    shape = (9, 40, 37)
    pred = np.zeros(shape, np.int64)
    lab = np.zeros(shape, np.uint8)
    for c in (1, 2, 3):
        pred[_blobs(rng, shape, 0.75, 2.0)] = c
        lab[_blobs(rng, shape, 0.75, 2.0)] = c
    classes = [1, 2, 3, 4]                                # class 4 is absent: NaN surface statistics
    r = metrics.per_class(pred, lab, classes)
    for k, c in enumerate(classes[:3]):
        s = metrics.binary_all(pred == c, lab == c)
        for name in ("dc", "jc", "ravd", "hd", "hd95", "asd", "assd"):
            assert r[name][k] == s[name], (c, name)
    assert r["n_a"][3] == 0 and math.isnan(r["hd95"][3]) and r["dc"][3] == 0.0
    r2 = metrics.per_class(pred, lab, classes)
    for name in r:
        assert np.array_equal(r[name], r2[name], equal_nan=True), name
    variants = [(torch.from_numpy(pred), torch.from_numpy(lab)), (torch.from_numpy(pred).to(DEV), torch.from_numpy(lab).to(DEV)),
                (torch.from_numpy(np.ascontiguousarray(pred.transpose(2, 1, 0))).to(DEV).permute(2, 1, 0),
                 torch.from_numpy(np.ascontiguousarray(lab.transpose(2, 1, 0))).permute(2, 1, 0))]
    for p, l in variants:
        r3 = metrics.per_class(p, l, classes)
        for name in r:
            assert np.array_equal(r[name], r3[name], equal_nan=True), name
    # bool / uint8 / int64 masks give the same binary result
    s0 = metrics.binary_all(pred == 2, lab == 2)
    s1 = metrics.binary_all((pred == 2).astype(np.uint8), torch.from_numpy((lab == 2).astype(np.int64) * 7).to(DEV))
    assert all(s0[k] == s1[k] for k in ("dc", "hd", "hd95", "asd", "assd"))


class _OneHot(torch.nn.Module):
    """Logits that are the one-hot of the (rounded) input intensities: the prediction is the input image itself."""

    def __init__(self, C):
        super().__init__()
        self.C = C

    def forward(self, x):
        lab = x[:, 0].round().long().clamp(0, self.C - 1)
        return torch.nn.functional.one_hot(lab, self.C).movedim(-1, 1).float().contiguous()


def test_test_single_volume_hd95_and_guards():
    try:
        import medpy  # noqa: F401
        pytest.skip("medpy installed: test_single_volume keeps the medpy path")
    except ImportError:
        pass
    from chap_amd import inference
    rng = np.random.default_rng(9)
    S, X, Y = 4, 48, 40
    img = np.zeros((S, X, Y), np.float32)
    img[_blobs(rng, (S, X, Y), 0.6, 2.0)] = 1.0
    img[_blobs(rng, (S, X, Y), 0.85, 2.0)] = 2.0          # class 2: predicted, absent from the label -> (dice, NaN)
    lab = np.zeros((S, X, Y), np.int64)
    lab[_blobs(rng, (S, X, Y), 0.6, 2.0)] = 1
    lab[_blobs(rng, (S, X, Y), 0.9, 2.0)] = 3          # class 3: in the label, never predicted -> (0, 0)
    net = _OneHot(4)
    pred = inference.predict_volume(img, net, (X, Y), "model1", DEV)
    assert np.array_equal(pred, img.astype(np.uint8))
    out = inference.test_single_volume(torch.from_numpy(img)[None], torch.from_numpy(lab)[None], net, classes=4,
                                       patch_size=[X, Y], model_type="model1", device=DEV)
    d1, h1 = out[0]
    assert math.isfinite(h1) and h1 > 0
    assert d1 == R.dc(pred == 1, lab == 1)
    assert abs(h1 - R.hd95(pred == 1, lab == 1)) <= 1e-12 * h1
    d2, h2 = out[1]
    assert d2 == 0.0 and math.isnan(h2)
    assert out[2] == (0, 0)


def test_calculate_metric_percase_on_test_single_case():
    from chap_amd import inference
    rng = np.random.default_rng(13)
    w, h, d = 30, 28, 20
    img = _blobs(rng, (w, h, d), 0.6, 2.0).astype(np.float32)
    gt = _blobs(rng, (w, h, d), 0.6, 2.0).astype(np.int64)
    label_map = inference.test_single_case(_OneHot(2), img, 8, 8, (16, 16, 16), num_classes=2, device=DEV)
    assert np.array_equal(label_map, img.astype(np.int64))
    got = inference.calculate_metric_percase(label_map == 1, gt == 1)
    want = np.array([R.dc(label_map == 1, gt == 1), abs(R.ravd(label_map == 1, gt == 1)), R.hd95(label_map == 1, gt == 1),
                     R.asd(label_map == 1, gt == 1)])
    assert got[0] == want[0] and got[1] == want[1]
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-12, atol=0)


def _la_pair():
    """LA-like: two 88 x 576 x 576 ellipsoids with noisy surfaces."""
    D, H, W = 88, 576, 576
    z, y, x = np.ogrid[:D, :H, :W]
    rng = np.random.default_rng(3)
    noise = ndimage.zoom(rng.standard_normal((12, 36, 36)), (D / 12, H / 36, W / 36), order=1)
    ra = ((z - 44) / 30.0) ** 2 + ((y - 290) / 150.0) ** 2 + ((x - 280) / 170.0) ** 2
    rb = ((z - 46) / 28.0) ** 2 + ((y - 284) / 156.0) ** 2 + ((x - 290) / 160.0) ** 2
    return ra + 0.08 * noise < 1.0, rb - 0.08 * noise < 1.0


def test_la_sized_case():
    from chap_amd import metrics
    a, b = _la_pair()
    s = metrics.binary_all(a, b)
    ba, bb = R.border(a), R.border(b)
    s_ab = ndimage.distance_transform_edt(~bb)[ba]
    s_ba = ndimage.distance_transform_edt(~ba)[bb]
    assert s["dc"] == R.dc(a, b) and s["jc"] == R.jc(a, b) and s["ravd"] == R.ravd(a, b)
    assert s["hd"] == max(s_ab.max(), s_ba.max())
    assert s["hd95"] == np.percentile(np.hstack((s_ab, s_ba)), 95)
    assert abs(s["asd"] - s_ab.mean()) <= 1e-12 * s_ab.mean()
    assert abs(s["assd"] - np.mean((s_ab.mean(), s_ba.mean()))) <= 1e-12 * s["assd"]


def test_train_logs_mean_hd95(tmp_path):
    from chap_amd.train_ours_2D import train
    snap = str(tmp_path / "run")
    train(dict(model="dualdecoder", decoder_type="mcnet", num_classes=4, batch_size=8, labeled_bs=4, image_size=[64, 64],
               max_iterations=4, val_interval=4, base_lr=0.05, gpu=0, seed=7, use_graph=False), snap)
    log = open(tmp_path / "run" / "log.txt").read()
    assert "model1_mean_dice" in log and "model1_mean_hd95" in log
