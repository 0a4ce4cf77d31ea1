"""Segmentation metrics on the GPU: medpy.metric.binary's dc, jc, ravd, hd, hd95, asd, assd.

The reference scores every prediction with medpy (val_2D.py:43-51, test_2D_fully.py:37-51, test_3D_util.py:82-88,147-152).  These
functions have medpy's signatures, so a caller switches with one line:

    from chap_amd import metrics as metric      # instead of `from medpy import metric`
    metric.binary.hd95(pred, gt)

`per_class` scores several classes of one pair of label maps with one launch chain (chap_metrics, include/chap_hip.h); the
medpy-named functions are thin fronts over the same core.  Inputs are numpy arrays (bool, uint8, int64, any other integer or float
type is converted) or torch tensors on the CPU or the GPU, contiguous or not; host arrays are copied to the device once, and one small
result array comes back.  Definitions (restated from scipy, tests/metrics_restatement.py):
    border(X) = X & ~binary_erosion(X, cross footprint of ndim, border_value 0)
    sds(A, B) = distance_transform_edt(~border(B), sampling=voxelspacing)[border(A)]
    hd = max of both directions, hd95 = numpy.percentile(both directions, 95), asd = mean sds(A, B), assd = mean of both asd.
"""
import math
import types

import numpy as np
import torch

from . import _lib as L
from . import ops

_RESULT = np.dtype([(name, "<i8" if t is L._i64 else "<f8") for name, t in L.MetricResult._fields_])
_Q95 = np.float64(95) / np.float64(100)          # numpy.percentile's quantile for q = 95


def _check_connectivity(connectivity):
    if connectivity != 1:
        raise NotImplementedError("chap_amd.metrics supports connectivity=1 only (got %r)" % (connectivity,))


def _spacing(voxelspacing, ndim):
    """(D, H, W) spacing of the kernel from medpy's `voxelspacing` (None, a scalar or one value per axis)."""
    if voxelspacing is None:
        s = [1.0] * ndim
    elif np.ndim(voxelspacing) == 0:
        s = [float(voxelspacing)] * ndim
    else:
        s = [float(v) for v in voxelspacing]
        if len(s) != ndim:
            raise ValueError("voxelspacing needs one value per axis (%d), got %d" % (ndim, len(s)))
    if not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError("voxelspacing must be positive and finite, got %r" % (voxelspacing,))
    return s if ndim == 3 else [1.0] + s


def _shape_of(x):
    return tuple(x.shape)


def _validate(a, b):
    sa, sb = _shape_of(a), _shape_of(b)
    if sa != sb:
        raise ValueError("result and reference must have the same shape, got %s and %s" % (sa, sb))
    if len(sa) not in (2, 3):
        raise ValueError("chap_amd.metrics supports 2D and 3D masks only, got ndim %d" % len(sa))
    if any(n > L.METRICS_MAX_AXIS for n in sa):
        raise ValueError("axis longer than %d (CHAP_METRICS_MAX_AXIS): shape %s" % (L.METRICS_MAX_AXIS, sa))
    if 0 in sa:
        raise ValueError("empty array, shape %s" % (sa,))
    return len(sa)


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(x, binary, device):
    """uint8 / int64, contiguous, [D, H, W] on the device (one host -> device copy for host inputs)."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        arr = np.asarray(x)
        if arr.dtype == np.bool_:
            arr = arr.view(np.uint8)
        elif arr.dtype.byteorder == ">":
            arr = arr.astype(arr.dtype.newbyteorder("="))
        t = torch.from_numpy(np.ascontiguousarray(arr))
    if t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
    if t.dtype not in (torch.uint8, torch.int64):
        t = (t != 0).to(torch.uint8) if binary else t.to(torch.int64)
    t = t.to(device).contiguous()
    return t if t.dim() == 3 else t.unsqueeze(0)


def _run(result, reference, classes, voxelspacing, binary, distances=True):
    """One chap_metrics chain; returns the chap_metric_result records (numpy structured array [K]) and the device tensors."""
    ndim = _validate(result, reference)
    spacing = _spacing(voxelspacing, ndim)
    if not binary:
        classes = [int(c) for c in classes]
        if not 1 <= len(classes) <= 255 or len(set(classes)) != len(classes):
            raise ValueError("classes: 1 to 255 distinct values, got %r" % (classes,))
    device = _device()
    a = _to_device(result, binary, device)
    b = _to_device(reference, binary, device)
    cls = None if binary else torch.tensor(classes, dtype=torch.int64).to(device)
    res, border_a, border_b, dist = ops.metrics(a, b, cls, ndim=ndim, spacing=spacing, binary=binary, distances=distances)
    rec = np.frombuffer(res.cpu().numpy().tobytes(), dtype=_RESULT)
    return rec, (border_a, border_b, dist)


def _lerp(a, b, t):
    """numpy's quantile interpolation (numpy/lib/_function_base_impl.py _lerp), scalars."""
    diff = b - a
    return b - diff * (1 - t) if t >= 0.5 else a + diff * t


def _hd95(r):
    n = int(r["n_ab_s"] + r["n_ba_s"])
    vi = np.float64(n - 1) * _Q95
    lo, hi = np.sqrt(np.float64(r["v2_lo"])), np.sqrt(np.float64(r["v2_hi"]))
    if vi >= n - 1:
        return lo
    return _lerp(lo, hi, vi - np.floor(vi))


def _stats(r, surface=True):
    """Every statistic of one record; NaN where a definition divides by zero or needs a non-empty mask (surface=False: a
    counts-only record, the surface statistics are NaN)."""
    n_a, n_b, n_ab = int(r["n_a"]), int(r["n_b"]), int(r["n_ab"])
    out = dict(n_a=n_a, n_b=n_b, n_ab=n_ab)
    out["dc"] = 2.0 * n_ab / float(n_a + n_b) if n_a + n_b else 0.0
    out["jc"] = float(n_ab) / float(n_a + n_b - n_ab) if n_a + n_b - n_ab else math.nan
    out["ravd"] = (n_a - n_b) / float(n_b) if n_b else math.nan
    if surface and n_a and n_b:
        asd_ab = np.float64(r["sum_ab"]) / np.float64(r["n_ab_s"])
        asd_ba = np.float64(r["sum_ba"]) / np.float64(r["n_ba_s"])
        out["hd"] = float(max(np.sqrt(np.float64(r["max2_ab"])), np.sqrt(np.float64(r["max2_ba"]))))
        out["hd95"] = float(_hd95(r))
        out["asd"] = float(asd_ab)
        out["asd_ba"] = float(asd_ba)
        out["assd"] = float(np.mean((asd_ab, asd_ba)))
    else:
        out.update(hd=math.nan, hd95=math.nan, asd=math.nan, asd_ba=math.nan, assd=math.nan)
    return out


_KEYS = ("dc", "jc", "ravd", "hd", "hd95", "asd", "asd_ba", "assd", "n_a", "n_b", "n_ab")


def per_class(prediction, label, classes, voxelspacing=None):
    """Every statistic for every class c of `classes`, with A = (prediction == c), B = (label == c), from one launch chain.
    Returns a dict of numpy arrays [len(classes)]: dc, jc, ravd, hd, hd95, asd (= asd(A, B)), asd_ba (= asd(B, A)), assd (float64;
    NaN where medpy would raise: jc of two empty masks, ravd of an empty B, a surface statistic of an empty A or B) and the counts
    n_a, n_b, n_ab (int64)."""
    rec, _ = _run(prediction, label, classes, voxelspacing, binary=False)
    rows = [_stats(r) for r in rec]
    return {k: np.array([row[k] for row in rows], dtype=np.int64 if k.startswith("n_") else np.float64) for k in _KEYS}


def _binary(result, reference, voxelspacing, distances):
    rec, _ = _run(result, reference, None, voxelspacing, binary=True, distances=distances)
    return _stats(rec[0], distances)


def _need_both(s):
    if s["n_a"] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if s["n_b"] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")


def dc(result, reference, voxelspacing=None, connectivity=1):
    """Dice coefficient 2|A&B| / (|A| + |B|); 0.0 when both are empty.  (voxelspacing / connectivity: signature only.)"""
    _check_connectivity(connectivity)
    if voxelspacing is not None:
        _spacing(voxelspacing, _validate(result, reference))
    return _binary(result, reference, None, False)["dc"]


def jc(result, reference, voxelspacing=None, connectivity=1):
    """Jaccard coefficient |A&B| / |A|B|; ZeroDivisionError when both are empty."""
    _check_connectivity(connectivity)
    if voxelspacing is not None:
        _spacing(voxelspacing, _validate(result, reference))
    s = _binary(result, reference, None, False)
    if s["n_a"] + s["n_b"] - s["n_ab"] == 0:
        raise ZeroDivisionError("jc: both masks are empty")
    return s["jc"]


def ravd(result, reference, voxelspacing=None, connectivity=1):
    """Relative absolute volume difference (|A| - |B|) / |B| (signed, as medpy); RuntimeError when B is empty."""
    _check_connectivity(connectivity)
    if voxelspacing is not None:
        _spacing(voxelspacing, _validate(result, reference))
    s = _binary(result, reference, None, False)
    if s["n_b"] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return s["ravd"]


def _surface(name, result, reference, voxelspacing, connectivity):
    _check_connectivity(connectivity)
    s = _binary(result, reference, voxelspacing, True)
    _need_both(s)
    return s[name]


def hd(result, reference, voxelspacing=None, connectivity=1):
    """Hausdorff distance: max over both directions of the surface distances."""
    return _surface("hd", result, reference, voxelspacing, connectivity)


def hd95(result, reference, voxelspacing=None, connectivity=1):
    """95th percentile (numpy 'linear') of the surface distances of both directions."""
    return _surface("hd95", result, reference, voxelspacing, connectivity)


def asd(result, reference, voxelspacing=None, connectivity=1):
    """Average surface distance from the border of `result` to the border of `reference`."""
    return _surface("asd", result, reference, voxelspacing, connectivity)


def assd(result, reference, voxelspacing=None, connectivity=1):
    """Average symmetric surface distance: the mean of asd(A, B) and asd(B, A)."""
    return _surface("assd", result, reference, voxelspacing, connectivity)


def binary_all(result, reference, voxelspacing=None):
    """Every statistic of one binary pair from one launch chain (dict as one row of per_class; NaN where medpy would raise)."""
    return _binary(result, reference, voxelspacing, True)


binary = types.SimpleNamespace(dc=dc, jc=jc, ravd=ravd, hd=hd, hd95=hd95, asd=asd, assd=assd)
