"""CPU restatement of the segmentation metrics, written from their definitions with scipy (no medpy): the yardstick of
chap_amd.metrics.  A helper module, not collected by pytest.

    border(X) = X & ~binary_erosion(X, generate_binary_structure(ndim, 1), iterations=1)      (border_value 0)
    sds(A, B) = distance_transform_edt(~border(B), sampling=voxelspacing)[border(A)]
"""
import numpy as np
from scipy import ndimage


def _masks(result, reference):
    a = np.atleast_1d(np.asarray(result).astype(bool))
    b = np.atleast_1d(np.asarray(reference).astype(bool))
    if a.shape != b.shape:
        raise ValueError("shape mismatch")
    return a, b


def border(x):
    x = np.asarray(x).astype(bool)
    fp = ndimage.generate_binary_structure(x.ndim, 1)
    return x & ~ndimage.binary_erosion(x, structure=fp, iterations=1)


def sds(a, b, voxelspacing=None, connectivity=1):
    if connectivity != 1:
        raise NotImplementedError
    a, b = _masks(a, b)
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    dt = ndimage.distance_transform_edt(~border(b), sampling=voxelspacing)
    return dt[border(a)]


def dc(result, reference):
    a, b = _masks(result, reference)
    inter = np.count_nonzero(a & b)
    size = np.count_nonzero(a) + np.count_nonzero(b)
    return 2.0 * inter / float(size) if size else 0.0


def jc(result, reference):
    a, b = _masks(result, reference)
    return float(np.count_nonzero(a & b)) / float(np.count_nonzero(a | b))       # ZeroDivisionError when both are empty


def ravd(result, reference):
    a, b = _masks(result, reference)
    va, vb = np.count_nonzero(a), np.count_nonzero(b)
    if vb == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return (va - vb) / float(vb)


def hd(result, reference, voxelspacing=None, connectivity=1):
    return max(sds(result, reference, voxelspacing, connectivity).max(), sds(reference, result, voxelspacing, connectivity).max())


def hd95(result, reference, voxelspacing=None, connectivity=1):
    return np.percentile(np.hstack((sds(result, reference, voxelspacing, connectivity),
                                    sds(reference, result, voxelspacing, connectivity))), 95)


def asd(result, reference, voxelspacing=None, connectivity=1):
    return sds(result, reference, voxelspacing, connectivity).mean()


def assd(result, reference, voxelspacing=None, connectivity=1):
    return np.mean((asd(result, reference, voxelspacing, connectivity), asd(reference, result, voxelspacing, connectivity)))


ALL = dict(dc=dc, jc=jc, ravd=ravd, hd=hd, hd95=hd95, asd=asd, assd=assd)
