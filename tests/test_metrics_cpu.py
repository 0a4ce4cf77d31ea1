"""CPU checks of the segmentation metrics: the scipy restatement (tests/metrics_restatement.py) against hand-derived values, the
ctypes mirror of the new chap_metrics structs against the header, and the argument errors raised before anything is launched."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import metrics_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_two_voxels_3_4_5():
    a = np.zeros((8, 8), bool)
    b = np.zeros((8, 8), bool)
    a[1, 1] = True
    b[4, 5] = True                       # offset (3, 4): distance 5 both ways
    assert R.hd(a, b) == 5.0 and R.hd95(a, b) == 5.0 and R.asd(a, b) == 5.0 and R.assd(a, b) == 5.0
    assert R.dc(a, b) == 0.0 and R.jc(a, b) == 0.0 and R.ravd(a, b) == 0.0
    # spacing (2, 1): offset (3*2, 4) -> sqrt(52)
    assert R.hd(a, b, voxelspacing=(2.0, 1.0)) == pytest.approx(math.sqrt(52.0), rel=1e-15)


def test_restatement_cube_and_shifted_copy():
    a = np.zeros((20, 20, 20), bool)
    a[5:11, 5:11, 5:11] = True           # 6^3 cube
    b = np.roll(a, 3, axis=2)            # shifted by 3 along the last axis
    assert R.hd(a, b) == 3.0
    inter = 6 * 6 * 3
    assert R.dc(a, b) == 2.0 * inter / (2 * 216)
    assert R.jc(a, b) == inter / (2 * 216 - inter)
    assert R.ravd(a, b) == 0.0
    # symmetric shift: asd(A, B) == asd(B, A)
    assert R.asd(a, b) == pytest.approx(R.asd(b, a), rel=1e-15)
    assert 0 < R.hd95(a, b) <= 3.0


def test_restatement_anisotropic_spacing():
    a = np.zeros((10, 10, 10), bool)
    b = np.zeros((10, 10, 10), bool)
    a[2, 3, 4] = True
    b[5, 3, 6] = True                    # offset (3, 0, 2)
    sp = (2.5, 0.625, 0.625)
    want = math.sqrt((3 * 2.5) ** 2 + (2 * 0.625) ** 2)
    assert R.hd(a, b, voxelspacing=sp) == pytest.approx(want, rel=1e-15)
    assert R.asd(a, b, voxelspacing=sp) == pytest.approx(want, rel=1e-15)


def test_restatement_border_2d_vs_3d():
    x = np.zeros((40, 40), bool)
    x[10:30, 10:30] = True
    b2 = R.border(x)
    assert b2.sum() == 4 * 20 - 4        # the ring of the square
    assert R.border(x[None]).sum() == x.sum()     # [1, 40, 40]: every voxel touches the array's z faces


def test_restatement_errors():
    z = np.zeros((5, 5), bool)
    o = np.zeros((5, 5), bool)
    o[2, 2] = True
    assert R.dc(z, z) == 0.0
    with pytest.raises(ZeroDivisionError):
        R.jc(z, z)
    with pytest.raises(RuntimeError):
        R.ravd(o, z)
    for f in (R.hd, R.hd95, R.asd, R.assd):
        with pytest.raises(RuntimeError):
            f(z, o)
        with pytest.raises(RuntimeError):
            f(o, z)


def test_metrics_struct_sizes_match_header(tmp_path):
    from chap_amd import _lib
    pairs = {"chap_metrics_params": _lib.MetricsParams, "chap_metric_result": _lib.MetricResult}
    c = tmp_path / "sz.c"
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in pairs)
    body += 'printf("max_axis %d\\n", CHAP_METRICS_MAX_AXIS);\n'
    body += 'printf("off_spacing %zu\\n", offsetof(chap_metrics_params, spacing));\n'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for name, st in pairs.items():
        assert int(sizes[name]) == ctypes.sizeof(st), (name, sizes[name], ctypes.sizeof(st))
    assert int(sizes["max_axis"]) == _lib.METRICS_MAX_AXIS
    assert int(sizes["off_spacing"]) == _lib.MetricsParams.spacing.offset


def test_argument_errors_before_launch():
    from chap_amd import metrics
    a = np.zeros((4, 5), np.uint8)
    with pytest.raises(ValueError, match="same shape"):
        metrics.hd95(a, np.zeros((5, 4), np.uint8))
    with pytest.raises(ValueError, match="2D and 3D"):
        metrics.hd95(np.zeros(7, np.uint8), np.zeros(7, np.uint8))
    with pytest.raises(ValueError, match="2D and 3D"):
        metrics.dc(np.zeros((2, 2, 2, 2), np.uint8), np.zeros((2, 2, 2, 2), np.uint8))
    for sp in ((1.0, 2.0, 3.0), (1.0, -1.0), (0.0, 1.0), (float("nan"), 1.0), 0.0):
        with pytest.raises(ValueError, match="voxelspacing"):
            metrics.hd(a, a, voxelspacing=sp)
    with pytest.raises(NotImplementedError):
        metrics.asd(a, a, connectivity=2)
    with pytest.raises(ValueError, match="axis longer"):
        metrics.hd95(np.zeros((2, 5000), np.uint8), np.zeros((2, 5000), np.uint8))
    with pytest.raises(ValueError, match="classes"):
        metrics.per_class(a, a, [1, 1])
    with pytest.raises(ValueError, match="classes"):
        metrics.per_class(a, a, list(range(300)))
    assert metrics.binary.hd95 is metrics.hd95 and set(vars(metrics.binary)) == {"dc", "jc", "ravd", "hd", "hd95", "asd", "assd"}
