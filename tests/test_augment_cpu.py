"""CPU checks of the device-resident data layer (DESIGN.md "Data layer"): the index plan of tests/augment_restatement.py -- the
arithmetic chap_augment2d performs -- against the scipy calls of the contract, pixel for pixel; the two-stream sampler and the
augmentation draws of chap_amd.data; the ABI boundary of the two new entry points; the host side of the stores."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import augment_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 216), (216, 256), (224, 154), (37, 29), (256, 256)]
ALL_DRAWS = ([dict(mode=R.MODE_ROTATE, k=0, axis=0, angle=a) for a in range(-20, 20)]
             + [dict(mode=R.MODE_ROTFLIP, k=k, axis=ax, angle=0) for k in range(4) for ax in range(2)]
             + [dict(mode=R.MODE_NONE, k=0, axis=0, angle=0)])


def _distinct(shape):
    """An image whose pixels are all distinct and non-zero (a wrong source index or a wrong inside test shows in the value) and a label
    map without zeros that changes from pixel to pixel."""
    n = shape[0] * shape[1]
    return (np.arange(n, dtype=np.float32) + 1).reshape(shape), (np.arange(n) % 251 + 1).astype(np.uint8).reshape(shape)


@pytest.mark.parametrize("out", [(256, 256), (64, 64)])
@pytest.mark.parametrize("shape", SHAPES)
def test_index_plan_equals_scipy(shape, out):
    """ndimage.rotate(order=0, reshape=False) / rot90 + flip, then ndimage.zoom(order=0), against one gather from the plain-IEEE index
    plan (separate multiply and add): all 40 angles, all 8 (k, axis), and the identity.  Required: zero differing pixels."""
    img, lab = _distinct(shape)
    assert len(ALL_DRAWS) == 49
    for d in ALL_DRAWS:
        a_img, a_lab = R.augment_scipy(img, lab, d, out)
        b_img, b_lab = R.augment_plan(img, lab, d, out)
        assert a_img.shape == b_img.shape == (1,) + out and a_img.dtype == b_img.dtype == np.float32
        assert a_lab.shape == b_lab.shape == out and a_lab.dtype == b_lab.dtype == np.int64
        assert int((a_img != b_img).sum()) == 0 and int((a_lab != b_lab).sum()) == 0, (shape, out, d)
    # a rotation leaves corners outside, the other modes leave nothing outside: the constant 0 is exercised and is not everywhere
    assert (R.augment_plan(img, lab, ALL_DRAWS[0], out)[0] == 0).any() and (R.augment_plan(img, lab, ALL_DRAWS[-1], out)[0] != 0).all()


def test_rotflip_of_a_non_square_slice_swaps_the_zoomed_shape():
    img, lab = _distinct((6, 4))
    d = dict(mode=R.MODE_ROTFLIP, k=1, axis=0, angle=0)
    a = R.augment_scipy(img, lab, d, (4, 6))           # (x', y') = (4, 6): both zoom factors are 1
    assert np.array_equal(a[0][0], np.flip(np.rot90(img, 1), 0)) and np.array_equal(R.augment_plan(img, lab, d, (4, 6))[0], a[0])


def test_augment3d_restatement_crops_so_that_the_output_has_the_patch_shape():
    vol = np.arange(10 * 12 * 9, dtype=np.float32).reshape(10, 12, 9)
    lab = (np.arange(10 * 12 * 9) % 3).astype(np.uint8).reshape(10, 12, 9)
    for k in range(4):
        for axis in range(2):
            im, lb = R.augment3d_numpy(vol, lab, dict(corner=(1, 2, 3), k=k, axis=axis), (6, 4, 5))
            assert im.shape == (1, 6, 4, 5) and lb.shape == (6, 4, 5) and lb.dtype == np.int64
    im, _ = R.augment3d_numpy(vol, lab, dict(corner=(1, 2, 3), k=0, axis=1), (6, 4, 5))
    assert np.array_equal(im[0], vol[1:7, 2:6, 3:8][:, ::-1])


# ---------------------------------------------------------------------------------------------------- sampler and draws
def test_two_stream_sampler():
    from chap_amd.data import TwoStreamBatchSampler
    lab, unl = list(range(0, 50)), list(range(50, 173))
    s = TwoStreamBatchSampler(lab, unl, 24, 12, seed=3)
    assert len(s) == 50 // 12 == 4
    for epoch in range(3):
        batches = list(s)
        assert len(batches) == len(s)
        seen = []
        for b in batches:
            assert len(b) == 24 and all(i in range(0, 50) for i in b[:12]) and all(i in range(50, 173) for i in b[12:])
            seen += b[:12]
        assert len(set(seen)) == len(seen)                       # one epoch visits a labelled index at most once
    a, b = TwoStreamBatchSampler(lab, unl, 24, 12, seed=3), TwoStreamBatchSampler(lab, unl, 24, 12, seed=3)
    assert [list(a), list(a)] == [list(b), list(b)]             # same seed, same sequence (over epochs)
    assert list(TwoStreamBatchSampler(lab, unl, 24, 12, seed=4)) != list(TwoStreamBatchSampler(lab, unl, 24, 12, seed=3))
    # the unlabelled stream is endless: every index comes round before any comes twice
    s = TwoStreamBatchSampler(list(range(8)), list(range(8, 14)), 4, 2, seed=0)
    unl_seen = [i for _ in range(3) for b in s for i in b[2:]]
    assert sorted(unl_seen[:6]) == list(range(8, 14)) and sorted(unl_seen[6:12]) == list(range(8, 14))
    # first epoch of the restatement's sampler from the same generator state
    assert list(TwoStreamBatchSampler(lab, unl, 24, 12, seed=11)) == R.two_stream_batches(lab, unl, 24, 12, np.random.default_rng(11))
    with pytest.raises(ValueError):
        TwoStreamBatchSampler(list(range(3)), unl, 24, 12)


def test_augmentation_draws():
    from chap_amd import data
    rng = np.random.default_rng(2024)
    n = 4000
    draws = [data.draw_sample(rng) for _ in range(n)]
    rng2 = np.random.default_rng(2024)
    assert draws == [R.draw_sample(rng2) for _ in range(n)]     # the restatement reads the same stream the same way
    counts = [sum(d["mode"] == m for d in draws) for m in (data.MODE_ROTFLIP, data.MODE_ROTATE, data.MODE_NONE)]
    for c, p in zip(counts, (0.5, 0.25, 0.25)):
        assert abs(c - n * p) <= 4.0 * np.sqrt(n * p * (1 - p)), (counts, p)
    assert {(d["k"], d["axis"]) for d in draws if d["mode"] == data.MODE_ROTFLIP} == {(k, a) for k in range(4) for a in range(2)}
    assert {d["angle"] for d in draws if d["mode"] == data.MODE_ROTATE} == set(range(-20, 20))
    for angle, shape in ((-20, (256, 216)), (7, (37, 29)), (0, (5, 5))):
        m, off = data.rotate_params(angle, shape)
        m2, off2 = R.rotate_params(angle, shape)
        assert np.array_equal(m, m2) and np.array_equal(off, off2) and m.dtype == off.dtype == np.float64


# ---------------------------------------------------------------------------------------------------- ABI boundary
def test_new_entry_points_load_and_bind(tmp_path):
    from chap_amd import _lib
    for name, st in (("chap_augment2d", _lib.Augment2dParams), ("chap_augment3d", _lib.Augment3dParams)):
        assert _lib._SIGS[name] is st
        fn = _lib._fn(name)
        assert fn.restype is ctypes.c_int
        with pytest.raises(_lib.ChapError, match="null"):       # argument check, no launch
            _lib.call(name, st(), 0)
    assert _lib.lib().chap_abi_version() == _lib.ABI_VERSION == 9
    pairs = {"chap_augment2d_record": _lib.Augment2dRecord, "chap_augment2d_params": _lib.Augment2dParams,
             "chap_augment3d_record": _lib.Augment3dRecord, "chap_augment3d_params": _lib.Augment3dParams}
    c = tmp_path / "sz.c"
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in pairs)
    body += 'printf("modes %d\\n", CHAP_AUG_NONE + 10 * CHAP_AUG_ROTFLIP + 100 * CHAP_AUG_ROTATE);\n'
    c.write_text('#include <stdio.h>\n#include "chap_hip.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    sizes = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for name, st in pairs.items():
        assert int(sizes[name]) == ctypes.sizeof(st), (name, sizes[name], ctypes.sizeof(st))
    assert int(sizes["modes"]) == _lib.AUG_NONE + 10 * _lib.AUG_ROTFLIP + 100 * _lib.AUG_ROTATE


# ---------------------------------------------------------------------------------------------------- stores (host side)
def test_store_layout_and_argument_checks():
    from chap_amd.data import DeviceLoader, SliceStore, VolumeStore
    rng = np.random.default_rng(0)
    shapes = [(5, 7), (3, 3), (8, 2)]
    images = [rng.random(s) for s in shapes]                    # float64 in, fp32 stored
    labels = [rng.integers(0, 4, s) for s in shapes]
    st = SliceStore(images, labels, device="cpu")
    assert len(st) == 3 and st.offsets.tolist() == [0, 35, 44] and st.shapes.tolist() == [list(s) for s in shapes]
    assert st.images.dtype.is_floating_point and st.images.numel() == st.labels.numel() == 60
    assert np.array_equal(st.images[35:44].numpy().reshape(3, 3), images[1].astype(np.float32))
    assert np.array_equal(st.labels[44:].numpy().reshape(8, 2), labels[2].astype(np.uint8))
    with pytest.raises(ValueError, match="255"):
        SliceStore(images, [l + 300 for l in labels], device="cpu")
    with pytest.raises(ValueError, match="shapes"):
        SliceStore(images, [labels[0], labels[1], labels[2].T], device="cpu")
    with pytest.raises(ValueError, match="2D"):
        SliceStore([np.zeros((2, 2, 2))], [np.zeros((2, 2, 2), dtype=np.uint8)], device="cpu")
    vs = VolumeStore([np.zeros((8, 12, 10)), np.zeros((12, 12, 10))], [np.zeros((8, 12, 10), dtype=np.uint8)] * 1 + [np.zeros((12, 12, 10), dtype=np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="smaller than the crop"):      # 8 < max(P0, P1): an odd number of quarter turns would leave the volume
        DeviceLoader(vs, [0], [1], 2, 1, (8, 12, 10))
    with pytest.raises(ValueError, match="output_size"):
        DeviceLoader(st, [0], [1], 2, 1, (8, 8, 8))
    with pytest.raises(IndexError):
        DeviceLoader(st, [0], [3], 2, 1, (8, 8))


def _have_h5py():
    try:
        import h5py  # noqa: F401
        return True
    except ImportError:
        return False


def test_from_h5_dir_without_h5py_says_so(tmp_path):
    if _have_h5py():
        pytest.skip("h5py is importable: the round trip below covers from_h5_dir")
    from chap_amd.data import SliceStore
    with pytest.raises(ImportError, match="h5py"):
        SliceStore.from_h5_dir(str(tmp_path), "train", device="cpu")


@pytest.mark.skipif(not _have_h5py(), reason="h5py is not importable here: from_h5_dir has nothing to read the files with")
def test_from_h5_dir_round_trip(tmp_path):
    import h5py
    from chap_amd.data import SliceStore
    rng = np.random.default_rng(1)
    os.makedirs(tmp_path / "data" / "slices")
    cases, images, labels = [], [], []
    for n, shape in enumerate([(16, 12), (9, 20), (16, 16)]):
        name = "patient%03d_frame01_slice_%d" % (n + 1, n)
        images.append(rng.random(shape).astype(np.float32))
        labels.append(rng.integers(0, 4, shape).astype(np.uint8))
        with h5py.File(tmp_path / "data" / "slices" / (name + ".h5"), "w") as h:
            h.create_dataset("image", data=images[-1])
            h.create_dataset("label", data=labels[-1])
        cases.append(name)
    (tmp_path / "train_slices.list").write_text("\n".join(cases) + "\n")
    st = SliceStore.from_h5_dir(str(tmp_path), "train", device="cpu")
    assert st.cases == cases and st.shapes.tolist() == [list(i.shape) for i in images]
    for o, im, lb in zip(st.offsets, images, labels):
        assert np.array_equal(st.images[o:o + im.size].numpy().reshape(im.shape), im)
        assert np.array_equal(st.labels[o:o + lb.size].numpy().reshape(lb.shape), lb)
