"""CPU checks of the 3D workflow (DESIGN.md "3D workflow"): the ABI boundary of the three new entry points, the `utils.test_3d_patch`
shim, the origin table of the device-side sliding window against the oracle's loop, the padding rule of DeviceLoader(pad=True) against
a literal RandomCrop restatement, and the near-tie share of the two-head restatement on the inputs the GPU tests use."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kernel_ref as kr
from tests import la_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- ABI boundary
def test_new_structs_match_the_header(tmp_path):
    """sizeof and every field offset of the new structs, from a C program compiled against include/chap_hip.h."""
    from chap_amd import _lib
    pairs = {"chap_window_gather_params": _lib.WindowGatherParams, "chap_window_acc_heads_params": _lib.WindowAccHeadsParams,
             "chap_augment3d_pad_record": _lib.Augment3dPadRecord, "chap_augment3d_pad_params": _lib.Augment3dPadParams}
    body = ""
    for n, st in pairs.items():
        body += 'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n)
        for f in st._fields_:
            body += 'printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f[0], n, f[0])
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, st in pairs.items():
        assert int(got[n]) == ctypes.sizeof(st), (n, got[n], ctypes.sizeof(st))
        for f in st._fields_:
            assert int(got["%s.%s" % (n, f[0])]) == getattr(st, f[0]).offset, (n, f[0])
    assert ctypes.sizeof(_lib.Augment3dPadRecord) == 8 + 4 * 12


def test_new_entry_points_load_and_bind():
    from chap_amd import _lib
    for name, st in (("chap_window_gather", _lib.WindowGatherParams), ("chap_window_accumulate_heads", _lib.WindowAccHeadsParams),
                     ("chap_augment3d_padded", _lib.Augment3dPadParams)):
        assert _lib._SIGS[name] is st
        assert _lib._fn(name).restype is ctypes.c_int
        with pytest.raises(_lib.ChapError):                      # argument check, no launch
            _lib.call(name, st(), 0)
    assert _lib.lib().chap_abi_version() == _lib.ABI_VERSION == 9      # additive: no version change


def test_utils_shim_resolves_the_reference_import():
    """`from utils.test_3d_patch import test_all_case` (code/test_LA.py:5) with chap_amd/shim on the path, in a fresh interpreter."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from utils.test_3d_patch import test_all_case\n"
            "from networks.net_factory_3d import net_factory_3d\n"
            "import chap_amd.test_3d_patch as T\n"
            "assert test_all_case is T.test_all_case\n"
            "import inspect; print(list(inspect.signature(test_all_case).parameters))\n" % (ROOT, os.path.join(ROOT, "chap_amd", "shim")))
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    assert eval(out.strip()) == ["model_name", "num_outputs", "model", "image_list", "num_classes", "patch_size", "stride_xy", "stride_z",
                                 "save_result", "test_save_path", "preproc_fn", "metric_detail", "nms"]


def test_readers_name_the_missing_package(tmp_path):
    from chap_amd import test_3d_patch as T
    from chap_amd.data import VolumeStore
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="h5py.*VolumeStore\\(images, labels\\)"):
            VolumeStore.from_h5_list(str(tmp_path), device="cpu")
        with pytest.raises(ImportError, match="h5py.*array pairs"):
            T._load_case(str(tmp_path / "case.h5"))
    try:
        import nibabel  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="nibabel.*save_result=False"):       # at the start of the call: the model is never touched
            T.test_all_case("m", 1, None, [(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))], 2, save_result=True, test_save_path=str(tmp_path))


def test_from_h5_list_round_trip(tmp_path):
    h5py = pytest.importorskip("h5py")
    from chap_amd.data import VolumeStore
    rng = np.random.default_rng(1)
    cases, images, labels = [], [], []
    for n, shape in enumerate([(8, 6, 5), (7, 9, 4)]):
        name = "CASE%02d" % n
        os.makedirs(tmp_path / "2018LA_Seg_Training Set" / name)
        images.append(rng.random(shape).astype(np.float32))
        labels.append(rng.integers(0, 2, shape).astype(np.uint8))
        with h5py.File(tmp_path / "2018LA_Seg_Training Set" / name / "mri_norm2.h5", "w") as h:
            h.create_dataset("image", data=images[-1])
            h.create_dataset("label", data=labels[-1])
        cases.append(name)
    (tmp_path / "train.list").write_text("\n".join(cases) + "\n")
    st = VolumeStore.from_h5_list(str(tmp_path), device="cpu")
    assert st.cases == cases and st.shapes.tolist() == [list(i.shape) for i in images]
    for o, im in zip(st.offsets, images):
        assert np.array_equal(st.images[o:o + im.size].numpy().reshape(im.shape), im)


# ---------------------------------------------------------------------------------------------------- origin table
@pytest.mark.parametrize("shape", [(21, 40, 13), (30, 45, 24), (16, 32, 16), (15, 33, 17), (17, 31, 16), (40, 70, 33)])
@pytest.mark.parametrize("strides", [(9, 4), (8, 4), (16, 16)])
def test_origin_table_equals_the_oracle_loop(shape, strides):
    """Volumes below, equal to and above the patch (16, 32, 16) on each axis: padding, origins and their order are those of the windows
    oracle.inference.test_single_case cuts (recovered from the patches themselves)."""
    from chap_amd.test_3d_patch import window_origins
    patch = (16, 32, 16)
    lo, hi, padded, origins = window_origins(shape, patch, *strides)
    ref_lo, ref_origins = LR.oracle_origins(shape, patch, *strides)
    assert lo == ref_lo and origins == ref_origins
    assert padded == tuple(max(shape[a], patch[a]) for a in range(3)) and all(lo[a] + hi[a] + shape[a] == padded[a] for a in range(3))
    assert all(0 <= o[a] <= padded[a] - patch[a] for o in origins for a in range(3))
    last = tuple(padded[a] - patch[a] for a in range(3))
    assert origins[0] == (0, 0, 0) and origins[-1] == last                # the clamped last window ends at the end of the volume


# ---------------------------------------------------------------------------------------------------- padded crop
def _store(shapes):
    from chap_amd.data import VolumeStore
    return VolumeStore([np.zeros(s, dtype=np.float32) for s in shapes], [np.zeros(s, dtype=np.uint8) for s in shapes], device="cpu")


def test_pad_rule_is_random_crop():
    """DeviceLoader(pad=True)._draw on a host-resident store against the literal RandomCrop restatement fed the same generator stream:
    shapes with an axis equal to the crop, one below it, crop - shape odd and even, far below and far above; k odd and even."""
    from chap_amd.data import DeviceLoader
    patch = (24, 20, 16)
    shapes = [(24, 20, 16), (23, 19, 15), (20, 24, 16), (19, 25, 17), (17, 14, 9), (18, 15, 10), (40, 40, 40), (25, 25, 17), (24, 50, 50), (60, 21, 16)]
    store = _store(shapes)
    loader = DeviceLoader(store, range(5), range(5, 10), 4, 2, patch, seed=3, pad=True)
    rng = np.random.default_rng([3, 1])
    seen = []
    for n in range(60):
        idxs = [int(i) for i in np.random.default_rng(n).integers(0, len(shapes), 4)]
        recs, draws = loader._draw(idxs)
        for r, d, i in zip(recs, draws, idxs):
            ref = LR.draw3d_padded(rng, shapes[i], patch)
            assert d == dict(index=i, **ref), (n, i, d, ref)
            crop = (patch[1], patch[0], patch[2]) if d["k"] % 2 else patch
            assert d["pad"] == LR.random_crop_pad(shapes[i], crop)
            for a in range(3):
                assert 0 <= d["corner"][a] and d["corner"][a] + crop[a] <= shapes[i][a] + 2 * d["pad"][a]
                want = max((crop[a] - shapes[i][a]) // 2 + 3, 0) if any(shapes[i][b] <= crop[b] for b in range(3)) else 0
                assert d["pad"][a] == want
            assert (r.offset, list(r.shape), list(r.corner), list(r.pad), r.k, r.axis) == \
                (int(store.offsets[i]), list(shapes[i]), list(d["corner"]), list(d["pad"]), d["k"], d["axis"])
            seen.append((i, d["k"] % 2, d["pad"]))
    assert {(i, k) for i, k, _ in seen} == {(i, k) for i in range(len(shapes)) for k in range(2)}          # every shape with k odd and even
    pads = {(i, k): p for i, k, p in seen}
    assert pads[(0, 0)] == (3, 3, 3)                               # shape == crop: padded by 3
    assert pads[(1, 0)] == (3, 3, 3)                               # crop - shape = 1: 1 // 2 + 3
    assert pads[(4, 0)] == (6, 6, 6) and pads[(5, 0)] == (6, 5, 6)  # crop - shape = 7, 6, 7 and 6, 5, 6
    assert pads[(6, 0)] == pads[(6, 1)] == (0, 0, 0)               # larger on every axis: nothing
    assert pads[(7, 0)] == (0, 0, 0) and pads[(7, 1)] == (0, 0, 0)  # (25, 25, 17) > (24, 20, 16) and > (20, 24, 16)
    assert pads[(8, 0)] == (3, 0, 0) and pads[(8, 1)] == (0, 0, 0)  # one axis equal: every axis gets its own (here 0) amount
    assert pads[(9, 0)] == (0, 2, 3) and pads[(9, 1)] == (0, 4, 3)  # (crop - shape) // 2 floors: (20 - 21) // 2 + 3 = 2


def test_pad_false_is_unchanged_and_pad_true_agrees_on_large_volumes():
    from chap_amd.data import DeviceLoader, SliceStore
    shapes = [(30, 28, 20), (26, 26, 18), (40, 31, 17), (25, 29, 22)]
    store = _store(shapes)
    a = DeviceLoader(store, range(2), range(2, 4), 4, 2, (24, 20, 16), seed=9)
    b = DeviceLoader(store, range(2), range(2, 4), 4, 2, (24, 20, 16), seed=9, pad=True)
    for _ in range(20):
        idxs = next(a._endless)
        assert idxs == next(b._endless)
        da, db = a._draw(idxs)[1], b._draw(idxs)[1]
        assert all("pad" not in d for d in da) and all(d["pad"] == (0, 0, 0) for d in db)
        assert da == [{k: v for k, v in d.items() if k != "pad"} for d in db]
    with pytest.raises(ValueError, match="smaller than the crop"):
        DeviceLoader(_store(shapes + [(10, 40, 40)]), range(2), range(2, 5), 4, 2, (24, 20, 16))
    DeviceLoader(_store(shapes + [(10, 40, 40)]), range(2), range(2, 5), 4, 2, (24, 20, 16), pad=True)      # accepted
    with pytest.raises(RuntimeError, match="_draw only"):           # a host-resident store draws, it does not launch
        a.next_into(torch.empty(4, 1, 24, 20, 16), torch.empty(4, 24, 20, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="pad=True"):
        DeviceLoader(SliceStore([np.zeros((8, 8))] * 2, [np.zeros((8, 8), dtype=np.uint8)] * 2, device="cpu"), [0], [1], 2, 1, (8, 8), pad=True)


# ---------------------------------------------------------------------------------------------------- near ties of the restatement
@pytest.mark.parametrize("C", [2, 4])
def test_near_tie_share_of_the_two_head_restatement(C):
    """On the inputs of tests/test_la_kernels_gpu.py (kernel_ref.WINDOW_CASE) and on the window geometry of
    tests/test_la_workflow_gpu.py with randn * 4 logits: the labels the GPU tests compare are decided almost everywhere."""
    logits, s0, c0 = kr.window_inputs(C, **kr.WINDOW_CASE)
    logits2, _, _ = kr.window_inputs(C, seed=11, **kr.WINDOW_CASE)
    score, bound, cnt = s0.double(), torch.zeros_like(s0).double(), c0.double()
    for l1, l2, org in zip(logits, logits2, kr.WINDOW_CASE["calls"]):
        r = LR.window_accumulate_heads_ref([l1, l2], org, score, cnt)
        score, bound, cnt = r["score"], bound + r["score_b"], r["cnt"]
    fin = kr.window_finalize_ref(score, cnt, bound)
    assert float(fin["near"].double().mean()) <= LR.NEAR_TIE_CAP
    shape, patch, strides = (30, 45, 24), (16, 32, 16), (8, 4)
    _, origins = LR.oracle_origins(shape, patch, *strides)
    assert len(origins) == 27
    g = torch.Generator().manual_seed(7)
    batches = [[torch.randn(min(4, 27 - k0), C, *patch, generator=g) * 4 for _ in range(2)] for k0 in range(0, 27, 4)]
    assert batches[-1][0].shape[0] == 3
    r = LR.window_pipeline_ref(shape, patch, *strides, batches, C)
    assert float(r["near"].double().mean()) <= LR.NEAR_TIE_CAP


@pytest.mark.parametrize("case", [((21, 40, 13), (9, 4)), ((30, 45, 24), (8, 4))])
def test_near_tie_share_of_the_stub_pipeline(case):
    """The stub network of the workflow tests, run on the CPU over the oracle's patches: near-tie share of both outputs' restatements."""
    shape, strides = case
    patch = (16, 32, 16)
    image = np.random.default_rng(5).random(shape, dtype=np.float32) + 0.5
    patches = LR.oracle_patches(image, patch, *strides)
    for C in (2, 4):
        net = LR.StubNet(C)
        batches = [list(net(torch.from_numpy(np.stack(patches[k0:k0 + 4]))[:, None])) for k0 in range(0, len(patches), 4)]
        for nheads in (1, 2):
            r = LR.window_pipeline_ref(shape, patch, *strides, [b[:nheads] for b in batches], C)
            assert float(r["near"].double().mean()) <= LR.NEAR_TIE_CAP
    zero = LR.StubNet(2)(torch.zeros(1, 1, 2, 2, 2))
    assert all(int(z.argmax(1).max()) == 0 for z in zero)            # the padding / an all-zero volume: class 0 in both heads
