"""chap_window_gather, chap_window_accumulate_heads and chap_augment3d_padded on the GPU, per element: the copies bit for bit against
numpy (np.pad + slicing; np.pad + crop + rot90 + flip fed the loader's own draws), the two-head score against the fp64 restatement and
bound of tests/la_ref.py (derived there from the kernels' arithmetic, before the first run), the one-head score bit for bit against
chap_window_accumulate.  Outputs are poisoned with NaN before a call.  Run with -s for the worst err / bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import ops
from chap_amd.data import DeviceLoader, VolumeStore
from chap_amd.test_3d_patch import window_origins
from tests import augment_restatement as R
from tests import kernel_ref as kr
from tests import la_ref as LR

DEV = torch.device("cuda", 0)
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("patch", [(12, 10, 8), (12, 10, 7)])
@pytest.mark.parametrize("vol", [(20, 18, 14), (9, 18, 5)])
def test_window_gather_is_np_pad_and_slicing(vol, patch):
    """Every window of strides 5 / 3 (the last one of an axis clamped; (9, 18, 5) is padded in x and z), in launches of 4: bitwise the
    slices of the np.pad-ded volume; the NaN canary behind the output stays.  (12, 10, 7): the scalar tail; an output that is not
    16-byte aligned: scalar stores for pd % 4 == 0 too.  An origin outside the padded volume reads zeros."""
    image = np.random.default_rng(2).random(vol, dtype=np.float32) + 0.5
    lo, hi, padded, origins = window_origins(vol, patch, 5, 3)
    assert any(o[a] == padded[a] - patch[a] and o[a] % (5, 5, 3)[a] for o in origins for a in range(3))      # a clamped window
    ref_vol = np.pad(image, list(zip(lo, hi)), mode="constant", constant_values=0)
    assert ref_vol.shape == padded
    ref = np.stack([ref_vol[x:x + patch[0], y:y + patch[1], z:z + patch[2]] for x, y, z in origins])[:, None]
    v = torch.from_numpy(image).to(DEV)
    table = torch.tensor(origins, dtype=torch.int32, device=DEV)
    pvox = patch[0] * patch[1] * patch[2]
    for shift in (0, 1):                                         # 1: the output starts 4 bytes past a 16-byte boundary
        got = []
        for k0 in range(0, len(origins), 4):
            og = table[k0:k0 + 4]
            buf = torch.full((shift + og.shape[0] * pvox + 8,), NAN, device=DEV)
            out = buf[shift:shift + og.shape[0] * pvox].view(og.shape[0], 1, *patch)
            assert out.data_ptr() % 16 == 4 * shift
            ops.window_gather(v, og, patch, lo, out=out)
            assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + og.shape[0] * pvox:]).all())
            got.append(out.cpu())
        got = torch.cat(got)
        assert got.shape == ref.shape and torch.equal(_bits(got), _bits(torch.from_numpy(ref)))
    assert torch.equal(ops.window_gather(v, table[:3], patch, lo).cpu(), torch.from_numpy(ref[:3]))          # the allocating form
    far = torch.tensor([[-40, 0, 0], [0, 100, 0], [lo[0] - 3, lo[1] + 2, lo[2] - 1]], dtype=torch.int32, device=DEV)
    out = ops.window_gather(v, far, patch, lo).cpu().numpy()
    big = np.pad(image, [(50, 50), (50, 120), (50, 50)])
    assert not out[:2].any() and np.array_equal(out[2, 0], big[47:47 + patch[0], 52:52 + patch[1], 49:49 + patch[2]])


# ---------------------------------------------------------------------------------------------------- accumulate, one and two heads
@pytest.mark.parametrize("C", [2, 4])
def test_window_accumulate_heads(C):
    """kernel_ref.WINDOW_CASE: two launches of three patches into a nonzero prior, an uncovered corner.  nheads 1: the bits of
    chap_window_accumulate.  nheads 2: |got - ref| <= score_b per element (la_ref: per patch (e_p1 + e_p2) / 2 + U32 pbar, then the
    sum rule), cnt exact, uncovered voxels untouched, labels after finalize equal outside `near`."""
    case = kr.WINDOW_CASE
    l1, s0, c0 = kr.window_inputs(C, **case)
    l2, _, _ = kr.window_inputs(C, seed=11, **case)
    assert not torch.equal(l1[0], l2[0])
    orgs = [torch.tensor(o, dtype=torch.int32, device=DEV) for o in case["calls"]]
    # one head
    sa, ca, sb, cb = s0.to(DEV), c0.to(DEV), s0.to(DEV), c0.to(DEV)
    for lg, og in zip(l1, orgs):
        ops.window_accumulate(lg.to(DEV), og, sa, ca)
        ops.window_accumulate_heads([lg.to(DEV)], og, sb, cb)
        assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(ca, cb)
    ops.window_accumulate_heads(l1[0].to(DEV), orgs[0], sb, cb)       # a bare tensor is one head
    ops.window_accumulate(l1[0].to(DEV), orgs[0], sa, ca)
    assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(ca, cb)
    # two heads
    runs = []
    ref_s, ref_b, ref_c = s0.double(), torch.zeros_like(s0).double(), c0.double()      # the restatement carried over both launches, in fp64
    for rep in range(2):
        score, cnt = s0.to(DEV), c0.to(DEV)
        for a, b, og, org in zip(l1, l2, orgs, case["calls"]):
            before_s, before_c = score.clone(), cnt.clone()
            ops.window_accumulate_heads([a.to(DEV), b.to(DEV)], og, score, cnt)
            if rep == 0:
                r = LR.window_accumulate_heads_ref([a, b], org, before_s.cpu(), before_c.cpu())
                worst = kr.check("heads C=%d score" % C, score.cpu(), r["score"], r["score_b"], "cxyz")
                print("  window_accumulate_heads C=%d: worst err/bound %.3f" % (C, worst))
                assert torch.equal(cnt.cpu(), r["cnt"].float())
                unc = ~r["covered"]
                assert bool(unc.any()) and torch.equal(_bits(score.cpu()[:, unc]), _bits(before_s.cpu()[:, unc])) and torch.equal(cnt.cpu()[unc], before_c.cpu()[unc])
                rc = LR.window_accumulate_heads_ref([a, b], org, ref_s, ref_c)
                ref_s, ref_b, ref_c = rc["score"], ref_b + rc["score_b"], rc["cnt"]
        acc_s, acc_c = score.clone(), cnt.clone()
        label = ops.window_finalize(score, cnt)
        runs.append((acc_s, acc_c, label))
    for t0, t1 in zip(*runs):                                    # no atomics: the same bits twice
        assert torch.equal(_bits(t0.float()), _bits(t1.float()))
    acc_s, acc_c, label = (t.cpu() for t in runs[0])
    kr.check("heads C=%d score, both launches" % C, acc_s, ref_s, ref_b, "cxyz")
    assert torch.equal(acc_c.double(), ref_c)
    fin = kr.window_finalize_ref(ref_s, ref_c, ref_b)            # labels of the independent fp64 map, the bound carried over both launches
    share = float(fin["near"].double().mean())
    assert share <= LR.NEAR_TIE_CAP
    ok = ~fin["near"] & ~fin["empty"]
    assert torch.equal(label.long()[ok], fin["label"][ok]) and not bool(label[fin["empty"]].any())
    # the mean of two equal heads is that head: fl(fl(p + p) / 2) = p
    sa, ca, sb, cb = s0.to(DEV), c0.to(DEV), s0.to(DEV), c0.to(DEV)
    ops.window_accumulate(l1[0].to(DEV), orgs[0], sa, ca)
    ops.window_accumulate_heads([l1[0].to(DEV), l1[0].to(DEV).clone()], orgs[0], sb, cb)
    assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(ca, cb)


def test_window_accumulate_heads_argument_checks():
    from chap_amd import _lib
    lg = torch.zeros(1, 2, 4, 4, 4, device=DEV)
    og = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    score, cnt = torch.zeros(2, 4, 4, 4, device=DEV), torch.zeros(4, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.window_accumulate_heads([lg, lg, lg], og, score, cnt)
    with pytest.raises(_lib.ChapError, match="patch larger"):
        ops.window_accumulate_heads([lg], og, torch.zeros(2, 3, 4, 4, device=DEV), torch.zeros(3, 4, 4, device=DEV))
    with pytest.raises(_lib.ChapError):
        ops.window_accumulate_heads([torch.zeros(1, 9, 4, 4, 4, device=DEV)], og, torch.zeros(9, 4, 4, 4, device=DEV), cnt)      # C > 8


# ---------------------------------------------------------------------------------------------------- padded augment
PAD_SHAPES = [(20, 30, 12), (40, 40, 36), (24, 24, 24), (10, 50, 30), (44, 44, 44), (33, 35, 31)]


def _volumes(shapes, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.random(s, dtype=np.float32) + 0.5 for s in shapes], [rng.integers(1, 3, s).astype(np.uint8) for s in shapes]      # no zeros: the padding shows


def test_augment3d_padded_bit_identical_to_numpy():
    """Six volumes, three of them smaller than some crop; patches (24, 24, 24), (32, 24, 20) and (16, 12, 10) (last side % 4 != 0:
    scalar stores); 10 batches each against np.pad by the drawn pad + crop + rot90 + flip, bit for bit."""
    images, labels = _volumes(PAD_SHAPES)
    store = VolumeStore(images, labels, DEV)
    seen_all = []
    for patch in ((24, 24, 24), (32, 24, 20), (16, 12, 10)):
        loader = DeviceLoader(store, range(3), range(3, 6), 4, 2, patch, seed=1, pad=True)
        img = torch.empty(4, 1, *patch, device=DEV)
        lab = torch.empty(4, *patch, dtype=torch.int64, device=DEV)
        seen = []
        for n in range(10):
            img.fill_(-1.0), lab.fill_(-1)
            loader.next_into(img, lab)
            ref_i, ref_l = LR.batch3d_padded_from_draws(images, labels, loader.last_draws, patch)
            assert torch.equal(_bits(img.cpu()), _bits(torch.from_numpy(ref_i))) and torch.equal(lab.cpu(), torch.from_numpy(ref_l)), (patch, n)
            seen += loader.last_draws
        assert {(d["k"], d["axis"]) for d in seen} == {(k, a) for k in range(4) for a in range(2)}, patch
        assert any(any(d["pad"]) for d in seen) and any(not any(d["pad"]) for d in seen), patch
        batch = next(iter(loader))                               # fresh tensors, uint8 labels below
        ref_i, ref_l = LR.batch3d_padded_from_draws(images, labels, loader.last_draws, patch)
        assert torch.equal(batch["image"].cpu(), torch.from_numpy(ref_i)) and torch.equal(batch["label"].cpu(), torch.from_numpy(ref_l))
        lab8 = torch.empty(4, *patch, dtype=torch.uint8, device=DEV)
        loader.next_into(img, lab8)
        ref_i, ref_l = LR.batch3d_padded_from_draws(images, labels, loader.last_draws, patch)
        assert torch.equal(img.cpu(), torch.from_numpy(ref_i)) and torch.equal(lab8.cpu(), torch.from_numpy(ref_l.astype(np.uint8)))
        seen_all += seen
        with pytest.raises(ValueError, match="smaller than the crop"):
            DeviceLoader(store, range(3), range(3, 6), 4, 2, patch, seed=1)
    for a in range(3):
        assert any(d["pad"][a] > 0 for d in seen_all), a         # a padded sample for every axis
    assert any((np.asarray(d["pad"]) > 0).all() for d in seen_all)


def test_augment3d_padded_equals_augment3d_without_padding():
    """Volumes larger than every crop on every axis: pad=True and pad=False draw the same and write the same bits."""
    shapes = [(40, 40, 36), (48, 40, 40), (40, 52, 44), (44, 44, 44), (33, 35, 31), (34, 33, 25)]
    images, labels = _volumes(shapes, seed=4)
    store = VolumeStore(images, labels, DEV)
    for patch in ((24, 24, 24), (32, 24, 20), (16, 12, 10)):
        a = DeviceLoader(store, range(3), range(3, 6), 4, 2, patch, seed=5)
        b = DeviceLoader(store, range(3), range(3, 6), 4, 2, patch, seed=5, pad=True)
        for n in range(4):
            ba, bb = next(iter(a)), next(iter(b))
            assert a.last_draws == [{k: v for k, v in d.items() if k != "pad"} for d in b.last_draws]
            assert all(d["pad"] == (0, 0, 0) for d in b.last_draws)
            assert torch.equal(_bits(ba["image"]), _bits(bb["image"])) and torch.equal(ba["label"], bb["label"])
            ref_i, ref_l = R.batch3d_from_draws(images, labels, a.last_draws, patch)
            assert torch.equal(ba["image"].cpu(), torch.from_numpy(ref_i)) and torch.equal(ba["label"].cpu(), torch.from_numpy(ref_l))


def test_augment3d_padded_zero_fills_a_bad_record():
    """A record that breaks the host's guarantee (corner + crop beyond shape + 2 pad; an offset that leaves the store; a negative pad) gives
    zeros, never a read outside the store."""
    import ctypes
    from chap_amd import _lib
    images, labels = _volumes([(12, 12, 12)], seed=6)
    store = VolumeStore(images, labels, DEV)
    recs = (_lib.Augment3dPadRecord * 4)()
    for r, (off, corner, pad) in zip(recs, ((0, (2, 2, 2), (1, 1, 1)), (0, (7, 0, 0), (1, 1, 1)), (8, (0, 0, 0), (1, 1, 1)), (0, (0, 0, 0), (-1, 2, 2)))):
        r.offset, r.k, r.axis = off, 0, 1
        for a in range(3):
            r.shape[a], r.corner[a], r.pad[a] = 12, corner[a], pad[a]
    dev = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)
    img = torch.full((4, 1, 8, 8, 8), NAN, device=DEV)
    lab = torch.full((4, 8, 8, 8), -1, dtype=torch.int64, device=DEV)
    ops.augment3d_padded(store.images, store.labels, dev, img, lab)
    ref_i, ref_l = LR.augment3d_padded_numpy(images[0], labels[0], dict(corner=(2, 2, 2), pad=(1, 1, 1), k=0, axis=1), (8, 8, 8))
    assert torch.equal(img[0].cpu(), torch.from_numpy(ref_i)) and torch.equal(lab[0].cpu(), torch.from_numpy(ref_l))
    assert not bool(img[1:].any()) and not bool(lab[1:].any())
    assert ctypes.sizeof(recs) == 4 * 56
