"""CPU restatements for the 3D workflow (DESIGN.md "3D workflow"): the padded random crop, the two-head sliding-window score with its
error bound, the window loop's patches and origins (through the oracle's line-by-line test_single_case), the largest connected
component with scipy, and the recording stub network of the GPU tests.  A helper module, not collected by pytest.  Builds on
tests/kernel_ref.py (soft-max bound, label rule, finalize), tests/augment_restatement.py (crop + rot90 + flip) and
tests/metrics_restatement.py.

Bounds (written down before the first GPU run, from the arithmetic of the kernels, never fitted):
  one patch, one head    p = softmax_c(z): e_p of kernel_ref.infer_softmax_ref.
  one patch, two heads   v = fl(fl(p1 + p2) / 2): the halving is exact, the add rounds once on (p1 + p2) <= 2 pbar:
                         e = (e_p1 + e_p2) / 2 + U32 pbar,  pbar = (p1 + p2) / 2           (kernel_ref.ensemble_ref, prob_ensemble)
  the sum over patches   one fp32 add per covering patch, each rounding at most U32 |partial sum| <= U32 (|prior| + sum_k pbar_k):
                         score_b = sum_k e_k + n_cover U32 (|prior| + sum_k pbar_k)          (kernel_ref.window_accumulate_ref's rule)
  across batches         the restatement never rounds, so the bound of a map built by several launches is the same expression over
                         ALL its patches: n_cover counts every covering patch, the prior is what the buffers held before the first.
  finalize               kernel_ref.window_finalize_ref: e_score / cnt + U32 |v|; labels compared outside `near`."""
import numpy as np
import torch
from scipy import ndimage

from oracle import inference as oinf
from tests import augment_restatement as R
from tests import kernel_ref as kr
from tests.kernel_ref import U32, _c

NEAR_TIE_CAP = 1e-4


# ---------------------------------------------------------------------------------------------------- padded random crop
def random_crop_pad(shape, crop):
    """The padding of the public LA RandomCrop, literally: if any axis of the volume is not larger than the crop, EVERY axis gets
    max((crop - size) // 2 + 3, 0) zero voxels on both sides; else none."""
    if shape[0] <= crop[0] or shape[1] <= crop[1] or shape[2] <= crop[2]:
        pw = max((crop[0] - shape[0]) // 2 + 3, 0)
        ph = max((crop[1] - shape[1]) // 2 + 3, 0)
        pd = max((crop[2] - shape[2]) // 2 + 3, 0)
        return (pw, ph, pd)
    return (0, 0, 0)


def draw3d_padded(rng, shape, patch):
    """The draws of one sample of DeviceLoader(pad=True), read from `rng` in the loader's order: k, axis, then the corner per axis."""
    k, axis = int(rng.integers(0, 4)), int(rng.integers(0, 2))
    crop = (patch[1], patch[0], patch[2]) if k % 2 else tuple(patch)
    pad = random_crop_pad(tuple(int(s) for s in shape), crop)
    padded = np.pad(np.zeros(shape, dtype=np.uint8), [(p, p) for p in pad]).shape
    corner = tuple(int(rng.integers(0, padded[a] - crop[a] + 1)) for a in range(3))
    return dict(corner=corner, k=k, axis=axis, pad=pad)


def augment3d_padded_numpy(image, label, draw, patch):
    """np.pad by the drawn pad (constant 0), then the crop + rot90 + flip of augment_restatement.augment3d_numpy."""
    width = [(p, p) for p in draw["pad"]]
    return R.augment3d_numpy(np.pad(image, width, mode="constant", constant_values=0), np.pad(label, width, mode="constant", constant_values=0), draw, patch)


def batch3d_padded_from_draws(images, labels, draws, patch):
    out = [augment3d_padded_numpy(np.asarray(images[d["index"]], dtype=np.float32), np.asarray(labels[d["index"]]), d, patch) for d in draws]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------------------------------------------- the window loop
class _Recorder:
    """A `net` for oracle.inference.test_single_case that keeps the patches it is shown and answers with zeros."""

    def __init__(self, C):
        self.C, self.patches = C, []

    def __call__(self, x):
        self.patches.append(x[0, 0].numpy().copy())
        return torch.zeros((1, self.C) + tuple(x.shape[2:]))


def oracle_patches(image, patch, stride_xy, stride_z):
    """The patches the reference's loop cuts (np.pad + slicing, test_3D_util.py:33-61 as restated in oracle/inference.py), in loop order."""
    rec = _Recorder(2)
    oinf.test_single_case(rec, np.asarray(image, dtype=np.float32), stride_xy, stride_z, patch, num_classes=2)
    return rec.patches


def oracle_origins(shape, patch, stride_xy, stride_z):
    """(pad_lo, origins in padded coordinates) of the windows oracle.inference.test_single_case walks over a volume of `shape`: the volume
    holds 1 + its own flat index, so any non-zero voxel of a patch names the source voxel it was cut from."""
    n = int(np.prod(shape))
    assert n < 2 ** 24                                       # exact in fp32
    image = (np.arange(n, dtype=np.float32) + 1).reshape(shape)
    lo = tuple(max(patch[a] - shape[a], 0) // 2 for a in range(3))
    origins = []
    for p in oracle_patches(image, patch, stride_xy, stride_z):
        assert p.shape == tuple(patch)
        pos = np.argwhere(p != 0)[0]
        src = np.unravel_index(int(p[tuple(pos)]) - 1, shape)
        origins.append(tuple(int(src[a]) + lo[a] - int(pos[a]) for a in range(3)))
    return lo, origins


def heads_value_ref(logits):
    """The value one batch of patches adds, per patch: logits = a list of one or two [K, C, pw, ph, pd] tensors.  dict(p, e_p) in fp64."""
    rs = [kr.infer_softmax_ref(_c(t)) for t in logits]
    if len(rs) == 1:
        return rs[0]
    p = (rs[0]["p"] + rs[1]["p"]) / 2.0
    return dict(p=p, e_p=(rs[0]["e_p"] + rs[1]["e_p"]) / 2.0 + U32 * p)


def window_accumulate_heads_ref(logits, origins, score0, cnt0):
    """chap_window_accumulate_heads, one launch: kernel_ref.window_accumulate_ref with the per-patch value of heads_value_ref."""
    val = heads_value_ref(logits)
    prior = _c(score0, val["p"])
    K, C, pw, ph, pd = val["p"].shape
    sp, se, n = torch.zeros_like(prior), torch.zeros_like(prior), torch.zeros_like(prior[0])
    for k, (x, y, z) in enumerate(origins):
        sl = (slice(x, x + pw), slice(y, y + ph), slice(z, z + pd))
        sp[(slice(None),) + sl] += val["p"][k]
        se[(slice(None),) + sl] += val["e_p"][k]
        n[sl] += 1
    return dict(score=prior + sp, score_b=se + n * U32 * (prior.abs() + sp), cnt=_c(cnt0, prior) + n, covered=n > 0)


def window_pipeline_ref(shape, patch, stride_xy, stride_z, batches, num_classes):
    """The whole sliding window in fp64 from the fp32 logits the network returned: `batches` = per launch a list of one or two
    [K, C, *patch] tensors, in order.  Origins and padding from the oracle's loop.  Returns dict(score [C, w, h, d], score_b, label, near)
    with the pad cropped off; the bound is carried over all launches (module docstring)."""
    lo, origins = oracle_origins(shape, patch, stride_xy, stride_z)
    padded = tuple(max(shape[a], patch[a]) for a in range(3))
    sp = torch.zeros((num_classes,) + padded, dtype=torch.float64)
    se, n = torch.zeros_like(sp), torch.zeros(padded, dtype=torch.float64)
    k0 = 0
    for logits in batches:
        val = heads_value_ref(logits)
        for k in range(val["p"].shape[0]):
            x, y, z = origins[k0 + k]
            sl = (slice(x, x + patch[0]), slice(y, y + patch[1]), slice(z, z + patch[2]))
            sp[(slice(None),) + sl] += val["p"][k]
            se[(slice(None),) + sl] += val["e_p"][k]
            n[sl] += 1
        k0 += val["p"].shape[0]
    assert k0 == len(origins) and bool((n > 0).all())
    fin = kr.window_finalize_ref(sp, n, se + n * U32 * sp)
    crop = tuple(slice(lo[a], lo[a] + shape[a]) for a in range(3))
    return dict(score=fin["score"][(slice(None),) + crop], score_b=fin["score_b"][(slice(None),) + crop],
                label=fin["label"][crop], near=fin["near"][crop], origins=origins, pad_lo=lo)


# ---------------------------------------------------------------------------------------------------- largest component
def largest_cc_scipy(seg):
    """The largest 26-connected component of seg > 0, labels kept inside it; scipy numbers the components in raster order of their first
    voxel and argmax takes the first maximum: equal sizes -> the component met first."""
    seg = np.asarray(seg)
    lab, n = ndimage.label(seg > 0, structure=np.ones((3, 3, 3)))
    if n == 0:
        return seg
    sizes = np.bincount(lab.reshape(-1))[1:]
    return seg * (lab == int(np.argmax(sizes)) + 1)


# ---------------------------------------------------------------------------------------------------- the stub network
class StubNet(torch.nn.Module):
    """Two logits tensors computed from the input alone: head h, class c = 4 sin(w[h][c] x + phi[h][c]), a fixed elementwise map that
    differs per head; class 0 wins where the input is 0 (the zero padding, an all-zero volume) in both heads.  Keeps the inputs and
    outputs of every call (CPU copies).  Runs where its input is."""
    W = ((2.3, 3.1, 4.7, 1.9), (2.9, 2.2, 3.7, 5.3))
    PHI = ((1.5, -0.5, 0.3, -1.2), (1.4, -0.3, 0.1, -1.0))

    def __init__(self, C=2, heads=2):
        super().__init__()
        self.C, self.heads, self.calls = C, heads, []

    def forward(self, x):
        outs = tuple(torch.cat([4.0 * torch.sin(self.W[h][c] * x + self.PHI[h][c]) for c in range(self.C)], dim=1).contiguous()
                     for h in range(self.heads))
        self.calls.append((x.detach().cpu().clone(), [o.detach().cpu().clone() for o in outs]))
        return outs if self.heads > 1 else outs[0]
