"""utils/test_3d_patch.py of the reference, which is ABSENT upstream: `code/test_LA.py:5` imports `test_all_case` from it and calls it at
:50-58, and that call site plus the window bookkeeping of `code/test_3D_util.py:14-79` (symmetric zero padding, loop order x, y, z, the
last window clamped, soft-max scores summed and divided by the cover count) is all the reference pins.  Everything else here -- the
averaged two-decoder output, getLargestCC, the metric tuple, var_all_case -- follows the public LA evaluation code the name comes from
and is this project's definition, UNPINNED (DESIGN.md "3D workflow").

The whole window runs on the device: the volume and the origin table are uploaded once; per batch of origins chap_window_gather cuts
the patches (zero padding included), the network runs, chap_window_accumulate_heads adds the soft-max (one head) or the mean of the two
heads' soft-maxes; chap_window_finalize divides and takes the arg-max.  --nms is chap_largest_cc, the metrics are one chap_metrics
chain (chap_amd.metrics)."""
import math
import os

import numpy as np
import torch

from . import metrics, ops

WINDOW_BATCH = 4      # windows per network call of test_all_case / var_all_case (test_single_case_*: their `batch` argument)
__test__ = False      # the names below are the reference's (test_LA.py:5), not pytest's: nothing here is collected


def window_origins(shape, patch_size, stride_xy, stride_z):
    """The bookkeeping of test_3D_util.py:17-58 for a volume of `shape`: returns (pad_lo, pad_hi, padded_shape, origins) -- per axis
    p = max(patch - size, 0) split as p // 2 in front and p - p // 2 behind, and the window origins (padded coordinates) in loop order
    x, y, z with the last window of an axis clamped to the end."""
    pad = [max(int(patch_size[a]) - int(shape[a]), 0) for a in range(3)]
    lo = tuple(p // 2 for p in pad)
    hi = tuple(p - p // 2 for p in pad)
    ww, hh, dd = (int(shape[a]) + pad[a] for a in range(3))
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    origins = []
    for x in range(0, sx):
        xs = min(stride_xy * x, ww - patch_size[0])
        for y in range(0, sy):
            ys = min(stride_xy * y, hh - patch_size[1])
            for z in range(0, sz):
                zs = min(stride_z * z, dd - patch_size[2])
                origins.append((xs, ys, zs))
    return lo, hi, (ww, hh, dd), origins


def _predict_device(net, image, stride_xy, stride_z, patch_size, num_classes, batch, device, average):
    """(label uint8 [w, h, d], score fp32 [C, w, h, d]) on the device, the pad cropped off."""
    image = np.asarray(image)
    w, h, d = image.shape
    patch_size = tuple(int(p) for p in patch_size)
    lo, _, (ww, hh, dd), origins = window_origins(image.shape, patch_size, stride_xy, stride_z)
    device = torch.device(device)
    with torch.cuda.device(device):
        vol = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)          # unpadded: the padding is an index test
        table = torch.tensor(origins, dtype=torch.int32).to(device)                                # every origin, one upload
        score = torch.zeros((num_classes, ww, hh, dd), dtype=torch.float32, device=device)
        cnt = torch.zeros((ww, hh, dd), dtype=torch.float32, device=device)
        net.eval()
        with torch.no_grad():
            for k0 in range(0, len(origins), batch):
                og = table[k0:k0 + batch]
                out = net(ops.window_gather(vol, og, patch_size, lo))
                heads = list(out) if isinstance(out, (tuple, list)) else [out]
                heads = heads[:2] if average else heads[:1]
                ops.window_accumulate_heads([t.contiguous() for t in heads], og, score, cnt)
        label = ops.window_finalize(score, cnt)
    return label[lo[0]:lo[0] + w, lo[1]:lo[1] + h, lo[2]:lo[2] + d], score[:, lo[0]:lo[0] + w, lo[1]:lo[1] + h, lo[2]:lo[2] + d]


def _to_host(label, score):
    return label.cpu().numpy().astype(np.int64), score.contiguous().cpu().numpy()


def test_single_case_first_output(net, image, stride_xy, stride_z, patch_size, num_classes=1, batch=4, device="cuda:0"):
    """Sliding-window prediction from the first output of `net` (test_3D_util.py:14-79).  image: numpy [w, h, d];
    returns (label_map int64 [w, h, d], score_map fp32 [C, w, h, d])."""
    return _to_host(*_predict_device(net, image, stride_xy, stride_z, patch_size, num_classes, batch, device, average=False))


def test_single_case_average_output(net, image, stride_xy, stride_z, patch_size, num_classes=1, batch=4, device="cuda:0"):
    """As test_single_case_first_output with the score of a window = the mean of the soft-maxes of the first two outputs of `net`
    (a net with one output: that output); label_map = the first maximal class of the averaged, count-normalised score."""
    return _to_host(*_predict_device(net, image, stride_xy, stride_z, patch_size, num_classes, batch, device, average=True))


def _cuda():
    return torch.device("cuda", torch.cuda.current_device())


def _largest_cc_device(seg):
    """seg: integer device tensor [w, h, d] -> seg where the largest 26-connected component of seg > 0 is, else 0."""
    keep = ops.largest_cc((seg > 0).to(torch.int64).unsqueeze(0).contiguous(), 2)[0]
    return seg * keep.to(seg.dtype)


def getLargestCC(segmentation):
    """Keep the largest 26-connected component of `segmentation > 0` (labels preserved inside it, 0 elsewhere); among components of
    equal size the one met first in raster order (chap_largest_cc's rule; also skimage.measure.label + argmax(bincount[1:])).  An
    empty input is returned unchanged -- the public code asserts there.  numpy in, numpy out; a torch tensor stays a tensor."""
    if isinstance(segmentation, torch.Tensor):
        if not bool((segmentation > 0).any()):
            return segmentation
        seg = segmentation if segmentation.is_cuda else segmentation.to(_cuda())
        with torch.cuda.device(seg.device):
            return _largest_cc_device(seg).to(segmentation.device)
    arr = np.asarray(segmentation)
    if not (arr > 0).any():
        return segmentation
    dev = _cuda()
    with torch.cuda.device(dev):
        seg = torch.from_numpy(np.ascontiguousarray(arr).astype(np.int64)).to(dev)
        return _largest_cc_device(seg).cpu().numpy().astype(arr.dtype)


def calculate_metric_percase(pred, gt):
    """(dice, jc, hd95, asd) of two binary masks from one chap_metrics launch chain (the public code: four medpy calls).  Raises
    where medpy does: RuntimeError when either mask is empty (hd95 / asd)."""
    s = metrics.binary_all(pred, gt)
    if s["n_a"] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if s["n_b"] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return s["dc"], s["jc"], s["hd95"], s["asd"]


def _load_case(entry):
    """An image_list entry: a path to an h5 file with `image` and `label` (test_LA.py:28), or an (image, label) pair of arrays."""
    if isinstance(entry, (str, os.PathLike)):
        try:
            import h5py
        except ImportError as e:
            raise ImportError("chap_amd.test_3d_patch needs h5py to read %s; pass (image, label) array pairs in image_list instead" % (entry,)) from e
        with h5py.File(str(entry).strip(), "r") as h:
            return h["image"][:], h["label"][:]
    image, label = entry
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return to_np(image), to_np(label)


def _model_device(model):
    try:
        return next(model.parameters()).device
    except (StopIteration, AttributeError):
        return _cuda()


def test_all_case(model_name, num_outputs, model, image_list, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4,
                  save_result=True, test_save_path=None, preproc_fn=None, metric_detail=1, nms=0):
    """The call of test_LA.py:50-58.  num_outputs == 1: the first output of `model`; > 1: the average of its two decoders.  Optional
    largest-component post-processing (`nms`).  A case whose prediction is empty scores (0, 0, 0, 0).  Prints one line per case when
    `metric_detail`; returns the mean (dice, jc, hd95, asd) over the cases, a numpy array of length 4.  save_result writes
    `<test_save_path>/<ii>_pred|_img|_gt.nii.gz` and needs nibabel.  Windows go through the network in batches of WINDOW_BATCH
    (the signature is the issue's and the call site's: no keyword of its own)."""
    nib = None
    if save_result:
        try:
            import nibabel as nib
        except ImportError as e:
            raise ImportError("chap_amd.test_3d_patch.test_all_case(save_result=True) needs nibabel to write the predictions; "
                              "call it with save_result=False (test_LA.py:52 does)") from e
        if test_save_path is None:
            raise ValueError("test_all_case: save_result=True needs test_save_path")
    if len(image_list) == 0:
        raise ValueError("test_all_case: empty image_list")
    device = _model_device(model)
    total = np.zeros(4, dtype=np.float64)
    for ith, entry in enumerate(image_list):
        image, label = _load_case(entry)
        if preproc_fn is not None:
            image = preproc_fn(image)
        pred, _ = _predict_device(model, image, stride_xy, stride_z, patch_size, num_classes, WINDOW_BATCH, device, average=num_outputs > 1)
        with torch.cuda.device(device):
            pred = pred.contiguous()
            if nms:
                pred = getLargestCC(pred)
            if not bool(pred.any()):
                single = (0, 0, 0, 0)
            else:
                single = calculate_metric_percase(pred, label[:])
        if metric_detail:
            print("%02d,\t%.5f, %.5f, %.5f, %.5f" % (ith, single[0], single[1], single[2], single[3]))
        total += np.asarray(single, dtype=np.float64)
        if save_result:
            eye = np.eye(4)
            nib.save(nib.Nifti1Image(pred.cpu().numpy().astype(np.float32), eye), os.path.join(test_save_path, "%02d_pred.nii.gz" % ith))
            nib.save(nib.Nifti1Image(np.asarray(image[:]).astype(np.float32), eye), os.path.join(test_save_path, "%02d_img.nii.gz" % ith))
            nib.save(nib.Nifti1Image(np.asarray(label[:]).astype(np.float32), eye), os.path.join(test_save_path, "%02d_gt.nii.gz" % ith))
    avg = total / len(image_list)
    print("average metric is decoder 1 {}".format(avg))
    return avg


def var_all_case(model, image_list, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4):
    """Validation during training: the mean foreground Dice over the cases, from the first output, without nms (an empty prediction
    scores 0).  The prediction stays on the device: one counts-only chap_metrics launch per case."""
    if len(image_list) == 0:
        raise ValueError("var_all_case: empty image_list")
    device = _model_device(model)
    total = 0.0
    for entry in image_list:
        image, label = _load_case(entry)
        pred, _ = _predict_device(model, image, stride_xy, stride_z, patch_size, num_classes, WINDOW_BATCH, device, average=False)
        with torch.cuda.device(device):
            total += metrics.dc(pred.contiguous(), label)
    return total / len(image_list)
