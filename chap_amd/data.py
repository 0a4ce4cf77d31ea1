"""Device-resident training input: the data layer of the reference's loop (code/train_ours_2D.py:258-274: BaseDataSets +
RandomGenerator(image_size) in four DataLoader worker processes, TwoStreamBatchSampler) with the slices kept in device memory and
the augmentation done by ONE kernel per batch (chap_augment2d / chap_augment3d, include/chap_hip.h).

`dataloaders/dataset.py` is ABSENT from the reference: the three names are known by their call sites and by the
public SSL4MIS code base; the definition used here is written down in DESIGN.md "Data layer" and is UNPINNED by necessity.  The
random draws are made on the HOST with a seeded numpy.random.Generator (a few integers per sample) and travel to the device as a
record table of a few KB; `DeviceLoader.last_draws` exposes them, so a CPU restatement can be fed the same draws.  The 3D transform
(crop + rot90 + flip) is this project's own definition: upstream has no 3D training script."""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from . import ops

MODE_NONE, MODE_ROTFLIP, MODE_ROTATE = L.AUG_NONE, L.AUG_ROTFLIP, L.AUG_ROTATE


class _Store:
    """Arrays of differing shapes as one flat fp32 image buffer and one flat uint8 label buffer on the device, plus the host table
    (offset, shape) per item."""
    ndim = 0

    def __init__(self, images, labels, device="cuda"):
        if len(images) == 0 or len(images) != len(labels):
            raise ValueError("%s: need as many labels as images, and at least one (got %d / %d)" % (type(self).__name__, len(images), len(labels)))
        imgs, labs, shapes = [], [], []
        for n, (im, lb) in enumerate(zip(images, labels)):
            im, lb = np.asarray(im), np.asarray(lb)
            if im.ndim != self.ndim or im.shape != lb.shape or im.size == 0:
                raise ValueError("%s: item %d: image %s / label %s, expected two equal non-empty %dD shapes"
                                 % (type(self).__name__, n, im.shape, lb.shape, self.ndim))
            if lb.dtype.kind not in "iub" or lb.min() < 0 or lb.max() > 255:
                raise ValueError("%s: item %d: labels must be integers in [0, 255] (dtype %s)" % (type(self).__name__, n, lb.dtype))
            imgs.append(np.ascontiguousarray(im, dtype=np.float32).reshape(-1))
            labs.append(np.ascontiguousarray(lb, dtype=np.uint8).reshape(-1))
            shapes.append(im.shape)
        self.shapes = np.asarray(shapes, dtype=np.int64)
        sizes = self.shapes.prod(axis=1)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.device = torch.device(device)
        self.images = torch.from_numpy(np.concatenate(imgs)).to(self.device)
        self.labels = torch.from_numpy(np.concatenate(labs)).to(self.device)

    def __len__(self):
        return len(self.offsets)


class SliceStore(_Store):
    """SliceStore(images, labels, device): lists of [x, y] arrays (image float, label integer <= 255)."""
    ndim = 2

    @classmethod
    def from_h5_dir(cls, root, split="train", device="cuda"):
        """The ACDC layout the reference's BaseDataSets(base_dir=root, split='train') call expects (train_ours_2D.py:258-262):
        `<root>/<split>_slices.list` names the cases, `<root>/data/slices/<case>.h5` holds `image` and `label`."""
        try:
            import h5py
        except ImportError as e:
            raise ImportError("SliceStore.from_h5_dir needs h5py to read %s; build the store from arrays instead: "
                              "SliceStore(images, labels)" % root) from e
        with open(os.path.join(root, "%s_slices.list" % split)) as f:
            cases = [ln.strip() for ln in f if ln.strip()]
        images, labels = [], []
        for c in cases:
            with h5py.File(os.path.join(root, "data", "slices", "%s.h5" % c), "r") as h:
                images.append(h["image"][:])
                labels.append(h["label"][:])
        store = cls(images, labels, device)
        store.cases = cases
        return store


class VolumeStore(_Store):
    """VolumeStore(images, labels, device): lists of [d, h, w] arrays."""
    ndim = 3

    @classmethod
    def from_h5_list(cls, root, list_name="train.list", subdir="2018LA_Seg_Training Set", fname="mri_norm2.h5", device="cuda"):
        """The LA layout the reference spells out (test_LA.py:25-28): `<root>/<list_name>` names the cases,
        `<root>/<subdir>/<case>/<fname>` holds `image` and `label`.  `store.cases` keeps the names."""
        try:
            import h5py
        except ImportError as e:
            raise ImportError("VolumeStore.from_h5_list needs h5py to read %s; build the store from arrays instead: "
                              "VolumeStore(images, labels)" % root) from e
        with open(os.path.join(root, list_name)) as f:
            cases = [ln.strip() for ln in f if ln.strip()]
        images, labels = [], []
        for c in cases:
            with h5py.File(os.path.join(root, subdir, c, fname), "r") as h:
                images.append(h["image"][:])
                labels.append(h["label"][:])
        store = cls(images, labels, device)
        store.cases = cases
        return store


class TwoStreamBatchSampler:
    """Each epoch one permutation of `primary_indices` (the labelled ones) cut into groups of batch_size - secondary_batch_size, each
    joined by the next secondary_batch_size indices of an endless stream of permutations of `secondary_indices`; labelled first (the
    loop slices the batch that way, train_ours_2D.py:307-309); len = len(primary) // primary_batch_size (:299)."""

    def __init__(self, primary_indices, secondary_indices, batch_size, secondary_batch_size, seed=0):
        self.primary_indices, self.secondary_indices = list(primary_indices), list(secondary_indices)
        self.secondary_batch_size = int(secondary_batch_size)
        self.primary_batch_size = int(batch_size) - self.secondary_batch_size
        if not len(self.primary_indices) >= self.primary_batch_size > 0:
            raise ValueError("TwoStreamBatchSampler: %d primary indices for a primary batch of %d" % (len(self.primary_indices), self.primary_batch_size))
        if not (len(self.secondary_indices) >= self.secondary_batch_size >= 0) or (self.secondary_batch_size and not self.secondary_indices):
            raise ValueError("TwoStreamBatchSampler: %d secondary indices for a secondary batch of %d" % (len(self.secondary_indices), self.secondary_batch_size))
        self.rng = np.random.default_rng(seed)
        self._secondary = self._eternal()

    def _eternal(self):
        while True:
            for i in self.rng.permutation(len(self.secondary_indices)):
                yield self.secondary_indices[i]

    def __iter__(self):
        prim = [self.primary_indices[i] for i in self.rng.permutation(len(self.primary_indices))]
        for b in range(len(self)):
            yield prim[b * self.primary_batch_size:(b + 1) * self.primary_batch_size] + [next(self._secondary) for _ in range(self.secondary_batch_size)]

    def __len__(self):
        return len(self.primary_indices) // self.primary_batch_size


def draw_sample(rng):
    """The draws of RandomGenerator.__call__: u1 > 0.5 -> rot90(k in 0..3) + flip(axis in 0..1); else u2 > 0.5 -> rotate by an integer
    angle in -20..19 degrees; else nothing."""
    d = dict(mode=MODE_NONE, k=0, axis=0, angle=0)
    if rng.random() > 0.5:
        d.update(mode=MODE_ROTFLIP, k=int(rng.integers(0, 4)), axis=int(rng.integers(0, 2)))
    elif rng.random() > 0.5:
        d.update(mode=MODE_ROTATE, angle=int(rng.integers(-20, 20)))
    return d


_ROTATE_PARAMS = {}


def rotate_params(angle, shape):
    """Matrix and offset of scipy.ndimage.rotate(reshape=False) for a plane of `shape`, computed by the expressions of its Python code
    (the kernel takes them as fp64 values; recomputing them any other way could differ in the last bit)."""
    key = (int(angle), int(shape[0]), int(shape[1]))
    v = _ROTATE_PARAMS.get(key)
    if v is None:
        from scipy import special
        c, s = special.cosdg(angle), special.sindg(angle)
        m = np.array([[c, s], [-s, c]])
        plane = np.asarray([key[1], key[2]])
        out_center = m @ ((plane - 1) / 2)
        in_center = (plane - 1) / 2
        v = _ROTATE_PARAMS[key] = (m, in_center - out_center)
    return v


class DeviceLoader:
    """DeviceLoader(store, labeled_idxs, unlabeled_idxs, batch_size, labeled_bs, output_size, seed): batches of `labeled_bs` labelled
    then batch_size - labeled_bs unlabelled items of `store`, augmented on the device.  A valid `args["trainloader"]` of train(): iterating
    yields one epoch of {'image': fp32 [B, 1, *output_size], 'label': int64 [B, *output_size]} DEVICE tensors (fresh tensors, written on the
    current stream); `next_into(image_out, label_out)` writes the next batch of the endless sequence of epochs into caller-owned
    buffers on the current stream (ChapStep.stage_from).  `last_draws`: the draws of the last batch, one dict per sample.
    A VolumeStore gives the 3D transform with output_size = the patch [P0, P1, P2].  `pad=True` (VolumeStore only): a volume with an axis
    not larger than the crop is zero-padded on every axis before the crop (the public LA RandomCrop rule, DESIGN.md "3D workflow")
    instead of being refused; the draws then carry a `pad` tuple and `corner` is in padded coordinates.
    `rank`, `world` (data-parallel, DESIGN.md section 6 "train() on several ranks"): `batch_size` and `labeled_bs` are PER RANK.  Every rank
    runs the sampler and the augmentation draws of the GLOBAL batch (world * labeled_bs labelled, then world * (batch_size - labeled_bs)
    unlabelled items) from the same seed, in today's order, and keeps its own contiguous block [rank * n, (rank + 1) * n) of each group: the
    ranks' batches, concatenated labelled-first, are the batches of the world=1 loader of world * batch_size / world * labeled_bs.  The device
    side is one launch of batch_size records, as without ranks.  `last_draws`: the rank's own samples; `last_global_indices`: the store
    indices of the whole global batch."""
    RING = 4

    def __init__(self, store, labeled_idxs, unlabeled_idxs, batch_size, labeled_bs, output_size, seed=0, pad=False, rank=0, world=1):
        self.store, self.batch_size, self.labeled_bs = store, int(batch_size), int(labeled_bs)
        self.rank, self.world = int(rank), int(world)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError("DeviceLoader: rank=%d outside [0, world=%d)" % (self.rank, self.world))
        self.pad = bool(pad)
        if self.pad and store.ndim != 3:
            raise ValueError("DeviceLoader: pad=True is the 3D crop's padding; the store is %dD" % store.ndim)
        self.output_size = tuple(int(s) for s in output_size)
        if len(self.output_size) != store.ndim:
            raise ValueError("DeviceLoader: output_size %s for a %dD store" % (self.output_size, store.ndim))
        for i in list(labeled_idxs) + list(unlabeled_idxs):
            if not 0 <= i < len(store):
                raise IndexError("DeviceLoader: index %d outside the store of %d items" % (i, len(store)))
        if store.ndim == 3 and not self.pad:
            # a crop has the patch shape or, after an odd number of quarter turns, the patch with its first two sides swapped
            p = self.output_size
            need = (max(p[0], p[1]), max(p[0], p[1]), p[2])
            small = [i for i in list(labeled_idxs) + list(unlabeled_idxs) if (store.shapes[i] < need).any()]
            if small:
                raise ValueError("DeviceLoader: volume %d of shape %s is smaller than the crop %s of patch %s"
                                 % (small[0], tuple(store.shapes[small[0]]), need, p))
        self.sampler = TwoStreamBatchSampler(labeled_idxs, unlabeled_idxs, self.world * self.batch_size, self.world * (self.batch_size - self.labeled_bs), seed)
        lbs, ubs = self.labeled_bs, self.batch_size - self.labeled_bs
        # positions of this rank's samples in the global batch: its block of the labelled group, then its block of the unlabelled one
        self._own = [self.rank * lbs + j for j in range(lbs)] + [self.world * lbs + self.rank * ubs + j for j in range(ubs)]
        self.rng = np.random.default_rng([int(seed), 1])          # the augmentation draws: a stream of their own
        self._rec_t = L.Augment2dRecord if store.ndim == 2 else (L.Augment3dPadRecord if self.pad else L.Augment3dRecord)
        nbytes = ctypes.sizeof(self._rec_t) * self.batch_size
        # the record table: a ring of pinned host blocks, each with a device block of its own; a slot is rewritten only after the
        # launch that last read it has run (event), as ChapStep._upload_sched does for the schedule block
        # a host-resident store is DRAW-ONLY (the CPU checks of the draws use it: pinning needs a GPU); _launch refuses it by name
        on_gpu = self.store.device.type == "cuda"
        self._pin = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() if on_gpu else None for _ in range(self.RING)]
        self._dev = [torch.empty(nbytes, dtype=torch.uint8, device=store.device) for _ in range(self.RING)]
        self._ev, self._slot = [None] * self.RING, 0
        self._endless = self._eternal()
        self.last_draws, self.last_global_indices = None, None

    def __len__(self):
        return len(self.sampler)

    def _eternal(self):
        while True:
            for idxs in self.sampler:
                yield idxs

    def __iter__(self):
        dev = self.store.device
        for idxs in self.sampler:
            image = torch.empty((self.batch_size, 1) + self.output_size, dtype=torch.float32, device=dev)
            label = torch.empty((self.batch_size,) + self.output_size, dtype=torch.int64, device=dev)
            self._launch(idxs, image, label)
            yield {"image": image, "label": label}

    def next_into(self, image_out, label_out):
        self._launch(next(self._endless), image_out, label_out)

    def _draw(self, idxs):
        """Records and draws of this rank's samples of the (global) batch `idxs`.  The draws are made for EVERY sample of the global batch, in
        its order: the augmentation stream advances on all ranks alike."""
        recs, draws = self._draw_all(idxs)
        self.last_global_indices = [int(i) for i in idxs]
        if self.world == 1:
            return recs, draws
        own = (self._rec_t * self.batch_size)()
        for j, g in enumerate(self._own):
            own[j] = recs[g]
        return own, [draws[g] for g in self._own]

    def _draw_all(self, idxs):
        st = self.store
        recs = (self._rec_t * len(idxs))()
        draws = []
        for r, i in zip(recs, idxs):
            r.offset = int(st.offsets[i])
            if st.ndim == 2:
                x, y = (int(v) for v in st.shapes[i])
                d = dict(index=int(i), **draw_sample(self.rng))
                r.x, r.y, r.mode, r.k, r.axis = x, y, d["mode"], d["k"], d["axis"]
                xi, yi = (y, x) if (d["mode"] == MODE_ROTFLIP and d["k"] % 2) else (x, y)       # the shape the zoom sees
                r.zoom[0] = float(xi - 1) / float(self.output_size[0] - 1)
                r.zoom[1] = float(yi - 1) / float(self.output_size[1] - 1)
                if d["mode"] == MODE_ROTATE:
                    m, off = rotate_params(d["angle"], (x, y))
                    r.m[0], r.m[1], r.m[2], r.m[3] = m[0, 0], m[0, 1], m[1, 0], m[1, 1]
                    r.off[0], r.off[1] = off[0], off[1]
            else:
                k, axis = int(self.rng.integers(0, 4)), int(self.rng.integers(0, 2))
                p = self.output_size
                crop = (p[1], p[0], p[2]) if k % 2 else p
                sh = [int(v) for v in st.shapes[i]]
                pad = (0, 0, 0)
                if self.pad and any(sh[a] <= crop[a] for a in range(3)):      # RandomCrop: one small axis pads all three
                    pad = tuple(max((crop[a] - sh[a]) // 2 + 3, 0) for a in range(3))
                corner = tuple(int(self.rng.integers(0, sh[a] + 2 * pad[a] - crop[a] + 1)) for a in range(3))
                d = dict(index=int(i), corner=corner, k=k, axis=axis)
                for a in range(3):
                    r.shape[a], r.corner[a] = sh[a], corner[a]
                r.k, r.axis = k, axis
                if self.pad:
                    d["pad"] = pad
                    r.pad[0], r.pad[1], r.pad[2] = pad
            draws.append(d)
        return recs, draws

    def _launch(self, idxs, image_out, label_out):
        if len(idxs) != self.world * self.batch_size or image_out.shape[0] != self.batch_size or tuple(image_out.shape[2:]) != self.output_size:
            raise ValueError("DeviceLoader: output buffer %s for batches of %d x %s" % (tuple(image_out.shape), self.batch_size, self.output_size))
        if self._pin[0] is None:
            raise RuntimeError("DeviceLoader: the store lives on %s; batches are built by a GPU kernel (a host-resident store serves _draw only)" % self.store.device)
        recs, draws = self._draw(idxs)
        k = self._slot
        self._slot = (k + 1) % self.RING
        if self._ev[k] is not None:
            self._ev[k].synchronize()
        ctypes.memmove(self._pin[k].data_ptr(), ctypes.addressof(recs), ctypes.sizeof(recs))
        self._dev[k].copy_(self._pin[k], non_blocking=True)
        fn = ops.augment2d if self.store.ndim == 2 else (ops.augment3d_padded if self.pad else ops.augment3d)
        fn(self.store.images, self.store.labels, self._dev[k], image_out, label_out)
        ev = torch.cuda.Event()
        ev.record()
        self._ev[k] = ev
        self.last_draws = draws
