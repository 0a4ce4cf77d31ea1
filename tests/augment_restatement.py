"""CPU restatement of the training-input contract (DESIGN.md "Data layer"): RandomGenerator and TwoStreamBatchSampler as their
call sites use them (code/train_ours_2D.py:258-274, code/train_ablation_2D.py:116-131).  `dataloaders/dataset.py` is ABSENT from
the reference: the definition below is the public SSL4MIS one the reference derives from, UNPINNED by
necessity.  numpy + scipy only; nothing here imports chap_amd.

Two forms of the same transform:
  * `augment_scipy`: the contract itself, as calls of numpy.rot90 / numpy.flip / scipy.ndimage.rotate / scipy.ndimage.zoom;
  * `augment_plan`:  the same as ONE gather per output pixel from an index plan computed in plain IEEE fp64 with separate
    multiply and add -- the arithmetic chap_augment2d performs.  tests/test_augment_cpu.py requires the two to agree on every
    pixel, which makes the GPU test independent of the scipy build of the GPU machine.
A draw is a dict {index, mode, k, axis, angle}: mode 0 = none, 1 = rot90(k) + flip(axis), 2 = rotate(angle degrees)."""
import numpy as np
from scipy import ndimage, special

MODE_NONE, MODE_ROTFLIP, MODE_ROTATE = 0, 1, 2


def draw_sample(rng):
    """The draws of RandomGenerator.__call__ from a numpy.random.Generator, in a fixed order: u1; then (k, axis) or u2 [, angle]."""
    d = dict(mode=MODE_NONE, k=0, axis=0, angle=0)
    if rng.random() > 0.5:
        d.update(mode=MODE_ROTFLIP, k=int(rng.integers(0, 4)), axis=int(rng.integers(0, 2)))
    elif rng.random() > 0.5:
        d.update(mode=MODE_ROTATE, angle=int(rng.integers(-20, 20)))
    return d


# ------------------------------------------------------------------------------------------------ the contract (scipy calls)
def augment_scipy(image, label, draw, output_size):
    """RandomGenerator(output_size)({'image', 'label'}) with the draws given: image float32 [1, H, W], label int64 [H, W]."""
    if draw["mode"] == MODE_ROTFLIP:
        image = np.flip(np.rot90(image, draw["k"]), axis=draw["axis"]).copy()
        label = np.flip(np.rot90(label, draw["k"]), axis=draw["axis"]).copy()
    elif draw["mode"] == MODE_ROTATE:
        image = ndimage.rotate(image, draw["angle"], order=0, reshape=False)
        label = ndimage.rotate(label, draw["angle"], order=0, reshape=False)
    x, y = image.shape
    image = ndimage.zoom(image, (output_size[0] / x, output_size[1] / y), order=0)
    label = ndimage.zoom(label, (output_size[0] / x, output_size[1] / y), order=0)
    return image.astype(np.float32)[None], label.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the index plan (plain IEEE)
def zoom_scale(n_in, n_out):
    """Step of the zoom coordinate along one axis, (n_in - 1) / (n_out - 1) in fp64 (0 for a one-pixel output)."""
    return float(n_in - 1) / float(n_out - 1) if n_out > 1 else 0.0


def zoom_axis(n_in, n_out):
    """scipy.ndimage.zoom(order=0) along one axis: output o reads input floor(o * scale + 0.5); a coordinate outside [0, n_in - 1]
    gives the constant 0 (the edge quirk chap_amd.inference.zoom0 documents)."""
    c = np.arange(n_out, dtype=np.float64) * zoom_scale(n_in, n_out)
    inside = (c >= 0) & (c <= n_in - 1)
    return np.clip(np.floor(c + 0.5).astype(np.int64), 0, n_in - 1), inside


def rotate_params(angle, shape):
    """Matrix and offset of scipy.ndimage.rotate(reshape=False), computed as its Python code computes them."""
    c, s = special.cosdg(angle), special.sindg(angle)
    m = np.array([[c, s], [-s, c]])
    plane = np.asarray(shape)
    out_center = m @ ((plane - 1) / 2)
    in_center = (plane - 1) / 2
    return m, in_center - out_center


def rotflip_index(i, j, k, axis, x, y):
    """Source index of element (i, j) of flip(rot90(src, k), axis), src of shape (x, y)."""
    xo, yo = (y, x) if k % 2 else (x, y)
    if axis == 0:
        i = xo - 1 - i
    else:
        j = yo - 1 - j
    k = k % 4
    if k == 0:
        return i, j
    if k == 1:
        return j, y - 1 - i
    if k == 2:
        return x - 1 - i, y - 1 - j
    return x - 1 - j, i


def index_plan(draw, shape, output_size):
    """(si, sj, inside): arrays [H, W]: output pixel (o0, o1) is src[si, sj] where inside, else 0."""
    x, y = shape
    mode = draw["mode"]
    xi, yi = (y, x) if (mode == MODE_ROTFLIP and draw["k"] % 2) else (x, y)          # the shape the zoom sees
    H, W = output_size
    i0, in0 = zoom_axis(xi, H)
    i1, in1 = zoom_axis(yi, W)
    i = np.broadcast_to(i0[:, None], (H, W))
    j = np.broadcast_to(i1[None, :], (H, W))
    inside = in0[:, None] & in1[None, :]
    if mode == MODE_ROTFLIP:
        si, sj = rotflip_index(i, j, draw["k"], draw["axis"], x, y)
    elif mode == MODE_ROTATE:
        m, off = rotate_params(draw["angle"], shape)
        fi, fj = i.astype(np.float64), j.astype(np.float64)
        c0 = off[0] + fi * m[0, 0]          # separate multiply and add, in the order of scipy's loop
        c0 = c0 + fj * m[0, 1]
        c1 = off[1] + fi * m[1, 0]
        c1 = c1 + fj * m[1, 1]
        inside = inside & (c0 >= 0) & (c0 <= x - 1) & (c1 >= 0) & (c1 <= y - 1)
        si = np.clip(np.floor(c0 + 0.5).astype(np.int64), 0, x - 1)
        sj = np.clip(np.floor(c1 + 0.5).astype(np.int64), 0, y - 1)
    else:
        si, sj = i, j
    return si, sj, inside


def augment_plan(image, label, draw, output_size):
    si, sj, inside = index_plan(draw, image.shape, output_size)
    img = np.where(inside, image[si, sj], 0).astype(np.float32)
    lab = np.where(inside, label[si, sj], 0).astype(np.int64)
    return img[None], lab


def batch_from_draws(images, labels, draws, output_size, fn=augment_plan):
    """The batch a loader builds from `draws` (one per sample, with the slice's `index`): float32 [B, 1, H, W], int64 [B, H, W]."""
    out = [fn(np.asarray(images[d["index"]], dtype=np.float32), np.asarray(labels[d["index"]]), d, output_size) for d in draws]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------------------------------------ 3D (the project's own definition)
def augment3d_numpy(image, label, draw, patch):
    """Random crop at draw['corner'], rot90(k) in the first two axes, flip(axis in {0, 1}); with odd k the crop is taken with its
    first two sides swapped so that the OUTPUT has the patch shape.  float32 [1, D, H, W], int64 [D, H, W]."""
    p0, p1, p2 = patch
    c0, c1, c2 = draw["corner"]
    n0, n1 = (p1, p0) if draw["k"] % 2 else (p0, p1)
    out = []
    for a in (image, label):
        a = a[c0:c0 + n0, c1:c1 + n1, c2:c2 + p2]
        assert a.shape == (n0, n1, p2), "crop leaves the volume"
        out.append(np.flip(np.rot90(a, draw["k"], axes=(0, 1)), axis=draw["axis"]).copy())
    return out[0].astype(np.float32)[None], out[1].astype(np.int64)


def batch3d_from_draws(images, labels, draws, patch):
    out = [augment3d_numpy(np.asarray(images[d["index"]], dtype=np.float32), np.asarray(labels[d["index"]]), d, patch) for d in draws]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------------------------------------ sampler
def two_stream_batches(primary, secondary, batch_size, secondary_batch_size, rng):
    """One epoch of TwoStreamBatchSampler: one permutation of `primary` cut into groups of batch_size - secondary_batch_size, each joined
    by the next secondary_batch_size indices of an endless stream of permutations of `secondary`; primary first."""
    pbs = batch_size - secondary_batch_size
    prim = [primary[i] for i in rng.permutation(len(primary))]

    def endless():
        while True:
            for i in rng.permutation(len(secondary)):
                yield secondary[i]

    sec = endless()
    return [prim[b * pbs:(b + 1) * pbs] + [next(sec) for _ in range(secondary_batch_size)] for b in range(len(primary) // pbs)]
