"""Inputs and bounds shared by tests/test_class_counts_cpu.py and tests/test_class_counts_kernels_gpu.py: the loss, pseudo-label and
VAT-distance kernels at the class counts 3, 5, 6, 7, 8 (csrc/loss.hip builds 2..8; 2 and 4 are covered by tests/kernel_ref.LOSS_SHAPES).

Bounds.  tests/kernel_ref.py's elementwise budget EW = 8 U32 counts the softmax chain "for C <= 4".  The chain of softmax_px at C classes is
the argument z - m, expf, C - 1 adds, the reciprocal and the product: C + 4 roundings.  `ew(C)` is that count in units of U32 (never below
kernel_ref's own 8, so no bound here is tighter or wider than kernel_ref's at C <= 4), and `chain_term(monkeypatch, C)` installs it for
a test's calls into kernel_ref.  Everything else in the bounds (accumulation gamma(N P), the propagated accumulator bounds, the stores) is
kernel_ref's, unchanged: those terms take C from the tensors.  Fixed before the first GPU run of the kernels at these counts."""
import torch

from tests import kernel_ref as kr

CLASSES = (3, 5, 6, 7, 8)
SCALAR = (4, (17, 19))              # P = 323, not a multiple of 4: the scalar KL path; two blocks, a ragged last wave
QUADS = (4, (16, 20))               # P = 320 on 16-byte-aligned tensors: the four-pixel KL path
TWO_TRIPS = (3, (420, 420))         # 529 200 pixels > 2048 * 256 > 512 * 256: a second grid-stride trip in every kernel (C = 3 and 8 only)
TWO_TRIPS_CLASSES = (3, 8)


def ew(C):
    return max(8, C + 4) * kr.U32


def chain_term(monkeypatch, C):
    monkeypatch.setattr(kr, "EW", ew(C))


def inputs(C, shape):
    """CPU inputs of one case: logits 3 randn (seed 100 + C), labels in [0, C) with some equal to C and to 255 (ignored: all-zero one-hot),
    a 0/1 mask, soft targets (one with exact zeros), and planted exact ties of the largest logit between class 0 and class C - 1 and, from
    C = 6 on, between classes 4 and 5: the first maximum wins."""
    N, sp = shape
    g = torch.Generator().manual_seed(100 + C)
    l1, l2 = 3 * torch.randn(N, C, *sp, generator=g), 3 * torch.randn(N, C, *sp, generator=g)
    P = l1[0, 0].numel()
    for lg, off in ((l1, 0), (l2, 7)):
        flat = lg.reshape(N, C, P)
        for j in range(40):
            n, px = j % N, (off + 97 * j) % P
            top = flat[n, :, px].max() + 1.0
            if j % 2 == 0 or C < 6:
                flat[n, 0, px] = top
                flat[n, C - 1, px] = top
            else:
                flat[n, 4, px] = top
                flat[n, 5, px] = top
    ta, tb = torch.randint(0, C, (N, *sp), generator=g), torch.randint(0, C, (N, *sp), generator=g)
    ta.reshape(-1)[3::11] = C                              # out of range by one: valid at C + 1 classes, ignored at C
    ta.reshape(-1)[5::13] = 255                            # the ignore label
    tb.reshape(-1)[2::17] = C
    tb.reshape(-1)[7::19] = 255
    mask = (torch.rand(N, *sp, generator=g) > 0.4).long()
    t1 = torch.softmax(torch.randn(N, C, *sp, generator=g), 1)
    t2 = torch.softmax(torch.randn(N, C, *sp, generator=g), 1)
    t2.reshape(N, C, P)[:, 0, ::5] = 0.0                   # exact zeros: the t > 0 guard of the KL term
    t2 = t2 / t2.sum(1, keepdim=True)
    return dict(N=N, C=C, sp=sp, l1=l1, l2=l2, ta=ta, tb=tb, mask=mask, t1=t1, t2=t2)


def cases():
    """(id, C, shape) of every GPU case."""
    out = []
    for C in CLASSES:
        out.append(("c%d_scalar" % C, C, SCALAR))
        out.append(("c%d_quads" % C, C, QUADS))
    for C in TWO_TRIPS_CLASSES:
        out.append(("c%d_two_trips" % C, C, TWO_TRIPS))
    return out
