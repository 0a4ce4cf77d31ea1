"""chap_sgd_ema_step per element: param / mom / the gradient buckets bit for bit what chap_sgd_step writes on the same inputs (and within
tests/kernel_ref.py::sgd_ref's bound of fp64), the average within tests/ema_ref.py's bound of its fp64 restatement, at the sizes where the
kernel changes path -- tail only (n = 1, 3), one quad, a quad and a tail (4, 5), body and a tail of 3 (1027), a second grid-stride trip and a
tail (2048 * 256 * 4 + 1024 + 3) -- with and without the second bucket, zeroing on and off, alpha = 0 (ema == the new parameter), 0.5 and
0.99, every buffer framed by NaN canaries that must stay.  One JSON line per size (worst err / bound; `-s` shows them):
profiles/mean_teacher_kernel.jsonl is a copy of those lines."""
import itertools
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import ops
from tests import ema_ref
from tests import kernel_ref as kr

DEV = torch.device("cuda", 0)
FRONT, BACK = 4, 8                      # canary elements around every buffer (the front keeps the payload 16-byte aligned)
SIZES = [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 1024 + 3]


def framed(t):
    """(device buffer [NaN x FRONT | t | NaN x BACK], the payload view)."""
    buf = torch.full((FRONT + t.numel() + BACK,), float("nan"), dtype=torch.float32, device=DEV)
    v = buf[FRONT:FRONT + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return buf, v


def canaries_intact(buf, n):
    return bool(torch.isnan(buf[:FRONT]).all()) and bool(torch.isnan(buf[FRONT + n:]).all())


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", SIZES)
def test_sgd_ema_step(n):
    g = torch.Generator().manual_seed(7000 + n % 9973)
    p, gr, m, g2, e = (torch.randn(n, generator=g) * s for s in (1.0, 1.0, 0.1, 1.0, 1.0))
    lr_buf, lr = framed(torch.tensor([0.013]))
    worst_e = worst_p = 0.0
    for grad2, zero, alpha in itertools.product((False, True), (False, True), (0.0, 0.5, 0.99)):
        gscale = 1.0 / 3.0 if grad2 else 1.0
        a, b = kr._fp32_scalar(alpha), kr._fp32_scalar(1.0 - alpha)
        tag = "n=%d grad2=%d zero=%d alpha=%g" % (n, grad2, zero, alpha)
        # the plain entry on the same inputs
        (pb0, p0), (gb0, gd0), (mb0, m0) = framed(p), framed(gr), framed(m)
        g2b0, g20 = framed(g2) if grad2 else (None, None)
        ops.sgd_step(p0, gd0, m0, lr, 0.9, 1e-4, grad_scale=gscale, zero_grad=zero, grad2=g20)
        # the fused one
        (pb, pd), (gb, gd), (mb, md), (eb, ed) = framed(p), framed(gr), framed(m), framed(e)
        g2b, g2d = framed(g2) if grad2 else (None, None)
        cb, coef = framed(torch.tensor([a, b]))
        ops.sgd_ema_step(pd, gd, md, lr, 0.9, 1e-4, ed, coef, grad_scale=gscale, zero_grad=zero, grad2=g2d)
        torch.cuda.synchronize()
        assert bits_equal(pd, p0) and bits_equal(md, m0) and bits_equal(gd, gd0), tag
        if grad2:
            assert bits_equal(g2d, g20), tag
        for t, src in ((gd, gr), (g2d, g2 if grad2 else None)):
            if t is not None:
                assert torch.equal(t.cpu(), torch.zeros(n) if zero else src), tag
        for buf in (pb, gb, mb, eb, g2b):
            assert buf is None or canaries_intact(buf, n), tag
        assert canaries_intact(cb, 2) and canaries_intact(lr_buf, 1) and coef.tolist() == [a, b] and lr.item() == kr._fp32_scalar(0.013), tag
        p2, e_p, m2, e_m = kr.sgd_ref(p, gr, m, 0.013, 0.9, 1e-4, gscale, g2 if grad2 else None)
        worst_p = max(worst_p, kr.check("sgd param " + tag, pd.cpu(), p2, e_p, "i"), kr.check("sgd mom " + tag, md.cpu(), m2, e_m, "i"))
        ref, bnd = ema_ref.ema_ref(e, pd.cpu(), a, b)           # on the parameter the kernel wrote (checked against fp64 just above)
        worst_e = max(worst_e, kr.check("ema " + tag, ed.cpu(), ref, bnd, "i"))
        if alpha == 0.0:
            assert bits_equal(ed, pd), tag                       # the first update: the teacher IS the student's new weights
    print(json.dumps({"kernel": "chap_sgd_ema_step", "n": n, "cases": 12, "ema_worst_err_over_bound": round(worst_e, 4),
                      "sgd_worst_err_over_bound": round(worst_p, 4)}))


def test_misaligned_ema_is_refused_on_device_pointers():
    from chap_amd import _lib
    n = 64
    t = [torch.zeros(n, device=DEV) for _ in range(3)]
    lr, coef = torch.tensor([0.01], device=DEV), torch.tensor([0.5, 0.5], device=DEV)
    off = torch.zeros(n + 1, device=DEV)[1:]
    with pytest.raises(_lib.ChapError, match="16-byte aligned"):
        ops.sgd_ema_step(t[0], t[1], t[2], lr, 0.9, 1e-4, off, coef)
    with pytest.raises(_lib.ChapError, match="null ema"):
        ops.sgd_ema_step(t[0], t[1], t[2], lr, 0.9, 1e-4, None, coef)
