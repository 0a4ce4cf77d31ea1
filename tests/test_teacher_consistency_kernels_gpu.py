"""chap_teacher_consistency per element against the fp64 restatement and bound of tests/teacher_ref.py, at every class count 2..8.  Shapes, the
class-count tests': 4 x C x 17 x 19 (P % 4 = 3: the one-pixel path, two blocks, a ragged last wave), 4 x C x 16 x 20 on 16-byte-aligned tensors
(the four-pixel path), the same shape through a view one float into its buffer (misaligned: the one-pixel path again) and, at C = 2 and 8,
3 x C x 420 x 420 (132 300 quads > 512 * 256: a second grid-stride trip).  Logits reach +-30.  The entry point is called through its parameter
struct on buffers with NaN behind every output, in the workspace rows the launch does not use and in `loss` beforehand.  Run with -s for one
line per check (worst err / bound) and one JSON line per case (profiles/teacher_consistency_kernels.jsonl holds those lines)."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from tests import kernel_ref as kr
from tests import teacher_ref as tr

DEV = torch.device("cuda", 0)
GUARD = 64
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, fill=None, offset=0):
    """(view of `shape` starting `offset` floats into a fresh buffer, the GUARD floats right behind it, the `offset` floats in front); NaN unless filled."""
    n = int(torch.Size(shape).numel())
    buf = torch.full((offset + n + GUARD,), NAN, dtype=torch.float32, device=DEV)
    v = buf[offset:offset + n].view(shape)
    if fill is not None:
        v.copy_(fill)
    return v, buf[offset + n:], buf[:offset]


def untouched(name, *guards):
    for g in guards:
        assert bool(torch.isnan(g).all()), "%s: a guard word next to it was written" % name


def blocks_of(N, P, quads):
    units = N * P // 4 if quads else N * P
    return min((units + 255) // 256, L.LOSS_SLOTS)


def launch(x, *, offset=0, want=(True, True), accumulate=False, gscale=1.0, gscale_dev=None, quads=None, prior_seed=5):
    """One call through the struct -> dict(loss, g [2] (None where dlogits was NULL), prior [2], ws).  Asserts which path the case reaches and
    that nothing outside the outputs was written."""
    N, C = x["s"][0].shape[:2]
    P = x["s"][0][0, 0].numel()
    shape = x["s"][0].shape
    ins = [guarded(shape, fill=t) for t in x["s"] + x["t"]]
    ins[0] = guarded(shape, fill=x["s"][0], offset=offset)            # the misaligned case: the first student head one float into its buffer
    gen = torch.Generator().manual_seed(prior_seed)
    prior = [0.01 * torch.randn(shape, generator=gen) if accumulate else None for _ in range(2)]
    outs = [guarded(shape, fill=prior[h]) if want[h] else None for h in range(2)]
    loss, loss_g, _ = guarded((1,))
    nb = blocks_of(N, P, quads)
    ws, ws_g, _ = guarded((1 + L.LOSS_SLOTS, 2))
    gd = None if gscale_dev is None else torch.tensor([gscale_dev], dtype=torch.float32, device=DEV)
    p = L.TeacherConsistencyParams()
    for h in range(2):
        p.logits[h], p.teacher[h] = ins[h][0].data_ptr(), ins[2 + h][0].data_ptr()
        p.dlogits[h] = outs[h][0].data_ptr() if want[h] else None
    aligned = P % 4 == 0 and all(t[0].data_ptr() % 16 == 0 for t in ins + [o for o in outs if o is not None])
    assert aligned == quads, "the case must reach the %s path" % ("four-pixel" if quads else "one-pixel")
    p.loss, p.ws, p.gscale, p.gscale_dev, p.accumulate = loss.data_ptr(), ws.data_ptr(), gscale, (None if gd is None else gd.data_ptr()), int(accumulate)
    p.N, p.C, p.P = N, C, P
    L.call("chap_teacher_consistency", p, _stream())
    torch.cuda.synchronize()
    untouched("loss", loss_g)
    untouched("ws", ws_g, ws[1 + nb:])                                # the rows behind the launch's blocks stay NaN
    assert bool(torch.isfinite(ws[:1 + nb]).all()), "a used workspace row was left unwritten"
    for t, src in zip(ins, x["s"] + x["t"]):
        untouched("input", t[1], t[2])
        assert torch.equal(t[0].cpu(), src), "an input was written"
    for o in outs:
        if o is not None:
            untouched("dlogits", o[1])
    return dict(loss=loss.clone(), g=[None if o is None else o[0].clone() for o in outs], prior=prior, ws=ws.clone(), nb=nb)


class Worst:
    def __init__(self, case, C):
        self.case, self.C, self.w = case, C, {}

    def chk(self, what, name, got, ref, bnd, dims="ncdhw"):
        r = kr.check("%s %s" % (self.case, name), got.cpu(), ref, bnd, dims)
        print("  %-52s worst err/bound %.3f" % ("%s %s" % (self.case, name), r))
        self.w[what] = max(self.w.get(what, 0.0), r)

    def compare(self, name, out, r):
        self.chk("loss", name + " loss", out["loss"], r["loss"], r["loss_b"], "i")
        count = r["g"][0].numel()
        for h in range(2):
            # row 0 of the workspace: the heads' own sums as the finalize kernel left them; over N C P, the heads' means (inside the loss's bound)
            self.chk("loss", "%s head %d" % (name, h), out["ws"][0, h:h + 1].double() / count, r["head"][h], r["loss_b"], "i")
            if out["g"][h] is not None:
                self.chk("grad", "%s g%d" % (name, h), out["g"][h], r["g"][h], r["g_b"][h])

    def log(self):
        print(json.dumps({"case": self.case, "C": self.C, "ew_u32": round(tr.ew(self.C) / kr.U32), "worst_ratio": {k: round(v, 4) for k, v in self.w.items()}}))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def cases():
    out = []
    for C in tr.CLASSES:
        out.append(("c%d_scalar" % C, C, tr.SCALAR, 0))
        out.append(("c%d_quads" % C, C, tr.QUADS, 0))
    for C in (2, 5, 8):
        out.append(("c%d_misaligned" % C, C, tr.QUADS, 1))
    for C in tr.TWO_TRIPS_CLASSES:
        out.append(("c%d_two_trips" % C, C, tr.TWO_TRIPS, 0))
    return out


@pytest.mark.parametrize("name,C,shape,offset", cases(), ids=[c[0] for c in cases()])
def test_teacher_consistency_per_element(name, C, shape, offset):
    x = tr.inputs(C, shape)
    assert max(float(t.abs().max()) for t in x["s"] + x["t"]) == 30.0
    quads = shape[1][0] * shape[1][1] % 4 == 0 and offset == 0
    big = shape == tr.TWO_TRIPS
    W = Worst(name, C)
    N, P = shape[0], shape[1][0] * shape[1][1]
    if big:
        assert N * P // 4 > L.LOSS_SLOTS * 256              # the second trip
    # plain write, no device scale
    a = launch(x, offset=offset, quads=quads)
    r = tr.teacher_ref(x["s"], x["t"])
    W.compare("write", a, r)
    assert a["nb"] == (L.LOSS_SLOTS if big else 2 if quads else (N * P + 255) // 256) and a["nb"] >= 2          # more than one block in every case
    # two launches: identical bits, workspace included
    b = launch(x, offset=offset, quads=quads)
    assert torch.equal(a["loss"], b["loss"]) and all(torch.equal(u, v) for u, v in zip(a["g"], b["g"])) and torch.equal(a["ws"][:1 + a["nb"]], b["ws"][:1 + b["nb"]])
    if not big:
        # accumulate over a nonzero prior, with the device scale
        c = launch(x, offset=offset, quads=quads, accumulate=True, gscale=0.3, gscale_dev=0.37)
        rc = tr.teacher_ref(x["s"], x["t"], gscale=0.3, gscale_dev=_f32(0.37), prior=c["prior"])
        W.compare("accumulate+gscale_dev", c, rc)
        assert torch.equal(c["loss"], a["loss"])            # the loss does not depend on the gradient's options
        # each dlogits NULL in turn, and both: the other output and the loss are bit for bit what they were
        for want in ((False, True), (True, False), (False, False)):
            d = launch(x, offset=offset, want=want, quads=quads)
            assert torch.equal(d["loss"], a["loss"])
            for h in range(2):
                assert (d["g"][h] is None) == (not want[h])
                if want[h]:
                    assert torch.equal(d["g"][h], a["g"][h])
    W.log()


@pytest.mark.parametrize("over,match", [(dict(C=9), r"C=9 \(2\.\.8 built\)"), (dict(C=1), r"C=1 \(2\.\.8 built\)"), (dict(N=0), "N=0, P=320")])
def test_refused_arguments_touch_nothing(over, match):
    shape = (4, 4, 16, 20)
    bufs = [guarded(shape) for _ in range(6)]
    loss, loss_g, _ = guarded((1,))
    ws, ws_g, _ = guarded((1 + L.LOSS_SLOTS, 2))
    p = L.TeacherConsistencyParams()
    for h in range(2):
        p.logits[h], p.teacher[h], p.dlogits[h] = bufs[h][0].data_ptr(), bufs[2 + h][0].data_ptr(), bufs[4 + h][0].data_ptr()
    p.loss, p.ws, p.gscale, p.N, p.C, p.P = loss.data_ptr(), ws.data_ptr(), 1.0, 4, 4, 320
    for k, v in over.items():
        setattr(p, k, v)
    with pytest.raises(L.ChapError, match=match):
        L.call("chap_teacher_consistency", p, _stream())
    torch.cuda.synchronize()
    untouched("everything", loss, loss_g, ws, ws_g, *[b[0] for b in bufs], *[b[1] for b in bufs])


def test_ops_wrapper_is_the_struct_call():
    x = tr.inputs(4, tr.QUADS)
    a = launch(x, quads=True, accumulate=True, gscale=0.3, gscale_dev=0.37)
    s, t = [v.to(DEV) for v in x["s"]], [v.to(DEV) for v in x["t"]]
    d = [v.to(DEV) for v in a["prior"]]
    loss = torch.full((1,), NAN, device=DEV)
    ops.teacher_consistency(s, t, loss, d, gscale=0.3, gscale_dev=torch.tensor([0.37], device=DEV), accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(loss, a["loss"]) and all(torch.equal(u, v) for u, v in zip(d, a["g"]))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.teacher_consistency(s, [t[0], t[1][:, :3]], loss)
