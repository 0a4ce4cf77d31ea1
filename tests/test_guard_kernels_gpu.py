"""chap_grad_norm and chap_sgd_guard_step per word.

chap_grad_norm at the smallest sizes that reach each path -- one vector (4), a tail of 3 (7, 1027), every thread of the fixed grid one vector
plus a tail (512 * 256 * 4 + 5), a second grid-stride trip (2 * 512 * 256 * 4 + 13) -- with and without the second bucket, at grad_scale 1 and
0.5, workspace and state pre-filled with NaN so that an unwritten word shows: the fp64 norm against math.fsum of the fp32-summed gradient
within (n * 2^-53 + 2 * 2^-52) relative (tests/guard_ref.py), the fp32 norm and coefficient within one ulp of the rounded reference, exact
cases bit for bit, the non-finite inputs, the ring.  chap_sgd_guard_step with and without the mean teacher's average: scale 1 and scale c bit
for bit the plain entries (called with fl32(grad_scale * c)), skip leaves param / mom / ema alone and zeroes the buckets."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib as L
from chap_amd import ops
from chap_amd.guard import HDR_WORDS, ROW_WORDS
from tests import guard_ref as gr

DEV = torch.device("cuda", 0)
T = L.GRADNORM_SLOTS * 256
SIZES = [4, 7, 1027, T * 4 + 5, 2 * T * 4 + 13]
NAN_BITS = int(np.float32("nan").view(np.int32))
COUNTERS = (5, 2, 1)                    # steps, skipped_total, clipped_total the state starts from


def fresh(ring, counters=COUNTERS):
    """(ws, state) filled with NaN bit patterns, the three counters (which the kernel reads) set."""
    ws = torch.full((L.GRADNORM_SLOTS,), float("nan"), dtype=torch.float64, device=DEV)
    state = torch.full((ops.guard_state_words(ring),), NAN_BITS, dtype=torch.int32, device=DEV)
    state[3:6] = torch.tensor(counters, dtype=torch.int32)
    return ws, state


def parse(state, ring):
    w = state.cpu().numpy()
    f = lambda i: float(w[i:i + 1].view(np.float32)[0])
    rows = w[HDR_WORDS:HDR_WORDS + ring * ROW_WORDS].reshape(ring, ROW_WORDS)
    return dict(scale=f(0), skip=int(w[1]), norm=f(2), steps=int(w[3]), skipped=int(w[4]), clipped=int(w[5]), reserved=w[6:8].tolist(), rows=rows, words=w)


def row_of(p, k):
    r = p["rows"][k]
    return int(r[0]), float(r[1:2].view(np.float32)[0]), float(r[2:3].view(np.float32)[0]), int(r[3])


def total_as_the_kernel_adds_it(ws):
    """The totals kernel's fixed order on the device's partials, in numpy doubles (IEEE additions: the same bits): lane l adds the partials
    l, l + 64, ..., then the xor butterfly 32, 16, ..., 1."""
    w = ws.cpu().numpy().astype(np.float64)
    v = np.zeros(64)
    for k in range(L.GRADNORM_SLOTS // 64):
        v = v + w[k * 64:(k + 1) * 64]
    o = 32
    while o:
        v = v + v[np.arange(64) ^ o]
        o >>= 1
    return float(v[0])


@functools.lru_cache(maxsize=None)
def inputs(n, two):
    g = torch.Generator().manual_seed(4100 + n % 9973)
    a = torch.randn(n, generator=g) * 0.05
    b = torch.randn(n, generator=g) * 0.05 if two else None
    return a, b, gr.total_of(gr.h_of(a, b))         # the reference sum once per input


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_against_fsum(n):
    for two in (False, True):
        a, b, total = inputs(n, two)
        ad, bd = a.to(DEV), (b.to(DEV) if two else None)
        for gs in (1.0, 0.5):
            ref_norm = math.sqrt(total) * gs
            max_norm = gr.fl32(0.5 * ref_norm)      # clips: coef near 1/2
            ref_coef = min(1.0, max_norm / (ref_norm + 1e-6))
            ws, state = fresh(3)
            ops.grad_norm(ad, bd, ws, state, 3, gs, max_norm, True)
            torch.cuda.synchronize()
            tag = "n=%d grad2=%d grad_scale=%g" % (n, two, gs)
            assert bool(torch.isfinite(ws).all()), tag                          # every block wrote its partial
            norm64 = math.sqrt(total_as_the_kernel_adds_it(ws)) * gs
            bound = n * 2.0 ** -53 + 2 * 2.0 ** -52
            print("  %s: |norm64 - ref| / ref = %.3g (bound %.3g)" % (tag, abs(norm64 - ref_norm) / ref_norm, bound))
            assert abs(norm64 - ref_norm) <= bound * ref_norm, tag
            p = parse(state, 3)
            assert gr.within_one_ulp(p["norm"], gr.fl32(ref_norm)) and gr.within_one_ulp(p["norm"], gr.fl32(norm64)), (tag, p["norm"], ref_norm)
            assert gr.within_one_ulp(p["scale"], gr.fl32(ref_coef)), (tag, p["scale"], ref_coef)
            assert (p["skip"], p["steps"], p["skipped"], p["clipped"], p["reserved"]) == (0, 6, 2, 2, [0, 0]), (tag, p)
            k = COUNTERS[0] % 3
            assert row_of(p, k) == (6, p["norm"], p["scale"], 0), tag
            others = np.delete(p["rows"], k, axis=0)
            assert (others == NAN_BITS).all(), tag                              # the other rows were not touched
            # the same launch again: the same bits (fixed order), the counters advance
            ops.grad_norm(ad, bd, ws, state, 3, gs, max_norm, True)
            torch.cuda.synchronize()
            q = parse(state, 3)
            assert (q["norm"], q["scale"], q["steps"], q["clipped"]) == (p["norm"], p["scale"], 7, 3), tag
            assert row_of(q, (k + 1) % 3) == (7, p["norm"], p["scale"], 0), tag


def test_exact_cases_match_the_restatement_bit_for_bit():
    for n in (7, 1027):
        z = torch.zeros(n)
        a = z.clone(); a[1], a[n - 1] = 3.0, 4.0
        b1, b2 = z.clone(), z.clone(); b1[1], b2[n - 1] = 3.0, -4.0
        for g, g2 in ((a, None), (b1, b2), (a, z)):
            for gs, mx in ((1.0, 2.5), (0.5, 1.0), (2.0, 0.0), (1.0, 7.0)):
                r = gr.guard_ref(g, g2, gs, mx)
                assert r["norm64"] == 5.0 * gs
                ws, state = fresh(2)
                ops.grad_norm(g.to(DEV), None if g2 is None else g2.to(DEV), ws, state, 2, gs, mx, True)
                torch.cuda.synchronize()
                p = parse(state, 2)
                assert (p["norm"], p["scale"], p["skip"]) == (r["norm"], r["coef"], 0), (n, gs, mx, p["norm"], p["scale"], r)
                assert p["clipped"] == COUNTERS[2] + int(r["coef"] < 1.0) and p["skipped"] == COUNTERS[1]
    # all zero: norm 0, coef 1 (max_norm / 1e-6 is far above 1)
    ws, state = fresh(2)
    ops.grad_norm(torch.zeros(1027, device=DEV), None, ws, state, 2, 1.0, 1.0, True)
    torch.cuda.synchronize()
    p = parse(state, 2)
    assert (p["norm"], p["scale"], p["skip"]) == (0.0, 1.0, 0)


def _nonfinite_cases(n):
    one = lambda: torch.ones(n) * 0.5
    a = one(); a[n - 1] = float("nan")
    yield "NaN in the last tail element", a, None
    yield "NaN in the last tail element, two buckets", a, one()
    a = one(); a[0] = float("inf")
    yield "inf at element 0", a, None
    b = one(); b[n // 2] = -float("inf")
    yield "-inf in grad2 only", one(), b
    a, b = one(), one(); a[5], b[5] = float("inf"), -float("inf")
    yield "+inf against -inf (h = NaN)", a, b
    a, b = one(), one(); a[4], b[4] = 3e38, 3e38
    yield "3e38 + 3e38 (h overflows in fp32)", a, b


@pytest.mark.parametrize("n", [7, 1027])
def test_nonfinite_inputs_set_skip(n):
    for name, a, b in _nonfinite_cases(n):
        ad, bd = a.to(DEV), (None if b is None else b.to(DEV))
        assert gr.guard_ref(a, b)["skip"] == 1, name
        ws, state = fresh(2)
        ops.grad_norm(ad, bd, ws, state, 2, 1.0, 1.0, True)
        torch.cuda.synchronize()
        p = parse(state, 2)
        assert (p["skip"], p["scale"]) == (1, 0.0) and not math.isfinite(p["norm"]), (name, p)
        assert (p["steps"], p["skipped"], p["clipped"]) == (COUNTERS[0] + 1, COUNTERS[1] + 1, COUNTERS[2]), (name, p)
        s, nm, cf, sk = row_of(p, COUNTERS[0] % 2)
        assert (s, cf, sk) == (COUNTERS[0] + 1, 0.0, 1) and not math.isfinite(nm), name
        # the user asked for no guard: the same input passes
        ws, state = fresh(2)
        ops.grad_norm(ad, bd, ws, state, 2, 1.0, 0.0, False)
        torch.cuda.synchronize()
        p = parse(state, 2)
        assert (p["skip"], p["scale"]) == (0, 1.0) and not math.isfinite(p["norm"]), (name, p)
        assert (p["skipped"], p["clipped"]) == (COUNTERS[1], COUNTERS[2]), (name, p)
    # 3e38 in ONE bucket is finite: nothing is skipped
    a = torch.ones(n); a[4] = 3e38
    ws, state = fresh(2)
    ops.grad_norm(a.to(DEV), None, ws, state, 2, 1.0, 0.0, True)
    torch.cuda.synchronize()
    p = parse(state, 2)
    assert p["skip"] == 0 and gr.within_one_ulp(p["norm"], gr.guard_ref(a)["norm"])


def test_ring_row_lands_at_steps_mod_ring_and_wraps():
    ring = 4
    ws, state = fresh(ring, (0, 0, 0))
    state[HDR_WORDS:] = 0
    norms = []
    for k in range(6):
        g = torch.zeros(7); g[0] = float(k + 1)
        ops.grad_norm(g.to(DEV), None, ws, state, ring, 1.0, 0.0, True)
        torch.cuda.synchronize()
        p = parse(state, ring)
        assert p["steps"] == k + 1 and row_of(p, k % ring) == (k + 1, float(k + 1), 1.0, 0)
        norms.append(p["norm"])
    assert norms == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert [row_of(p, i)[0] for i in range(ring)] == [5, 6, 3, 4]           # rows 0 and 1 were written a second time


# ---- chap_sgd_guard_step -------------------------------------------------------------------------------------------------------------------
STEP_SIZES = [7, 1027, 2048 * 256 * 4 + 1024 + 3]


def state_with(scale, skip):
    st = torch.full((ops.guard_state_words(1),), NAN_BITS, dtype=torch.int32, device=DEV)
    st[0] = int(np.float32(scale).view(np.int32))
    st[1] = skip
    return st


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", STEP_SIZES)
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_sgd_guard_step(n, ema):
    g = torch.Generator().manual_seed(8100 + n % 9973)
    p, gd, m, g2, e = (torch.randn(n, generator=g) * s for s in (1.0, 1.0, 0.1, 1.0, 1.0))
    lr = torch.tensor([0.013], device=DEV)
    coef = torch.tensor([0.99, gr.fl32(1.0 - 0.99)], device=DEV)
    dev = lambda *ts: [None if t is None else t.to(DEV).clone() for t in ts]

    def plain(gs, two):
        P, G, M, G2, E = dev(p, gd, m, g2 if two else None, e)
        if ema:
            ops.sgd_ema_step(P, G, M, lr, 0.9, 1e-4, E, coef, grad_scale=gs, zero_grad=True, grad2=G2)
        else:
            ops.sgd_step(P, G, M, lr, 0.9, 1e-4, grad_scale=gs, zero_grad=True, grad2=G2)
        return P, G, M, G2, E

    def guarded(gs, two, scale, skip, zero=True):
        P, G, M, G2, E = dev(p, gd, m, g2 if two else None, e)
        st = state_with(scale, skip)
        ops.sgd_guard_step(P, G, M, lr, 0.9, 1e-4, st, E if ema else None, coef if ema else None, grad_scale=gs, zero_grad=zero, grad2=G2)
        return P, G, M, G2, E

    for two in (False, True):
        gs = 1.0 / 3.0 if two else 1.0
        for scale in (1.0, 0.37):
            tag = "n=%d ema=%d grad2=%d scale=%g" % (n, ema, two, scale)
            gs_eff = float(np.float32(gs) * np.float32(scale))                  # fl32(grad_scale * c), the one product the kernel forms
            if scale == 1.0:
                assert gs_eff == gr.fl32(gs)
            want, got = plain(gs_eff, two), guarded(gs, two, scale, 0)
            torch.cuda.synchronize()
            for name, a, b in zip(("param", "grad", "mom", "grad2", "ema"), got, want):
                if a is not None and (name != "ema" or ema):
                    assert bits_equal(a, b), (tag, name)
            assert float(got[1].abs().max()) == 0.0 and (not two or float(got[3].abs().max()) == 0.0), tag
            assert not bits_equal(got[0], p.to(DEV)), tag
        # skip: nothing but the zeroing of the buckets
        tag = "n=%d ema=%d grad2=%d skip" % (n, ema, two)
        P, G, M, G2, E = guarded(gs, two, 0.0, 1)
        torch.cuda.synchronize()
        assert bits_equal(P, p.to(DEV)) and bits_equal(M, m.to(DEV)) and bits_equal(E, e.to(DEV)), tag
        assert float(G.abs().max()) == 0.0 and (not two or float(G2.abs().max()) == 0.0), tag
        # ... even with NaN in them, and left alone when the caller keeps its gradients (zero_grad = 0)
        P, G, M, G2, E = guarded(gs, two, 0.0, 1, zero=False)
        torch.cuda.synchronize()
        assert bits_equal(P, p.to(DEV)) and bits_equal(M, m.to(DEV)) and bits_equal(G, gd.to(DEV)) and (not two or bits_equal(G2, g2.to(DEV))), tag


def test_norm_then_guarded_step_skips_a_poisoned_gradient_and_clears_it():
    """The two entries as FusedSGD.step issues them: a NaN in the last element of bucket 1."""
    n = 1027
    g = torch.Generator().manual_seed(5)
    p, gd, m, g2 = (torch.randn(n, generator=g).to(DEV) for _ in range(4))
    g2[n - 1] = float("nan")
    p0, m0 = p.clone(), m.clone()
    lr = torch.tensor([0.01], device=DEV)
    ws, state = fresh(2, (0, 0, 0))
    ops.grad_norm(gd, g2, ws, state, 2, 0.5, 1.0, True)
    ops.sgd_guard_step(p, gd, m, lr, 0.9, 1e-4, state, grad_scale=0.5, grad2=g2)
    torch.cuda.synchronize()
    assert bits_equal(p, p0) and bits_equal(m, m0) and float(gd.abs().max()) == 0.0 and float(g2.abs().max()) == 0.0
    assert parse(state, 2)["skipped"] == 1


def test_misaligned_buffers_are_refused_on_device_pointers():
    n = 64
    t = [torch.zeros(n, device=DEV) for _ in range(3)]
    lr = torch.tensor([0.01], device=DEV)
    ws, state = fresh(1)
    off = torch.zeros(n + 1, device=DEV)[1:]
    with pytest.raises(L.ChapError, match="16-byte"):
        ops.grad_norm(off, None, ws, state, 1)
    with pytest.raises(L.ChapError, match="16-byte aligned"):
        ops.sgd_guard_step(t[0], t[1], t[2], lr, 0.9, 1e-4, state, grad2=off)
    with pytest.raises(ValueError, match="int32 words"):
        ops.grad_norm(t[0], None, ws, state, 2)                 # a state block too small for the ring
