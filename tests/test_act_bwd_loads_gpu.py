"""chap_act_bwd_reduce / _apply (pointwise.hip) bit for bit against what the commit BEFORE the load reordering computed.

The kernels' load order changed (all loads of a trip requested together, the next trip as soon as the current one is consumed, the
constants next to the first trip); their arithmetic and the order of every sum did not, so every output must keep its bits: the gradient `g`, the per-block
partial rows, the totals in row 0, dgamma and dbeta.  tests/golden/act_bwd_parent/blocks{1,2,3}.npz hold those arrays as recorded
on an MI355X from a build of the parent commit (`python tests/test_act_bwd_loads_gpu.py --golden --out <file>` with
CHAP_ACTBWD_BLOCKS = 1, 2, 3 and CHAP_LIBPATH naming the parent's library).  They are NEVER regenerated from the tree under test.

Shapes: the smallest at which the loop can go wrong -- N = 2 with 6x10 and 8x8 pixels, one 3D volume 2x4x6; C = 8, 16, 256 (one,
two and 32 threads per pixel: 256, 128 and 8 pixels per block step); 0..3 incoming gradients, one of them a slice of a wider buffer
(ld = 2C, coff = C); pooled gradient, keep mask, channel multipliers on and off; bn modes 0 / 1 / 2; with and without activation;
bf16 and fp32.  The grid is capped at 1, 2 and 3 blocks (CHAP_ACTBWD_BLOCKS is read once per process: one child process per
setting computes all cases), so threads make no trip (C = 8, 16: rows past the last pixel; a whole second block is never launched
as the grid is min(cap, steps)), exactly one trip, or several with a ragged last one (C = 256: 12 or 16 block steps over 1, 2 or 3
blocks).  The inputs are small integers over powers of two drawn from numpy's legacy MT19937 stream: the same bits on every host.

Bounds: `gout` sits inside a NaN-filled buffer with guard bands on both sides and the workspace is NaN-filled: every element of
`g` must have been written, and nothing outside it or past the last partial row.  Every case is also checked per element against
the fp64 restatement (tests/kernel_ref.py) with the bounds test_act_bwd_matrix uses."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "act_bwd_parent")
BLOCKS = (1, 2, 3)
GUARD = 64                                                 # elements of NaN on either side of gout (a multiple of 8: 16-byte alignment kept)
SLOPE, KEEP_SCALE = 0.01, 1.25
BF, F32 = "bf16", "fp32"
_DT = {BF: torch.bfloat16, F32: torch.float32}

# name: (N, D, H, W), C, dtype, incoming gradients, one of them a concat slice, pooled gradient, keep mask, channel multipliers, bn, activation
CASES = {
    "c16_bf16_one":        ((2, 1, 6, 10), 16, BF, 1, False, False, False, False, 1, True),
    "c16_bf16_ng2_pool":   ((2, 1, 6, 10), 16, BF, 2, True, True, False, False, 1, True),
    "c16_bf16_keep":       ((2, 1, 6, 10), 16, BF, 1, False, False, True, False, 1, True),
    "c8_bf16_ng3_all":     ((2, 1, 8, 8), 8, BF, 3, True, True, True, False, 1, True),
    "c8_f32_ng0_pool":     ((2, 1, 8, 8), 8, F32, 0, False, True, False, False, 1, True),
    "c8_bf16_ng0_pool":    ((2, 1, 6, 10), 8, BF, 0, False, True, False, False, 1, True),
    "c16_f32_ng2_all":     ((2, 1, 6, 10), 16, F32, 2, True, True, True, False, 1, True),
    "c16_bf16_3d_cm":      ((2, 2, 4, 6), 16, BF, 1, True, False, False, True, 1, True),
    "c8_f32_3d_ng3_bn2":   ((2, 2, 4, 6), 8, F32, 3, True, False, False, True, 2, True),
    "c16_bf16_bn0":        ((2, 1, 8, 8), 16, BF, 1, False, False, False, False, 0, True),
    "c16_f32_bn0_keep_cm": ((2, 1, 6, 10), 16, F32, 1, True, False, True, True, 0, True),
    "c16_bf16_bn2_noact":  ((2, 1, 6, 10), 16, BF, 2, False, False, False, False, 2, False),
    "c16_bf16_3d_noact":   ((2, 2, 4, 6), 16, BF, 1, False, False, False, False, 1, False),
    "c16_f32_3d_noact":    ((2, 2, 4, 6), 16, F32, 2, True, False, False, False, 1, False),
    "c16_bf16_everything": ((2, 1, 8, 8), 16, BF, 3, True, True, True, True, 1, True),
    "c256_bf16_ng2_all":   ((2, 1, 8, 8), 256, BF, 2, True, True, True, False, 1, True),
    "c256_f32_3d_keep_cm": ((2, 2, 4, 6), 256, F32, 1, False, False, True, True, 1, True),
}
FIXTURE_KEYS = ("g", "rows", "row0", "dgamma", "dbeta")


def _inputs(name):
    """CPU tensors of one case, NC(D)HW fp32; every value a small integer over a power of two (exact in bf16)."""
    (N, D, H, W), C, dtype, ng, sliced, pool, with_keep, with_cm, bn, act = CASES[name]
    rs = np.random.RandomState(1000 + sorted(CASES).index(name))
    sp = (H, W) if D == 1 else (D, H, W)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    k = rs.randint(-40, 41, (N, C) + sp).astype(np.int64)
    raw = k / 8.0
    red = (0,) + tuple(range(2, raw.ndim))
    cnt = float(N * D * H * W)                                                  # integer sums: the statistics do not depend on a summation order
    m1, m2 = k.sum(red) / cnt, (k * k).sum(red) / cnt
    mean = (m1 / 8.0).astype(np.float32)
    invstd = (1.0 / np.sqrt((m2 - m1 * m1) / 64.0 + 1e-5)).astype(np.float32)
    gamma = (rs.randint(8, 25, C) / 16.0).astype(np.float32)
    beta = (rs.randint(-8, 9, C) / 32.0).astype(np.float32)
    scale = gamma * invstd
    shift = beta - mean * scale
    d = dict(raw=f(raw), mean=f(mean), invstd=f(invstd), gamma=f(gamma), scale=f(scale), shift=f(shift))
    d["grads"] = [f(rs.randint(-32, 33, (N, C) + sp) / 16.0) for _ in range(ng)]
    d["gp"] = f(rs.randint(-32, 33, (N, C, H // 2, W // 2)) / 16.0) if pool else None
    d["idx"] = torch.from_numpy(rs.randint(0, 4, (N, C, H // 2, W // 2)).astype(np.uint8)) if pool else None
    d["keep"] = f(rs.randint(0, 5, (N, C) + sp) > 0) if with_keep else None
    d["cm"] = f((rs.randint(0, 3, (N, C)) > 0) * 1.5) if with_cm else None
    d["prior"] = f(rs.randint(-16, 17, (2, C)) / 16.0)                          # dgamma / dbeta accumulate (+=)
    d["count"] = N * D * H * W
    return d


def _nblocks(name, cap):
    (N, D, H, W), C = CASES[name][:2]
    ppb = 256 // (C // 8)
    return min(-(-(N * D * H * W) // ppb), cap)


def _bits(t):
    """a device tensor's storage as an integer numpy array"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def _run_case(name, cap):
    """One reduce + apply on the GPU; returns the arrays of FIXTURE_KEYS plus what the bounds check saw."""
    from chap_amd import ops
    from tests.test_kernels_gpu import DEV, cl
    (N, D, H, W), C, dtype, ng, sliced, pool, with_keep, with_cm, bn, act = CASES[name]
    dt, d = _DT[dtype], _inputs(name)
    lz = ops.Lazy(cl(d["raw"], dt), d["scale"].to(DEV), d["shift"].to(DEV), act, SLOPE, keep=None if d["keep"] is None else cl(d["keep"], torch.uint8),
                  keep_scale=KEEP_SCALE, chan_mul=None if d["cm"] is None else d["cm"].to(DEV))
    glist = []
    for i, gr in enumerate(d["grads"]):
        if sliced and i == min(1, ng - 1):                 # inside a wider buffer: ld = 2C, coff = C, the other half NaN (never to be read)
            wide = torch.full((N, D, H, W, 2 * C), float("nan"), device=DEV, dtype=dt)
            wide[..., C:] = cl(gr, dt)
            glist.append((wide, C))
        else:
            glist.append((cl(gr, dt), 0))
    n = N * D * H * W * C
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV, dtype=dt)
    gout = buf[GUARD:GUARD + n].view(N, D, H, W, C)
    sums = torch.full((ops.act_bwd_sums_size(C),), float("nan"), device=DEV, dtype=torch.float32)
    dgamma, dbeta = d["prior"][0].to(DEV), d["prior"][1].to(DEV)
    kw = dict(g_pool=cl(d["gp"], dt), pool_idx=cl(d["idx"], torch.uint8)) if pool else {}
    if bn:
        kw.update(mean=d["mean"].to(DEV), invstd=d["invstd"].to(DEV), gamma=d["gamma"].to(DEV), dgamma=dgamma, dbeta=dbeta, count=d["count"], bn_mode=bn, sums=sums)
    ops.act_bwd(lz, glist, gout, **kw)
    torch.cuda.synchronize()
    nb = _nblocks(name, cap) if bn else 0
    rows = sums.view(-1, 2 * C)
    return dict(g=_bits(gout), rows=_bits(rows[1:1 + nb]), row0=_bits(rows[:1 if bn else 0]), dgamma=_bits(dgamma), dbeta=_bits(dbeta),
                guards_nan=np.array(bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all())),
                tail_nan=np.array(bool(torch.isnan(rows[1 + nb:] if bn else rows).all())))


def _main(argv):
    """child process: every case at this process's CHAP_ACTBWD_BLOCKS into one .npz (--golden: the fixture arrays only)"""
    out = argv[argv.index("--out") + 1]
    cap = int(os.environ["CHAP_ACTBWD_BLOCKS"])
    res = {}
    for name in CASES:
        for k, v in _run_case(name, cap).items():
            if "--golden" not in argv or k in FIXTURE_KEYS:
                res[name + "/" + k] = v
    np.savez_compressed(out, **res)


@pytest.fixture(scope="module", params=BLOCKS)
def computed(request, tmp_path_factory):
    """(block cap, what a fresh process with that cap computed for every case)"""
    out = str(tmp_path_factory.mktemp("act_bwd_loads") / ("blocks%d.npz" % request.param))
    env = dict(os.environ, CHAP_ACTBWD_BLOCKS=str(request.param))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return request.param, dict(np.load(out)), dict(np.load(os.path.join(GOLDEN, "blocks%d.npz" % request.param)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent(computed, name):
    """g, the partial rows, row 0, dgamma and dbeta equal the parent build's, bit for bit; nothing written outside them."""
    cap, got, gold = computed
    for k in FIXTURE_KEYS:
        a, b = got[name + "/" + k], gold[name + "/" + k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), "%s %s (cap %d): %d of %d elements differ from the parent's" % (name, k, cap, int((a != b).sum()), a.size)
    assert bool(got[name + "/guards_nan"]), "written outside gout"
    assert bool(got[name + "/tail_nan"]), "written past the last partial row"
    assert CASES[name][8] == 0 or got[name + "/rows"].shape[0] == _nblocks(name, cap)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp64_reference(computed, name):
    """The same outputs per element against the fp64 restatement, bounds as in test_act_bwd_matrix."""
    from tests import kernel_ref as kr
    cap, got, _ = computed
    (N, D, H, W), C, dtype, ng, sliced, pool, with_keep, with_cm, bn, act = CASES[name]
    dt, d = _DT[dtype], _inputs(name)
    ref = kr.act_bwd_ref(d["raw"], d["grads"], scale=d["scale"], shift=d["shift"], act=act, slope=SLOPE, keep=d["keep"], keep_scale=KEEP_SCALE,
                         chan_mul=d["cm"], g_pool=d["gp"], pool_idx=d["idx"], bn_mode=bn, mean=d["mean"] if bn else None, invstd=d["invstd"],
                         gamma_=d["gamma"], count=d["count"])
    g = torch.from_numpy(got[name + "/g"]).view(dt).float().permute(0, 4, 1, 2, 3).contiguous()
    g = g if D > 1 else g.squeeze(2)
    w = [kr.check("gout", g, ref["g"], kr.bound(ref["g"], extra=ref["g_bound"], store=dt))]
    if bn:
        f = lambda k: torch.from_numpy(got[name + "/" + k]).view(torch.float32)
        w.append(kr.check("dbeta", f("dbeta"), ref["S0"] + d["prior"][1].double(), kr.param_grad_bound(ref["S0"], ref["b0"], d["prior"][1])))
        w.append(kr.check("dgamma", f("dgamma"), ref["S1"] + d["prior"][0].double(), kr.param_grad_bound(ref["S1"], ref["b1"], d["prior"][0])))
    print("act_bwd %s cap %d: worst err/bound %s" % (name, cap, " ".join("%.3f" % v for v in w)))


if __name__ == "__main__":
    _main(sys.argv[1:])
