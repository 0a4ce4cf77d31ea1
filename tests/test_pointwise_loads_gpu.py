"""chap_act_pool2, chap_upsample2x, chap_channel_sum and chap_wgrad's slab reduction bit for bit against what the commit BEFORE their
loads were reordered computed.

What changed is how these kernels ask for their data (pointwise.hip "A lazy source ...", wgrad_api.hip): the 2D pool window and the
corners of an up-sampling cell are requested together, the channel sum requests its next trip while it adds the current one, the two
totalling kernels request their partial rows and the prior value they add to at once.  The arithmetic and the order of every sum,
maximum and comparison did not change, so every output must keep its bits.  tests/golden/pointwise_parent/{base,ragged}.npz hold the
outputs as recorded on an MI355X from a build of the parent commit (`python tests/test_pointwise_loads_gpu.py --golden --set base|ragged
--out <file>` with CHAP_LIBPATH naming the parent's library; `ragged` with CHAP_GRID_SCALE=1).  They are NEVER regenerated from the tree
under test.  An output of more than 32 KB is kept as the SHA-256 digest of its bytes.

Cases: the smallest shapes at which these loops can go wrong.
  pool      N = 2 at 6x10 and 8x8, one 3D volume 2x4x6; C = 8, 16, 24 (three channel groups: a thread's group changes between trips), 256;
            plain source, scale / shift + activation, + keep mask, + channel multipliers (the last two and 3D take the general kernel);
            index bytes on and off; ties inside every window; NaNs inside windows; bf16 and fp32
  upsample  inputs 2x2, 3x5, 3D 2x3x4, one axis of length 1 (the per-output kernel); half_pixel 0 / 1; the output as the second half of
            a NaN-filled concat buffer; the same source variants
  chansum   60 and 64 pixels; C = 8, 16, 512; the source variants; 611 block steps over CHAP_CHANSUM_SLOTS = 512 blocks (two trips, ragged)
  wgrad     cases of tests/k3_conv_cases.py that reach both reduce instances: 1, 4, 5, 9, 12, 16, 18, 40 slabs (wgrad_reduce_kernel<64>:
            below, at and above one and four slab groups) and 80 (<8>); db on and off; the padded head (kn_valid = 4); kc_valid = 8 and 1
  ragged    (a child process with CHAP_GRID_SCALE=1: every grid cap at 1 %, 64 blocks at least) pool C = 256, N = 2, 36x32 (64 blocks) and
            up-sampling C = 256, N = 2, 17x18 and 33x34 (163 blocks): several trips per thread, the last one ragged
Outputs sit in NaN-filled buffers with NaN guard bands; accumulated outputs (dw, db, the channel sums) start from non-zero priors.
Pool, up-sampling and channel-sum inputs are small integers over powers of two from numpy's legacy MT19937 stream; the weight-gradient
cases draw theirs as tests/k3_conv_cases.py does.  Every case is also checked per element against the fp64 restatements of
tests/kernel_ref.py with the bounds tests/test_step_launches_gpu.py and tests/k3_conv_cases.py use."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.plan_probe import KNOBS, probe  # noqa: E402,F401  (probe: the planner fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "pointwise_parent")
GUARD = 64
BIG = 32 * 1024                                            # bytes: larger outputs are compared (and stored) as digests
SLOPE, KEEP_SCALE = 0.01, 1.25
BF, F32 = "bf16", "fp32"
_DT = {BF: torch.bfloat16, F32: torch.float32}
CHANSUM_SLOTS = 512

# source variants: p plain, a scale / shift + LeakyReLU, ak + keep mask, akm + channel multipliers
# pool: (N, D, H, W), C, dtype, variant, idx, special (None / "tie" / "nan")
POOL = {
    "pool_6x10_c8_bf16_p_idx":    ((2, 1, 6, 10), 8, BF, "p", True, None),
    "pool_8x8_c16_f32_a":         ((2, 1, 8, 8), 16, F32, "a", False, None),
    "pool_6x10_c24_bf16_a_idx":   ((2, 1, 6, 10), 24, BF, "a", True, None),
    "pool_6x10_c24_f32_p_idx":    ((2, 1, 6, 10), 24, F32, "p", True, None),
    "pool_6x10_c16_bf16_ak_idx":  ((2, 1, 6, 10), 16, BF, "ak", True, None),
    "pool_8x8_c16_f32_akm_idx":   ((2, 1, 8, 8), 16, F32, "akm", True, None),
    "pool_8x8_c256_bf16_a_idx":   ((2, 1, 8, 8), 256, BF, "a", True, None),
    "pool_3d_c16_bf16_a_idx":     ((2, 2, 4, 6), 16, BF, "a", True, None),
    "pool_3d_c8_f32_akm":         ((2, 2, 4, 6), 8, F32, "akm", False, None),
    "pool_8x8_c8_bf16_tie_idx":   ((2, 1, 8, 8), 8, BF, "a", True, "tie"),
    "pool_6x10_c16_f32_tie_idx":  ((2, 1, 6, 10), 16, F32, "p", True, "tie"),
    "pool_6x10_c16_bf16_nan_idx": ((2, 1, 6, 10), 16, BF, "a", True, "nan"),
    "pool_8x8_c8_f32_nan_idx":    ((2, 1, 8, 8), 8, F32, "p", True, "nan"),
}
# upsample: input (N, D, H, W), C, dtype, variant, dims, half_pixel, concat slot
UP = {
    "up_2x2_c8_bf16_p":         ((2, 1, 2, 2), 8, BF, "p", 2, 0, False),
    "up_3x5_c16_f32_a_hp":      ((2, 1, 3, 5), 16, F32, "a", 2, 1, False),
    "up_3x5_c16_bf16_a_slot":   ((2, 1, 3, 5), 16, BF, "a", 2, 0, True),
    "up_3x5_c24_bf16_a":        ((2, 1, 3, 5), 24, BF, "a", 2, 0, False),
    "up_3x5_c16_bf16_ak_slot":  ((2, 1, 3, 5), 16, BF, "ak", 2, 1, True),
    "up_3x5_c16_f32_akm":       ((2, 1, 3, 5), 16, F32, "akm", 2, 0, False),
    "up_3d_c8_bf16_a":          ((2, 2, 3, 4), 8, BF, "a", 3, 0, False),
    "up_3d_c16_f32_p_hp_slot":  ((2, 2, 3, 4), 16, F32, "p", 3, 1, True),
    "up_3d_c16_bf16_akm":       ((2, 2, 3, 4), 16, BF, "akm", 3, 0, False),
    "up_1x5_c8_bf16_a":         ((2, 1, 1, 5), 8, BF, "a", 2, 0, False),
    "up_3d_1x3x4_c8_f32_a":     ((2, 1, 3, 4), 8, F32, "a", 3, 0, False),
}
# channel sum: (N, D, H, W), C, dtype, variant
CHANSUM = {
    "sum_60_c8_bf16_p":      ((2, 1, 5, 6), 8, BF, "p"),
    "sum_64_c16_f32_a":      ((2, 1, 4, 8), 16, F32, "a"),
    "sum_60_c16_bf16_ak":    ((2, 1, 5, 6), 16, BF, "ak"),
    "sum_64_c8_f32_akm":     ((2, 1, 4, 8), 8, F32, "akm"),
    "sum_3d_60_c16_bf16_akm": ((2, 2, 3, 5), 16, BF, "akm"),
    "sum_64_c512_bf16_a":    ((2, 1, 4, 8), 512, BF, "a"),
    "sum_60_c512_f32_p":     ((2, 1, 5, 6), 512, F32, "p"),
    "sum_trips_c512_bf16_a": ((2, 1, 33, 37), 512, BF, "a"),
}
# weight gradient: (case of tests/k3_conv_cases.py, dtype name there, CHAP_WGRAD_BLOCKS override or None, slab count)
WGRAD = {
    "wg_split1_bf16":    ("w2_split1", "bf16", None, 1),
    "wg_split4_f32":     ("w2_split5", "f32", 4, 4),
    "wg_split5_f32":     ("w2_split5", "f32", None, 5),
    "wg_split9_wp_bf16": ("wp2_split9_of_9", "bf16", None, 9),
    "wg_split12_bf16":   ("w2_split12", "bf16", None, 12),
    "wg_split16_bf16":   ("w2_split5", "bf16", 16, 16),
    "wg_split18_bf16":   ("w2_16_16", "bf16", None, 18),
    "wg_3d_split40_f32": ("w3_16_16", "f32", None, 40),
    "wg_reduce8_bf16":   ("w2_reduce8", "bf16", None, 80),
    "wg_reduce8_f32":    ("w2_reduce8", "f32", None, 80),
    "wg_head_bf16":      ("w2_head_16_4", "bf16", None, None),
    "wg_kc_valid_f32":   ("w2_kc_valid_8", "f32", None, None),
    "wg_kc_valid1_bf16": ("w2_kc_valid_8", "bf16", None, None, dict(kc_valid=1)),      # the one-channel first layer: one valid row of the padded K
}
RAGGED_POOL = {"ragged_pool_36x32_c256_bf16_a_idx": ((2, 1, 36, 32), 256, BF, "a", True, None)}
RAGGED_UP = {"ragged_up_17x18_c256_bf16_a": ((2, 1, 17, 18), 256, BF, "a", 2, 0, False),       # (163 blocks: 17408 cells in one trip)
             "ragged_up_33x34_c256_bf16_a": ((2, 1, 33, 34), 256, BF, "a", 2, 0, False)}       # 67584 cells over 163 blocks: two trips, the second ragged
POOL_ALL, UP_ALL = dict(POOL, **RAGGED_POOL), dict(UP, **RAGGED_UP)
SETS = {"base": sorted(POOL) + sorted(UP) + sorted(CHANSUM) + sorted(WGRAD), "ragged": sorted(RAGGED_POOL) + sorted(RAGGED_UP)}
SET_ENV = {"base": {}, "ragged": {"CHAP_GRID_SCALE": "1"}}
ALL = sorted(POOL_ALL) + sorted(UP_ALL) + sorted(CHANSUM) + sorted(WGRAD)


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _source(name, shape, C, variant, special=None):
    """CPU tensors of one lazy source, NC(D)HW fp32: small integers over powers of two (exact in bf16)"""
    N, D, H, W = shape
    rs = np.random.RandomState(2000 + ALL.index(name))
    sp = (H, W) if D == 1 else (D, H, W)
    raw = rs.randint(-40, 41, (N, C) + sp) / 8.0
    if special == "tie":
        raw = rs.randint(-1, 2, (N, C) + sp) / 2.0          # three values: every window has equal samples
    d = dict(scale=None, shift=None, keep=None, cm=None)
    if variant != "p":
        d["scale"], d["shift"] = _f(rs.randint(8, 25, C) / 16.0), _f(rs.randint(-8, 9, C) / 32.0)
    if "k" in variant:
        d["keep"] = _f(rs.randint(0, 5, (N, C) + sp) > 0)
    if "m" in variant:
        d["cm"] = _f((rs.randint(0, 3, (N, C)) > 0) * 1.5)
    if special == "nan":
        raw = raw.reshape(N, C, -1)
        raw[:, :, rs.randint(0, raw.shape[2], raw.shape[2] // 3)] = np.nan      # first, middle and last samples of windows
        raw[0, 0, :] = np.nan                                                   # and whole windows
        raw = raw.reshape((N, C) + sp)
    d["raw"] = _f(raw)
    d["prior"] = _f(rs.randint(-16, 17, C) / 16.0)
    return d


def _lazy(d, variant, dt):
    from chap_amd import ops
    from tests.test_kernels_gpu import DEV, cl
    dev = lambda t: None if t is None else t.to(DEV)
    return ops.Lazy(cl(d["raw"], dt), dev(d["scale"]), dev(d["shift"]), variant != "p", SLOPE, keep=None if d["keep"] is None else cl(d["keep"], torch.uint8),
                    keep_scale=KEEP_SCALE, chan_mul=dev(d["cm"]))


def _lazy_ref(d, variant):
    from tests import kernel_ref as kr
    return kr.lazy_f32(d["raw"], scale=d["scale"], shift=d["shift"], act=variant != "p", slope=SLOPE, keep=d["keep"], keep_scale=KEEP_SCALE, chan_mul=d["cm"])


def _bits(t):
    t = t.contiguous()
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype]).cpu().numpy()


def _guarded(shape, dt, fill=float("nan")):
    """a tensor of `shape` inside a NaN-filled buffer with GUARD elements on either side: (buffer, view)"""
    from tests.test_kernels_gpu import DEV
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dt)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_ok(buf, n, nan=True):
    edge = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return np.array(bool((torch.isnan(edge) if nan else edge == 0xAB).all()))


def _run_pool(name):
    from chap_amd import ops
    (N, D, H, W), C, dtype, variant, want_idx, special = POOL_ALL[name]
    dt, d = _DT[dtype], _source(name, (N, D, H, W), C, variant, special)
    oshape = (N, max(D // 2, 1), H // 2, W // 2, C)
    buf, out = _guarded(oshape, dt)
    ibuf, idx = _guarded(oshape, torch.uint8, 0xAB) if want_idx else (None, None)
    ops.act_pool2(_lazy(d, variant, dt), out, idx, dims=3 if D > 1 else 2)
    torch.cuda.synchronize()
    res = dict(out=_bits(out), guards=_guards_ok(buf, out.numel()))
    if want_idx:
        res.update(idx=_bits(idx), idx_guards=_guards_ok(ibuf, idx.numel(), nan=False))
    return res


def _run_up(name):
    from chap_amd import ops
    (N, D, H, W), C, dtype, variant, dims, hp, slot = UP_ALL[name]
    dt, d = _DT[dtype], _source(name, (N, D, H, W), C, variant)
    ld = 2 * C if slot else C
    buf, out = _guarded((N, 2 * D if dims == 3 else D, 2 * H, 2 * W, ld), dt)
    ops.upsample2x(_lazy(d, variant, dt), out, dims=dims, out_coff=C if slot else 0, half_pixel=bool(hp))
    torch.cuda.synchronize()
    return dict(out=_bits(out[..., ld - C:]), guards=_guards_ok(buf, out.numel()),
                slot_nan=np.array(bool(torch.isnan(out[..., :ld - C]).all())))


def _run_chansum(name):
    from chap_amd import ops
    from tests.test_kernels_gpu import DEV
    shape, C, dtype, variant = CHANSUM[name]
    dt, d = _DT[dtype], _source(name, shape, C, variant)
    buf, out = _guarded((C,), torch.float32)
    out.copy_(d["prior"].to(DEV))
    ops.channel_sum(_lazy(d, variant, dt), out)
    torch.cuda.synchronize()
    return dict(out=_bits(out), guards=_guards_ok(buf, C))


def _wgrad_case(name):
    from tests import k3_conv_cases as kc
    case, dtn, blocks = WGRAD[name][:3]
    c = dict(kc.BY_NAME[case], **(WGRAD[name][4] if len(WGRAD[name]) > 4 else {}))
    return c, dtn, dict(c["knobs"], **({"CHAP_WGRAD_BLOCKS": blocks} if blocks else {}))


def _run_wgrad(name):
    from chap_amd import ops
    from tests import k3_conv_cases as kc
    from tests.test_k3_conv_families_gpu import sources
    from tests.test_kernels_gpu import DEV
    c, dtn, knobs = _wgrad_case(name)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in knobs.items()})
    dtype = kc.DTYPES[dtn]
    inp = kc.wgrad_inputs(c, dtn)
    As, B = sources(c, inp["As"], dtype), sources(c, [inp["B"]], dtype)[0]
    buf, dw = _guarded(tuple(inp["prior_dw"].shape), torch.float32)
    dw.copy_(inp["prior_dw"])
    res = {}
    dbuf = db = None
    if c["db"]:
        dbuf, db = _guarded((inp["knv"],), torch.float32)
        db.copy_(inp["prior_db"])
    D, H, W = kc.spatial(c)
    ops.wgrad(As, B, dw, inp["strides"], grid=(c["N"], D, H, W), in_dims=(D, H, W), ksize=3, stride=1, dims=c["dims"], combine=int(c["arr"] == "add"),
              db=db, kc_valid=c["kc_valid"], kn_valid=c["kn_valid"])
    torch.cuda.synchronize()
    for k in knobs:
        os.environ.pop(k, None)
    res.update(dw=_bits(dw), guards=_guards_ok(buf, dw.numel()))
    if c["db"]:
        res.update(db=_bits(db), db_guards=_guards_ok(dbuf, db.numel()))
    return res


def _run(name):
    return (_run_pool if name in POOL_ALL else _run_up if name in UP_ALL else _run_chansum if name in CHANSUM else _run_wgrad)(name)


OUTPUTS = ("out", "idx", "dw", "db")


def _fixture_form(a):
    """what the golden file keeps of an output: the array, or the digest of its bytes"""
    return a if a.nbytes <= BIG else np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _main(argv):
    """child process: every case of a set into one .npz (--golden: the fixture form of the outputs only)"""
    out, which = argv[argv.index("--out") + 1], argv[argv.index("--set") + 1]
    res = {}
    for name in SETS[which]:
        for k, v in _run(name).items():
            if k in OUTPUTS:
                res[name + "/" + k] = _fixture_form(v)
                if "--golden" not in argv:
                    res[name + "/" + k + "#full"] = v
            elif "--golden" not in argv:
                res[name + "/" + k] = v
    np.savez_compressed(out, **res)


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    """{case/key: array} of what one fresh process per set computed, and the parent's"""
    got, gold = {}, {}
    for which in sorted(SETS):
        out = str(tmp_path_factory.mktemp("pointwise_loads") / (which + ".npz"))
        env = dict({k: v for k, v in os.environ.items() if k not in KNOBS and k != "CHAP_GRID_SCALE"}, **SET_ENV[which])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--set", which, "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got.update(np.load(out))
        gold.update(np.load(os.path.join(GOLDEN, which + ".npz")))
    return got, gold


@pytest.mark.parametrize("name", ALL)
def test_bits_of_the_parent(computed, name):
    """every output equals the parent build's, bit for bit; nothing written outside it"""
    got, gold = computed
    keys = [k.split("/")[1] for k in gold if k.split("/")[0] == name]
    assert keys and sorted(keys) == sorted(k.split("/")[1] for k in got if k.split("/")[0] == name and k.split("/")[1] in OUTPUTS), keys
    for k in keys:
        a, b = got[name + "/" + k], gold[name + "/" + k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), "%s %s: %d of %d elements differ from the parent's" % (name, k, int((a != b).sum()), a.size)
    for k in ("guards", "idx_guards", "db_guards", "slot_nan"):
        assert bool(got.get(name + "/" + k, True)), "%s: %s: written outside the output" % (name, k)


def _nc(a, dt, shape):
    """stored bits [N, D, H, W, C] -> NCDHW fp64"""
    t = torch.from_numpy(a.copy()).view(dt).reshape(shape)
    return t.double().permute(0, 4, 1, 2, 3).contiguous()


def _v5(t):
    return t if t.dim() == 5 else t.unsqueeze(2)


@pytest.mark.parametrize("name", sorted(POOL_ALL))
def test_pool_fp64(computed, name):
    from tests import kernel_ref as kr
    got, _ = computed
    (N, D, H, W), C, dtype, variant, want_idx, special = POOL_ALL[name]
    dt, d = _DT[dtype], _source(name, (N, D, H, W), C, variant, special)
    v, dv = (_v5(t) for t in _lazy_ref(d, variant))
    k = (2, 2, 2) if D > 1 else (1, 2, 2)
    nanw = F.max_pool3d(torch.isnan(v).double(), k) > 0                     # windows with a NaN: the output is NaN
    ref = F.max_pool3d(torch.nan_to_num(v, nan=-1e30), k)
    oshape = (N, max(D // 2, 1), H // 2, W // 2, C)
    o = _nc(got[name + "/out#full"], dt, oshape)
    assert bool((torch.isnan(o) == nanw).all()), name + ": NaN windows"
    z = torch.zeros_like(ref)
    w = [kr.check("act_pool2 out", torch.where(nanw, z, o), torch.where(nanw, z, ref), kr.bound(ref, extra=F.max_pool3d(torch.nan_to_num(dv), k), store=dt))]
    if want_idx:                                            # the index names the FIRST sample that holds the stored maximum (or the last NaN)
        idx = torch.from_numpy(got[name + "/idx#full"].copy()).reshape(oshape).permute(0, 4, 1, 2, 3).long()
        assert int(idx.max()) < (8 if D > 1 else 4)
        kz, ky, kx = idx >> 2, (idx >> 1) & 1, idx & 1
        oz, oy, ox = torch.meshgrid(torch.arange(oshape[1]), torch.arange(oshape[2]), torch.arange(oshape[3]), indexing="ij")
        picked = v[torch.arange(N)[:, None, None, None, None], torch.arange(C)[None, :, None, None, None],
                   (k[0] * oz + kz), 2 * oy + ky, 2 * ox + kx]
        assert bool((torch.isnan(picked) == nanw).all()), name + ": the index of a NaN window names a NaN"
        # the sample the index names is a maximum of its window within the source's own bound
        assert bool(((ref - picked)[~nanw].abs() <= 2 * F.max_pool3d(torch.nan_to_num(dv), k)[~nanw]).all()), name + ": idx does not name a maximum"
        if special == "tie" and variant == "p":             # exact values: the first of the equal maxima
            first = torch.full_like(idx, 99)
            for kk in reversed(range(8 if D > 1 else 4)):
                s = v[:, :, (kk >> 2)::k[0], ((kk >> 1) & 1)::2, (kk & 1)::2]
                first = torch.where(s == ref, torch.full_like(idx, kk), first)
            assert bool((first == idx).all()), name + ": not the first maximum"
    print("pointwise %s: worst err/bound %s" % (name, " ".join("%.3f" % x for x in w)))


def _interp(t, dims, hp):
    y = F.interpolate(t if dims == 3 else t[:, :, 0], scale_factor=2, mode="trilinear" if dims == 3 else "bilinear", align_corners=not hp)
    return y if dims == 3 else y.unsqueeze(2)


@pytest.mark.parametrize("name", sorted(UP_ALL))
def test_upsample_fp64(computed, name):
    """bounds of Checker.upsample2x (tests/test_step_launches_gpu.py)"""
    from tests import kernel_ref as kr
    got, _ = computed
    (N, D, H, W), C, dtype, variant, dims, hp, slot = UP_ALL[name]
    dt, d = _DT[dtype], _source(name, (N, D, H, W), C, variant)
    v, dv = (_v5(t) for t in _lazy_ref(d, variant))
    ref = _interp(v, dims, bool(hp))
    vmax = v.abs().amax(dim=(2, 3, 4), keepdim=True)
    extra = _interp(dv, dims, bool(hp)) + 8 * kr.U32 * max(v.shape[2:]) * vmax
    o = _nc(got[name + "/out#full"], dt, (N, 2 * D if dims == 3 else D, 2 * H, 2 * W, C))
    w = kr.check("upsample2x out", o, ref, kr.bound(ref, sabs=_interp(v.abs(), dims, bool(hp)), chain=8, extra=extra, store=dt))
    print("pointwise %s: worst err/bound %.3f" % (name, w))


@pytest.mark.parametrize("name", sorted(CHANSUM))
def test_channel_sum_fp64(computed, name):
    from tests import kernel_ref as kr
    got, _ = computed
    shape, C, dtype, variant = CHANSUM[name]
    d = _source(name, shape, C, variant)
    ref, b = kr.channel_sum_ref(_lazy_ref(d, variant), d["prior"])
    w = kr.check("channel_sum", torch.from_numpy(got[name + "/out#full"].copy()).view(torch.float32), ref, b, "c")
    if name == "sum_trips_c512_bf16_a":
        assert -(-int(np.prod(shape)) // (256 // (C // 8))) > CHANSUM_SLOTS      # more block steps than blocks
    print("pointwise %s: worst err/bound %.3f" % (name, w))


@pytest.mark.parametrize("name", sorted(WGRAD))
def test_wgrad_fp64(computed, name):
    from tests import k3_conv_cases as kc
    got, _ = computed
    c, dtn, _ = _wgrad_case(name)
    inp = kc.wgrad_inputs(c, dtn)
    f = lambda k, shape: torch.from_numpy(got[name + "/" + k + "#full"].copy()).view(torch.float32).reshape(shape)
    w = kc.wgrad_check(c, dtn, kc.wgrad_reference(c, dtn, inp), inp, f("dw", tuple(inp["prior_dw"].shape)), f("db", (inp["knv"],)) if c["db"] else None)
    print("pointwise %s: worst err/bound %s" % (name, " ".join("%.3f" % x for x in w)))


def test_wgrad_split_counts(probe):
    """the slab counts the cases are chosen for, from the planner itself: both reduce instances (64 slabs and more: <8>), and for <64>, whose four
    thread groups take four slabs each per trip, counts below, at and above 4 and 16"""
    from tests import k3_conv_cases as kc
    seen = set()
    for name in sorted(WGRAD):
        c, dtn, knobs = _wgrad_case(name)
        req = (["setenv " + " ".join("%s=%s" % kv for kv in knobs.items())] if knobs else []) + [kc.wgrad_request(c, dtn)]
        r = probe(req)[0]
        assert r["rc"] == 0, (name, r)
        want = WGRAD[name][3]
        assert want is None or r["nsplit"] == want, (name, r["nsplit"], want)
        seen.add(r["nsplit"])
    assert {1, 4, 5, 16} <= seen and any(4 < n < 16 for n in seen) and any(16 < n < 64 for n in seen) and any(n >= 64 for n in seen), sorted(seen)


if __name__ == "__main__":
    _main(sys.argv[1:])
