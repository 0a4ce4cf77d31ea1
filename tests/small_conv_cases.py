"""The small ragged cases of the conv families next to the 3x3 kernels -- 1x1(x1), k2 s2 (2D, 3D), 1x1 + depth-to-space, the V-Net head kernel, the
k1 / k2 s2 weight gradients -- as ONE host-only table (a helper module, not a conftest).  tests/test_small_conv_cases_cpu.py checks, with the planner
probe (tests/plan_probe.py), that every case reaches the kernel instance it names and that the table covers the instances the bench-shaped steps launch
(tests/golden/launch_plan_parent.csv); tests/test_small_conv_families_gpu.py runs every case once on the GPU.  Both go through the same inputs, the same
fp64 references (tests/kernel_ref.py) and the same checks below: the CPU file feeds them an fp32 torch emulation of the kernel (and emulations with one
planted fault each, which must fail), the GPU file the kernel's output.

Only the shape selects the instance of these families (CHAP_CONV_NT / CHAP_CONV_MR apply to the k3 s1 layers): every grid below is the smallest found
with the probe that reaches its plan and is ragged against the instance's pixel tile (4 MR x 16; weight gradient 8 x 16, 4 x 16 for 3D k2 s2)."""
import itertools
import math

import torch

from tests import kernel_ref as kr

F32, BF16 = 0, 1                                           # chap_hip.h CHAP_F32 / CHAP_BF16
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_ID = {"f32": F32, "bf16": BF16}
SLOT_COFF, SLOT_EXTRA, GUARD = 8, 16, 512                  # outputs sit at channel 8 of a buffer 16 channels wider, 512 guard elements behind it
SRC_COFF, SRC_EXTRA = 8, 16                                # a `slice` source: channels [8, 8 + C) of a buffer 16 channels wider, NaN elsewhere
KEEP_P, KEEP_SCALE, SLOPE = 0.25, 1.0 / 0.75, 0.01


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
# forward: op k1 = 1x1(x1), k2 = k2 s2, d2s = 1x1 + depth-to-space (cout = real channels out_Cn; the launch's Cout is 2^dims * cout), head = planar
# fp32 logits.  grid = the OUTPUT grid of the launch (d2s: the coarse grid).  src kinds (one per source): p plain, ar BatchNorm affine + LeakyReLU,
# ark ar + element keep mask (2D), arm ar + per-sample channel multipliers, sl plain channel slice of a NaN buffer.  plan = (KC, NT, MR);
# chunks = K chunks; wlds = resident weights per dtype name (None: not pinned); route: generic / head per dtype.
def _fwd(name, op, dims, N, grid, cin, cout, plan, kind, src, bias=True, stats=False, chunks=None, wlds=None, route=None):
    cin = cin if isinstance(cin, tuple) else (cin,)
    src = src if isinstance(src, tuple) else (src,)
    assert len(cin) == len(src)
    return dict(name=name, op=op, dims=dims, N=N, grid=tuple(grid), cin=cin, cout=cout, plan=plan, kind=kind, src=src, bias=bias, stats=stats,
                chunks=chunks, wlds=wlds, route=route or {"f32": "generic", "bf16": "generic"})


CF, CD, DF, DD, WD = kr.PACK_CONV_FWD, kr.PACK_CONV_DGRAD, kr.PACK_DECONV_FWD, kr.PACK_DECONV_DGRAD, kr.PACK_DOWN_DGRAD
G2, G3, G3S = (9, 21), (3, 5, 19), (3, 5, 7)
RES, NONRES = {"f32": True, "bf16": True}, {"f32": False, "bf16": False}

FWD_CASES = [
    # ---- 1x1(x1)
    _fwd("k1_3d_16_16", "k1", 3, 1, (6, 58, 122), 16, 16, (16, 1, 2), CF, "arm", stats=True),
    _fwd("k1_16_32", "k1", 2, 3, (58, 250), 16, 32, (16, 2, 2), CF, "ark", stats=True),
    _fwd("k1_16_48", "k1", 2, 3, (58, 250), 16, 48, (16, 2, 2), CD, "sl", stats=True),
    _fwd("k1_32_16", "k1", 2, 3, (58, 250), 32, 16, (32, 1, 2), CF, "ar", stats=True),
    _fwd("k1_64_16", "k1", 2, 2, (10, 18), 64, 16, (32, 1, 1), CD, "ark", bias=False, wlds=RES),
    _fwd("k1_64_32", "k1", 2, 3, (58, 250), 64, 32, (32, 2, 2), CF, "sl", bias=False),
    _fwd("k1_64_96", "k1", 2, 3, (58, 250), 64, 96, (32, 4, 2), CF, "p", stats=True),
    _fwd("k1_64_128", "k1", 2, 4, (30, 122), 64, 128, (32, 4, 1), CF, "ar", stats=True),
    _fwd("k1_3d_32_64", "k1", 3, 2, (3, 10, 18), 32, 64, (32, 1, 1), CF, "arm", stats=True),
    _fwd("k1_cat_16_32_32", "k1", 2, 2, (10, 18), (16, 32), 32, (16, 1, 1), CF, ("ar", "p"), chunks=3),
    # 23 chunks of 16 channels x 4 tiles: the first 1x1 whose weights do not fit the 100 KB beside the halo buffers (staged per chunk)
    _fwd("k1_368_128", "k1", 2, 4, (30, 122), 368, 128, (16, 4, 1), CF, "p", bias=False, chunks=23, wlds=NONRES),
    # ---- 2D k2 s2, output grid 9 x 21, N = 2
    _fwd("k2_16_16", "k2", 2, 2, G2, 16, 16, (16, 1, 2), CF, "ar", stats=True, wlds=RES),
    _fwd("k2_16_32", "k2", 2, 2, G2, 16, 32, (16, 2, 2), DD, "p", bias=False, stats=True),
    _fwd("k2_16_64", "k2", 2, 2, G2, 16, 64, (16, 4, 2), CF, "ark", stats=True),
    _fwd("k2_32_16", "k2", 2, 2, G2, 32, 16, (32, 1, 2), CF, "sl"),
    _fwd("k2_32_32", "k2", 2, 2, G2, 32, 32, (32, 2, 2), CF, "ark"),
    _fwd("k2_64_96", "k2", 2, 2, G2, 64, 96, (32, 4, 2), CF, "ar", stats=True),
    _fwd("k2_48_32", "k2", 2, 2, G2, 48, 32, (16, 2, 2), DD, "sl", bias=False, chunks=3),
    _fwd("k2_128_256", "k2", 2, 2, G2, 128, 256, (32, 4, 2), CF, "p", chunks=4, wlds=NONRES),
    # ---- 3D k2 s2, output grid 3 x 5 x 19
    _fwd("k2_3d_16_16", "k2", 3, 2, G3, 16, 16, (16, 1, 1), CF, "arm", stats=True, wlds=RES),
    _fwd("k2_3d_16_32", "k2", 3, 2, G3, 16, 32, (16, 2, 1), CF, "ar", stats=True),
    _fwd("k2_3d_16_48", "k2", 3, 2, G3, 16, 48, (16, 2, 1), CF, "sl", stats=True),
    _fwd("k2_3d_16_64", "k2", 3, 2, G3, 16, 64, (16, 4, 1), DD, "p", bias=False, stats=True),
    _fwd("k2_3d_32_16", "k2", 3, 2, G3, 32, 16, (32, 1, 1), CF, "sl"),
    _fwd("k2_3d_32_32", "k2", 3, 2, G3, 32, 32, (32, 2, 1), CF, "arm"),
    _fwd("k2_3d_32_64", "k2", 3, 2, G3, 32, 64, (32, 4, 1), CF, "ar", stats=True, wlds={"f32": False, "bf16": True}),
    _fwd("k2_3d_64_96", "k2", 3, 2, G3, 64, 96, (32, 4, 1), CF, "p", stats=True),
    _fwd("k2_3d_64_128", "k2", 3, 2, G3, 64, 128, (32, 4, 1), DD, "p", bias=False),
    _fwd("k2_3d_48_32", "k2", 3, 2, G3, 48, 32, (16, 2, 1), CF, "arm", chunks=3),
    _fwd("k2_3d_128_256", "k2", 3, 2, G3, 128, 256, (32, 4, 1), CF, "ar", stats=True, chunks=4, wlds=NONRES),
    # ---- 1x1 + depth-to-space (cout = out_Cn), into a channel slot of a wider buffer
    _fwd("d2s_3d_256_128", "d2s", 3, 2, (5, 7, 7), 256, 128, (32, 2, 1), DF, "arm", stats=True),
    _fwd("d2s_128_64_mr2", "d2s", 2, 2, (26, 186), 128, 64, (32, 4, 2), DF, "ar", stats=True, chunks=4),
    _fwd("d2s_128_64_mr1", "d2s", 2, 2, (18, 150), 128, 64, (32, 4, 1), DF, "ark", stats=True, chunks=4),
    _fwd("d2s_32_16_mr1", "d2s", 2, 3, (30, 250), 32, 16, (32, 4, 1), WD, "sl", bias=False, chunks=1),
    _fwd("d2s_16_48", "d2s", 2, 3, (18, 150), 16, 48, (16, 4, 1), WD, "p", bias=False, stats=True),
    _fwd("d2s_3d_256_128_mr2", "d2s", 3, 2, (3, 10, 26), 256, 128, (32, 4, 2), DF, "ar", stats=True, chunks=8),
    _fwd("d2s_3d_256_128_mr1", "d2s", 3, 2, (3, 6, 26), 256, 128, (32, 4, 1), WD, "sl", bias=False, chunks=8),
    _fwd("d2s_3d_16_16", "d2s", 3, 2, (4, 10, 122), 16, 16, (16, 4, 1), WD, "arm", stats=True),
]

# the head route (bf16: conv_head1x1_kernel; fp32: the generic 1x1 kernel with planar stores, the cross-check of the same weights): 16 channels to
# 1 .. 8 classes; `straddle`: N = 3 with 3 * 7 * 23 = 483 voxels per sample, so 256-thread blocks straddle samples with different multipliers;
# `second_trip`: 4096 * 256 + 2 * 1047 voxels, the kernel's grid is capped at 4096 blocks
HEAD = {"f32": "generic", "bf16": "head"}
HEAD_CASES = [
    _fwd("head_c1", "head", 2, 2, (10, 18), 16, 1, (16, 1, 1), CF, "ar", route=HEAD),
    _fwd("head_c2", "head", 3, 1, (6, 10, 12), 16, 2, (16, 1, 1), CF, "p", route=HEAD),
    _fwd("head_c3_straddle", "head", 3, 3, (3, 7, 23), 16, 3, (16, 1, 1), CF, "arm", route=HEAD),
    _fwd("head_c5", "head", 2, 3, (7, 23), 16, 5, (16, 1, 1), CF, "arm", bias=False, route=HEAD),
    _fwd("head_c8", "head", 3, 2, (3, 5, 19), 16, 8, (16, 1, 1), CF, "sl", route=HEAD),
    _fwd("head_c2_second_trip", "head", 3, 2, (5, 349, 301), 16, 2, (16, 1, 2), CF, "ar", route=HEAD),
]
SECOND_TRIP = "head_c2_second_trip"


# weight gradients: ks 1 / 2 (k2 s2); grid = the grid of B (k2: the coarse grid, A is twice as fine); plan = {dtype name: (KC, bn)}; A / B: source kinds;
# role: conv (A = the layer's input, B = its output gradient) or deconv (A = the fine gradient, B = the coarse lazy input); kn_valid: live B channels
def _wg(name, ks, dims, N, grid, ca, cb, plan, A="p", B="p", db=False, kn_valid=0, role="conv"):
    plan = plan if isinstance(plan, dict) else {"f32": plan, "bf16": plan}
    return dict(name=name, ks=ks, dims=dims, N=N, grid=tuple(grid), ca=ca, cb=cb, plan=plan, A=A, B=B, db=db, kn_valid=kn_valid, role=role)


K2F = lambda kc, bn: {"f32": (16, bn), "bf16": (kc, bn)}    # fp32 k2 s2: KC is forced to 16 (wgrad_plan.h)
# (db on a deconv case: the bias gradient of a LAZY B, summed from its fp32 value -- kernel_ref.wgrad_ref(Bv=); the training step never asks for it there)
WGRAD_CASES = [
    _wg("wg_k1_3d_16_16", 1, 3, 1, (3, 11, 21), 16, 16, (16, 16), A="arm", db=True, kn_valid=2),
    _wg("wg_k1_3d_16_16_n2", 1, 3, 2, (3, 11, 21), 16, 16, (16, 16), A="arm", db=True),
    _wg("wg_k1_32_16", 1, 2, 2, (11, 21), 32, 16, (32, 16), A="ar", db=True),
    _wg("wg_k1_48_40", 1, 2, 2, (11, 21), 48, 40, (16, 32), A="ark", db=True),
    _wg("wg_k1_128_64", 1, 2, 2, (11, 21), 128, 64, (32, 32), A="sl"),
    _wg("wg_k2_16_32", 2, 2, 2, G2, 16, 32, K2F(16, 32), B="ar", db=True, role="deconv"),
    _wg("wg_k2_32_16", 2, 2, 2, G2, 32, 16, K2F(32, 16), A="ark", db=True),
    _wg("wg_k2_64_128", 2, 2, 2, G2, 64, 128, K2F(32, 32), B="ar", role="deconv"),
    _wg("wg_k2_3d_16_32", 2, 3, 2, G3, 16, 32, K2F(16, 32), A="arm", db=True),
    _wg("wg_k2_3d_32_16", 2, 3, 2, G3S, 32, 16, K2F(32, 16), B="arm", db=True, role="deconv"),
    _wg("wg_k2_3d_128_256", 2, 3, 2, G3S, 128, 256, K2F(32, 32), B="ar", role="deconv"),
    _wg("wg_k2_3d_32_64", 2, 3, 2, G3, 32, 64, K2F(32, 32), A="ar", db=True),
]

ALL_FWD = FWD_CASES + HEAD_CASES
BY_NAME = {c["name"]: c for c in ALL_FWD + WGRAD_CASES}
assert len(BY_NAME) == len(ALL_FWD) + len(WGRAD_CASES)


# ---- planner requests (the request lines of tests/plan_probe.py) ----------------------------------------------------------------------------------------
def _sp(c):
    g = c["grid"]
    return dict(zip("DHW", g)) if len(g) == 3 else dict(D=1, H=g[0], W=g[1])


def launch_cout(c):
    return c["cout"] * 2 ** c["dims"] if c["op"] == "d2s" else c["cout"]


def fwd_request(c, dt):
    k = 2 if c["op"] == "k2" else 1
    f = dict(dims=c["dims"], k=k, s=k, N=c["N"], Cout=launch_cout(c), nsrc=len(c["cin"]), C0=c["cin"][0], C1=c["cin"][1] if len(c["cin"]) > 1 else 0,
             dtype=DTYPE_ID[dt], d2s=int(c["op"] == "d2s"), Cn=c["cout"] if c["op"] == "d2s" else 0, planar=int(c["op"] == "head"),
             f32out=int(c["op"] == "head"), stats=int(c["stats"]), **_sp(c))
    for i, s in enumerate(c["src"]):
        f["keep%d" % i], f["cm%d" % i] = int(s == "ark"), int(s == "arm")
        if s == "sl" and i == 0:
            f["ld0"] = c["cin"][0] + SRC_EXTRA
    return "conv " + " ".join("%s=%s" % kv for kv in f.items())


def wgrad_request(c, dt):
    k = c["ks"]
    f = dict(dims=c["dims"], k=k, s=k, N=c["N"], Cb=c["cb"], na=1, C0=c["ca"], dtype=DTYPE_ID[dt], keep0=int(c["A"] == "ark"), cm0=int(c["A"] == "arm"), **_sp(c))
    return "wgrad " + " ".join("%s=%s" % kv for kv in f.items())


def conv_tile(c):
    """pixel tile (TH, TW) of the generic instance a forward case names, as conv_geom (conv_kernel.h) derives it from MR: 4 MR x 16"""
    return 4 * c["plan"][2], 16


def wgrad_tile(c):
    """wgrad_plan.h: 8 x 16 tiles, 4 x 16 for the 3D geometries with ksize >= 2"""
    return (4 if c["dims"] == 3 and c["ks"] >= 2 else 8), 16


def fwd_instance(c, dt):
    """the key of a conv_fwd_kernel instance: (dtype, KS, D3, KC, NT, MR)"""
    k = 2 if c["op"] == "k2" else 1
    return (dt, k, c["dims"] == 3 and k == 2) + tuple(c["plan"])


def wgrad_instance(c, dt):
    """the key of a wgrad_kernel instance: (dtype, KS, D3, KC, BN)"""
    return (dt, c["ks"], c["dims"] == 3 and c["ks"] == 2) + tuple(c["plan"][dt])


# ---- resident weights: launch_one (conv_dispatch.inc) restated ----------------------------------------------------------------------------------------
PIX_STRIDE = {(32, 2): 48, (32, 4): 36, (16, 2): 16, (16, 4): 20}       # conv_kernel.h lds_pix_stride: (KC, element bytes)
HALO_DUMMY, MAX_AFFINE_C = 8, 1024


def conv_lds(esize, KS, ST, D3, KC, NT, MR, ZW, nchunks):
    """(WLDS, dynamic LDS bytes) of a generic conv launch.  conv_geom: the halo of a 4 MR x 16 tile (ZW: a 4 x MR x 16 brick); conv_lds_fixed_bytes:
    two halo buffers and the block statistics, plus the affine cache; the weights of all K chunks stay resident while everything fits 100 KB (158 KB
    for the 3D instances); otherwise one chunk's weights are staged through one (bf16) or two (fp32) buffers when conv_wstaged says so."""
    TH, TD = (MR, 4) if ZW else (4 * MR, 1)
    KD, STD = (KS, ST) if D3 else (1, 1)
    HP = ((TD - 1) * STD + KD) * ((TH - 1) * ST + KS) * (15 * ST + KS)
    fixed = 2 * (HP * PIX_STRIDE[(KC, esize)] + HALO_DUMMY) * esize + 4 * 2 * 16 * NT * 4 + 2 * MAX_AFFINE_C * 4
    steps = (KD * KS * KS * (KC // 8) + 3) // 4
    wbytes = nchunks * steps * NT * 64 * 8 * esize
    wlds = fixed + wbytes <= (158 if D3 else 100) * 1024
    staged = (steps * NT + 3) // 4 <= 14 and fixed + 2 * steps * NT * 512 * esize <= 158 * 1024
    wst = (1 if esize == 2 else 2) * steps * NT * 512 * esize
    return wlds, fixed + (wbytes if wlds else (wst if staged else 0))


def case_lds(c, dt):
    k = 2 if c["op"] == "k2" else 1
    KC, NT, MR = c["plan"]
    return conv_lds(2 if dt == "bf16" else 4, k, k, c["dims"] == 3 and k == 2, KC, NT, MR, False, sum(c["cin"]) // KC)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def _rq(x, dtype):
    return x.to(dtype).float()


LANE_SEED = 100003                                         # lane k of a merged-grid case (tests/group_cases.py): the same shapes, another draw


def _gen(c, dt, lane=0):
    return torch.Generator().manual_seed(sum(map(ord, c["name"])) * 2 + DTYPE_ID[dt] + LANE_SEED * lane)


def make_source(kind, N, C, sp, dtype, g):
    """one source of `kind`: dict(x [N, C, *sp] in the storage type's values, and the lazy transform's arguments as kernel_ref.lazy_f32 names them)"""
    s = dict(kind=kind, x=_rq(torch.randn(N, C, *sp, generator=g), dtype), lazy={})
    if kind in ("ar", "ark", "arm"):
        s["lazy"].update(scale=torch.rand(C, generator=g) + 0.5, shift=torch.randn(C, generator=g) * 0.2, act=True, slope=SLOPE)
    if kind == "ark":
        s["lazy"].update(keep=(torch.rand(N, C, *sp, generator=g) > KEEP_P).float(), keep_scale=KEEP_SCALE)
    if kind == "arm":                                      # Dropout3d multipliers, another draw per sample
        cm = (torch.rand(N, C, generator=g) > 0.3).float() * 1.5
        cm[:, 0] = torch.arange(N) % 2 * 1.5               # channel 0: dropped in even samples, kept in odd ones
        s["lazy"].update(chan_mul=cm)
    return s


def source_operand(s, dtype, chan_mul_of_sample0=False, raw=False):
    """(MFMA operand, flip) of a source; the two switches are the planted faults of the emulation"""
    lazy = {} if raw else dict(s["lazy"])
    if chan_mul_of_sample0 and "chan_mul" in lazy:
        lazy["chan_mul"] = lazy["chan_mul"][:1].expand_as(lazy["chan_mul"])
    return kr.operand(s["x"], dtype, **lazy)


def weight_shape(kind, K, M, dims, op):
    """checkpoint layout of the weight of a launch with K input and M (real) output channels"""
    k = (1 if op in ("k1", "head") else 2,) * dims
    # CONV_FWD w [cout, cin, k..] and DECONV_DGRAD w [cin, cout, 2..] put the launch's OUTPUT channels first; CONV_DGRAD w [cout, cin, k..], DECONV_FWD
    # w [cin, cout, 2..] and DOWN_DGRAD w [cout, cin, 2..] its input channels (kernel_ref.conv_linear)
    return ((M, K) if kind in (kr.PACK_CONV_FWD, kr.PACK_DECONV_DGRAD) else (K, M)) + k


def pack_args(c):
    """(Cin, Cout, taps) of chap_pack_weights for the case's weight"""
    K, M, taps = sum(c["cin"]), c["cout"], (1 if c["op"] in ("k1", "head") else 2 ** c["dims"])
    return (K, M, taps) if c["kind"] in (kr.PACK_CONV_FWD, kr.PACK_DECONV_FWD) else (M, K, taps)


def in_spatial(c):
    return tuple(2 * s for s in c["grid"]) if c["op"] == "k2" else c["grid"]


def out_spatial(c):
    return tuple(2 * s for s in c["grid"]) if c["op"] == "d2s" else c["grid"]


def fwd_inputs(c, dt, lane=0):
    dtype, g = DTYPES[dt], _gen(c, dt, lane)
    K, M = sum(c["cin"]), c["cout"]
    srcs = [make_source(kd, c["N"], ci, in_spatial(c), dtype, g) for kd, ci in zip(c["src"], c["cin"])]
    taps = 1 if c["op"] in ("k1", "head", "d2s") else 2 ** c["dims"]
    w = torch.randn(weight_shape(c["kind"], K, M, c["dims"], c["op"]), generator=g) / math.sqrt(K * taps)
    bias = torch.randn(M, generator=g) if c["bias"] else None
    shift = torch.randn(M, generator=g) * 0.3 if c["stats"] else None
    return dict(srcs=srcs, w=w, bias=bias, shift=shift)


def fwd_reference(c, dt, inp):
    """the fp64 restatement: conv_ref's dict, plus stats = ((S, bound), (Q, bound)) where the case takes statistics"""
    dtype = DTYPES[dt]
    ops_ = [source_operand(s, dtype) for s in inp["srcs"]]
    a, flip = torch.cat([o[0] for o in ops_], 1), torch.cat([o[1] for o in ops_], 1)
    r = kr.conv_ref(c["kind"], a, kr.weight_operand(inp["w"], dtype), inp["bias"], flip=flip)
    r["stats"] = kr.stats_ref(r, inp["shift"]) if c["stats"] else None
    return r


# ---- the output buffer: a channel slot of a wider channel-last buffer, NaN everywhere else, a guard behind it ------------------------------------------------
def out_layout(c):
    """(shape of the output view, first channel of the slot, elements of the flat buffer).  The head writes planar fp32 [N, C, *sp]."""
    sp = out_spatial(c)
    sp5 = sp if len(sp) == 3 else (1,) + sp
    if c["op"] == "head":
        shape = (c["N"], c["cout"]) + sp
        return shape, 0, math.prod(shape) + GUARD
    shape = (c["N"],) + sp5 + (c["cout"] + SLOT_EXTRA,)
    return shape, SLOT_COFF, math.prod(shape) + GUARD


def new_out(c, dtype, device="cpu"):
    shape, coff, numel = out_layout(c)
    flat = torch.full((numel,), float("nan"), dtype=torch.float32 if c["op"] == "head" else dtype, device=device)
    return flat, flat[:numel - GUARD].view(shape)


def split_out(c, flat):
    """flat buffer (CPU) -> (the slot as NC(D)HW fp32, True where every element outside the slot still holds its NaN bits)"""
    shape, coff, numel = out_layout(c)
    view = flat[:numel - GUARD].view(shape)
    bits = flat.view(torch.int32 if flat.element_size() == 4 else torch.int16)
    fresh = torch.full((1,), float("nan"), dtype=flat.dtype).view(bits.dtype)
    outside = torch.ones(numel, dtype=torch.bool)
    if c["op"] == "head":
        outside[:numel - GUARD] = False
        got = view.float()
    else:
        m = outside[:numel - GUARD].view(shape)
        m[..., coff:coff + c["cout"]] = False
        got = view[..., coff:coff + c["cout"]].float().permute(0, 4, 1, 2, 3)
        if c["dims"] == 2:
            got = got.squeeze(2)
    return got.contiguous(), bool((bits[outside] == fresh).all())


def fwd_check(c, dt, r, flat, stats):
    """the checks of a forward case, for the kernel and for its emulation alike: per element under conv_bound, the statistics under stats_ref's
    bounds, the NaN canaries.  flat: the output buffer on the CPU; stats: [2, real channels] totals or None.  Returns the worst error / bound of each."""
    got, intact = split_out(c, flat)
    store = torch.float32 if c["op"] == "head" else DTYPES[dt]
    worst = [kr.check(c["name"] + " out", got, r["y"], kr.conv_bound(r, store))]
    assert intact, c["name"] + ": an element outside the output slot was written"
    if c["stats"]:
        (s1, b1), (s2, b2) = r["stats"]
        worst += [kr.check(c["name"] + " stats S", stats[0], s1, b1, dims="c"), kr.check(c["name"] + " stats Q", stats[1], s2, b2, dims="c")]
    return worst


# ---- the fp32 emulation of the forward kernels, with the planted faults ---------------------------------------------------------------------------------
FWD_FAULTS = ("d2s_xy_swapped", "bias_not_folded", "tile_tail_stored", "stats_ragged_columns", "last_column_dropped", "k2_taps_transposed",
              "chan_mul_of_sample0")


def fwd_emulate(c, dt, inp, fault=None):
    """What the kernel does, in fp32 torch: the lazy operands rounded to the MFMA operand type, the products summed in fp32 (another order than the
    kernel's), bias, statistics of the unrounded value, one rounding into the slot.  fault: one of FWD_FAULTS.  Returns (flat buffer, stats or None)."""
    dtype, dims = DTYPES[dt], c["dims"]
    ops_ = [source_operand(s, dtype, chan_mul_of_sample0=(fault == "chan_mul_of_sample0")) for s in inp["srcs"]]
    a = torch.cat([o[0] for o in ops_], 1).float()
    w = kr.weight_operand(inp["w"], dtype).float()
    if fault == "k2_taps_transposed":
        assert c["op"] == "k2"
        w = w.transpose(-1, -2)
    M = c["cout"]
    bias = inp["bias"].float() if inp["bias"] is not None else torch.zeros(M)
    bsh = [1, M] + [1] * dims
    if c["op"] == "d2s":                                   # a 1x1 conv to 2^dims * M channels (sub-position major; both kinds: w [K, M, 2..]), then depth-to-space
        y = a.new_zeros(a.shape[0], M, *[2 * s for s in a.shape[2:]])
        for j, t in enumerate(itertools.product(range(2), repeat=dims)):
            z = torch.einsum("nc...,co->no...", a, w[(slice(None), slice(None)) + t])
            z = z + (bias.view(bsh) if (fault != "bias_not_folded" or j == 0) else 0.0)       # the fault reads bias[c] at c = j * M + m: beyond the array
            if fault == "d2s_xy_swapped":
                t = t[:-2] + (t[-1], t[-2])
            y[(slice(None), slice(None)) + tuple(slice(t[i], None, 2) for i in range(dims))] = z
    else:
        assert fault not in ("d2s_xy_swapped", "bias_not_folded")
        y = kr.conv_linear(c["kind"], a, w) + bias.view(bsh)
    stats = None
    if c["stats"]:
        d = y.double() - inp["shift"].double().view(bsh)
        red = [0] + list(range(2, y.dim()))
        S, Q = d.sum(red), (d * d).sum(red)
        if fault == "stats_ragged_columns":                # the columns W .. 16 ceil(W / 16) of the last tile: no input there, the value is the bias
            W = c["grid"][-1]
            extra = (-W) % 16 * (y[:, 0].numel() // y.shape[-1]) * (2 if c["op"] == "d2s" else 1)
            assert extra > 0
            e = bias.double() - inp["shift"].double()
            S, Q = S + extra * e, Q + extra * e * e
        stats = torch.stack((S, Q))
    flat, view = new_out(c, dtype)
    if c["op"] == "head":
        view.copy_(y)
    else:
        ycl = (y if dims == 3 else y.unsqueeze(2)).permute(0, 2, 3, 4, 1)
        view[..., SLOT_COFF:SLOT_COFF + M] = ycl.to(dtype)
        if fault == "tile_tail_stored":                    # the tiles of the last block row beyond Cout land behind the slot
            KC, NT, MR = c["plan"]
            tail = 16 * NT * -(-launch_cout(c) // (16 * NT)) - launch_cout(c)
            assert tail > 0
            view[..., SLOT_COFF + M:SLOT_COFF + M + min(tail, SLOT_EXTRA - SLOT_COFF)] = 0
        if fault == "last_column_dropped":
            view[:, :, :, -1, SLOT_COFF:SLOT_COFF + M] = float("nan")
    return flat, stats


# ---- weight gradients -------------------------------------------------------------------------------------------------------------------------------------
def wgrad_inputs(c, dt, lane=0):
    dtype, g = DTYPES[dt], _gen(c, dt, lane)
    a_sp = tuple(c["ks"] * s for s in c["grid"])
    A = make_source(c["A"], c["N"], c["ca"], a_sp, dtype, g)
    B = make_source(c["B"], c["N"], c["cb"], c["grid"], dtype, g)
    knv = c["kn_valid"] or c["cb"]
    if knv != c["cb"]:
        B["x"][:, knv:] = 0                                # a head's gradient arrives zero-padded to 16 channels
    taps = c["ks"] ** c["dims"]
    prior_dw = torch.randn(knv, c["ca"], taps, generator=g) * 0.5
    prior_db = torch.randn(knv, generator=g) * 0.5 if c["db"] else None
    return dict(A=A, B=B, prior_dw=prior_dw, prior_db=prior_db, strides=(1, taps, c["ca"] * taps), knv=knv)


def wgrad_reference(c, dt, inp):
    dtype = DTYPES[dt]
    A, fA = source_operand(inp["A"], dtype)
    B, fB = source_operand(inp["B"], dtype)
    knv = inp["knv"]
    lazyB = {} if not inp["B"]["lazy"] else dict(zip(("Bv", "dBv"), (t[:, :knv] for t in kr.lazy_f32(inp["B"]["x"], **inp["B"]["lazy"]))))
    return kr.wgrad_ref(A, B[:, :knv], ksize=c["ks"], stride=c["ks"], flipA=fA, flipB=fB[:, :knv] if bool((fB != 0).any()) else None, **lazyB)


def wgrad_check(c, dt, rw, inp, dw, db):
    """dw [kn_valid, Ca, taps] and db after the accumulating launch, against prior + the fp64 total under wgrad_bound(prior=)"""
    st, shape = inp["strides"], tuple(inp["prior_dw"].shape)
    prior = inp["prior_dw"].double().as_strided(rw["dw"].shape, st)           # [taps, Ca, Cb] view of the prior, as wgrad_bound wants it
    ref = inp["prior_dw"].double() + kr.to_layout(rw["dw"], st, shape)
    worst = [kr.check(c["name"] + " dW", dw, ref, kr.to_layout(kr.wgrad_bound(rw, prior), st, shape), dims="kct")]
    if c["db"]:
        worst.append(kr.check(c["name"] + " db", db, inp["prior_db"].double() + rw["db"], kr.wgrad_bound(rw, inp["prior_db"], which="db"), dims="k"))
    return worst


WGRAD_FAULTS = ("lazy_b_raw", "db_one_split", "chan_mul_of_sample0", "db_of_rounded_b")


def wgrad_emulate(c, dt, inp, fault=None):
    """fp32 torch: the operands as the kernel rounds them, dW and db summed in fp32 and added onto the priors.  Returns (dw, db)."""
    dtype = DTYPES[dt]
    A = source_operand(inp["A"], dtype, chan_mul_of_sample0=(fault == "chan_mul_of_sample0"))[0].float()
    B = source_operand(inp["B"], dtype, raw=(fault == "lazy_b_raw"), chan_mul_of_sample0=(fault == "chan_mul_of_sample0"))[0].float()[:, :inp["knv"]]
    r = kr.wgrad_ref(A, B, ksize=c["ks"], stride=c["ks"])
    dw = inp["prior_dw"] + kr.to_layout(r["dw"], inp["strides"], tuple(inp["prior_dw"].shape))
    db = None
    if c["db"]:
        # the bias gradient sums a lazy B's fp32 value before it is rounded to the operand type (the fault: after)
        lz = {} if fault == "lazy_b_raw" else dict(inp["B"]["lazy"])
        if fault == "chan_mul_of_sample0" and "chan_mul" in lz:
            lz["chan_mul"] = lz["chan_mul"][:1].expand_as(lz["chan_mul"])
        Bv = B if fault == "db_of_rounded_b" else kr.lazy_f32(inp["B"]["x"], **lz)[0].float()[:, :inp["knv"]]
        tot = Bv.sum([0] + list(range(2, Bv.dim())))
        B = Bv
        if fault == "db_one_split":                        # the reduction reads the bias-gradient row of the first of two splits only
            tot = B[:1].sum([0] + list(range(2, B.dim()))) if c["N"] > 1 else B[..., :B.shape[-1] // 2].sum([0] + list(range(2, B.dim())))
        db = inp["prior_db"] + tot
    return dw, db
