"""The small ragged cases of the 3x3(x3) stride-1 conv and weight-gradient families -- conv_fwd_kernel, conv_wp_kernel, conv_kpar(2d)_kernel, wgrad_kernel,
wgrad_wp_kernel -- as ONE host-only table (a helper module, not a conftest), the k3 half of tests/small_conv_cases.py, whose sources, output slot, canaries
and resident-weights arithmetic it reuses.  tests/test_k3_conv_cases_cpu.py checks with the planner probe (tests/plan_probe.py) that every (case, dtype)
reaches the plan it names under its LIVE knobs, builds each case's kernel instance name from the restated dispatch rules (conv_dispatch.inc,
conv_wp_bf16.hip, conv_kpar_bf16.hip, wgrad_dispatch.inc) and proves that the table reaches every k3 instance name of
tests/golden/launch_plan_parent.csv; tests/test_k3_conv_families_gpu.py runs every (case, dtype) once on the GPU.  Both go through the same inputs, the
same fp64 references (tests/kernel_ref.py) and the same checks below.

Base grids, ragged against every pixel tile: 2D N = 2, 19 x 37 (4 x 16: 5 x 3 tiles, 8 x 16: 3 x 3, 16 x 16: 2 x 3); 3D N = 2, 5 x 7 x 19 (4 x 4 x 16
bricks: 2 x 2 x 2, 1 x 4 x 16 slabs: 5 x 2 x 2).  A row with another grid says why."""
import itertools
import math

import torch
import torch.nn.functional as F

from tests import kernel_ref as kr
from tests import small_conv_cases as sc

DTYPES, DTYPE_ID, SLOT_COFF, SLOT_EXTRA, GUARD = sc.DTYPES, sc.DTYPE_ID, sc.SLOT_COFF, sc.SLOT_EXTRA, sc.GUARD
CF, CD = kr.PACK_CONV_FWD, kr.PACK_CONV_DGRAD
G2, G3 = (19, 37), (5, 7, 19)
BOTH, BF = ("f32", "bf16"), ("bf16",)


def gen(nt=0, mr=0, **more):
    """the live knobs of a generic-route case: the blocking override from 16 input channels up, no wave-private and no K-parallel route"""
    k = dict(CHAP_CONV_MINC=16, CHAP_CONV_WP=0, CHAP_CONV_KPAR=0)
    if nt:
        k["CHAP_CONV_NT"] = nt
    if mr:
        k["CHAP_CONV_MR"] = mr
    k.update(more)
    return k


# ---- forward table ------------------------------------------------------------------------------------------------------------------------------------------
# grid: the spatial grid ((H, W); (D, H, W) with dims = 3; (D, H, W) with dims = 2: N * D slices); cin: channels per source; arr: one / cat / add;
# src: source kinds per source (small_conv_cases.make_source); plan = (KC, NT, MR) of the planner; route generic / wp / kpar; cpar: K chunks side by side
# (kpar); wlds: resident weights per dtype name (None: not pinned); knobs: LIVE knobs; trip: a persistent block owns >= 2 tiles (asserted on the GPU from
# the statistics header); out: slot (channel slot of a wider NaN buffer) / out2 (two such buffers, split at cout / 2) / planar (fp32 [N, C, H, W]).
def _fwd(name, dims, N, grid, cin, cout, plan, src, knobs, *, route="generic", arr=None, kind=CF, bias=True, stats=False, out="slot", dts=BOTH, cpar=0,
         wlds=None, trip=False, why=""):
    cin = cin if isinstance(cin, tuple) else (cin,)
    src = src if isinstance(src, tuple) else (src,)
    assert len(cin) == len(src) and (len(cin) == 1 or arr in ("cat", "add")) and (not trip or stats)
    return dict(name=name, op="k3", dims=dims, N=N, grid=tuple(grid), cin=cin, cout=cout, plan=plan, src=src, knobs=dict(knobs), route=route,
                arr=arr or "one", kind=kind, bias=bias, stats=stats, out=out, dts=dts, cpar=cpar, wlds=wlds, trip=trip, why=why)


WP, KP = dict(), dict(CHAP_CONV_KPAR=1)                      # wave-private: the default knobs; K-parallel: whenever eligible
FWD_CASES = [
    # ---- 2D generic, 16-channel chunks: every (NT, MR)
    _fwd("g2_16_16_n1m1", 2, 2, G2, 16, 16, (16, 1, 1), "ark", gen(1, 1), stats=True),
    _fwd("g2_16_16_n1m2", 2, 2, G2, 16, 16, (16, 1, 2), "ar", gen(1, 2), bias=False, stats=True),
    _fwd("g2_16_4_planar", 2, 2, G2, 16, 4, (16, 1, 4), "ar", gen(1, 4), out="planar", wlds=sc.RES),             # the golden file's `16->4 planar`
    _fwd("g2_16_32_n2m1", 2, 2, G2, 16, 32, (16, 2, 1), "sl", gen(2, 1), kind=CD),
    _fwd("g2_16_48_n2m2", 2, 2, G2, 16, 48, (16, 2, 2), "arm", gen(2, 2), stats=True),                            # 3 channel tiles at NT 2: a tile tail
    _fwd("g2_16_32_n2m4", 2, 2, G2, 16, 32, (16, 2, 4), "p", gen(2, 4), stats=True, wlds=sc.RES),
    _fwd("g2_48_64_n4m1", 2, 2, G2, 48, 64, (16, 4, 1), "p", gen(4, 1), bias=False),                              # three 16-channel chunks
    _fwd("g2_16_100_n4m2", 2, 2, G2, 16, 100, (16, 4, 2), "ar", gen(4, 2), stats=True),                           # 7 channel tiles at NT 4, Cout % 16 = 4
    _fwd("g2_16_64_n4m4", 2, 2, G2, 16, 64, (16, 4, 4), "ark", gen(4, 4)),
    _fwd("g2_16_20_n2m2", 2, 2, G2, 16, 20, (16, 2, 2), "sl", gen(2, 2), stats=True),                             # Cout a multiple of 4, not of 16
    # ---- 2D generic, 32-channel chunks
    _fwd("g2_128_16_n1m1", 2, 2, G2, 128, 16, (32, 1, 1), "p", gen(1, 1), wlds={"f32": False, "bf16": True}),
    _fwd("g2_32_16_n1m2", 2, 2, G2, 32, 16, (32, 1, 2), "sl", gen(1, 2), stats=True, wlds=sc.RES),
    _fwd("g2_cat_16_16_16_n1m2", 2, 2, G2, (16, 16), 16, (32, 1, 2), ("ar", "p"), gen(1, 2), arr="cat", stats=True, wlds=sc.RES),   # LANESEL: 16 % 32
    _fwd("g2_32_16_n1m4", 2, 2, G2, 32, 16, (32, 1, 4), "p", gen(1, 4)),
    _fwd("g2_128_32_n2m1", 2, 2, G2, 128, 32, (32, 2, 1), "ark", gen(2, 1), stats=True, wlds=sc.NONRES),
    _fwd("g2_32_32_n2m2", 2, 2, G2, 32, 32, (32, 2, 2), "arm", gen(2, 2), stats=True, wlds=sc.RES),
    _fwd("g2_64_32_n2m2", 2, 2, G2, 64, 32, (32, 2, 2), "ar", gen(2, 2), bias=False, wlds={"f32": False, "bf16": True}),
    _fwd("g2_64_64_n2m2", 2, 2, G2, 64, 64, (32, 2, 2), "ar", gen(2, 2), stats=True, dts=BF, wlds={"bf16": True}),
    _fwd("g2_128_64_n2m2", 2, 2, G2, 128, 64, (32, 2, 2), "p", gen(2, 2), dts=BF, wlds={"bf16": False}),          # staged bf16: 128 K channels at NT 2
    _fwd("g2_cat_32_32_32_n2m2", 2, 2, G2, (32, 32), 32, (32, 2, 2), ("ar", "p"), gen(2, 2), arr="cat", stats=True, wlds={"f32": False, "bf16": True}),
    _fwd("g2_cat_64_64_64_n2m2", 2, 2, G2, (64, 64), 64, (32, 2, 2), ("ar", "sl"), gen(2, 2), arr="cat", stats=True, dts=BF, wlds={"bf16": False}),
    _fwd("g2_cat_48_16_32_n2m2", 2, 2, G2, (48, 16), 32, (32, 2, 2), ("p", "ar"), gen(2, 2), arr="cat"),         # LANESEL: chunk 1 straddles the sources
    _fwd("g2_64_32_n2m4", 2, 2, G2, 64, 32, (32, 2, 4), "p", gen(2, 4)),
    _fwd("g2_64_64_n4m1", 2, 2, G2, 64, 64, (32, 4, 1), "sl", gen(4, 1), stats=True, wlds=sc.NONRES),
    _fwd("g2_cat_32_32_64_n4m1", 2, 2, G2, (32, 32), 64, (32, 4, 1), ("ark", "p"), gen(4, 1), arr="cat", wlds=sc.NONRES),
    _fwd("g2_64_64_n4m2", 2, 2, G2, 64, 64, (32, 4, 2), "arm", gen(4, 2), kind=CD, wlds=sc.NONRES),
    _fwd("g2_cat_32_32_64_n4m2", 2, 2, G2, (32, 32), 64, (32, 4, 2), ("ar", "arm"), gen(4, 2), arr="cat", stats=True, wlds=sc.NONRES),
    _fwd("g2_64_100_n4m4", 2, 2, G2, 64, 100, (32, 4, 4), "ar", gen(4, 4), stats=True),                           # KC 32 with MR 4, 7 tiles at NT 4
    # ---- 2D add-combine: launch_geom<3, 1, false, 2, true> whatever MR the plan holds; mask / multipliers on the first source
    _fwd("g2_add_16_16", 2, 2, G2, (16, 16), 16, (16, 1, 1), ("ark", "ar"), gen(1, 1), arr="add", stats=True),
    _fwd("g2_add_32_32_n2m4", 2, 2, G2, (32, 32), 32, (32, 2, 4), ("arm", "p"), gen(2, 4), arr="add", bias=False),
    _fwd("g2_add_64_48", 2, 2, G2, (64, 64), 48, (32, 2, 2), ("ar", "ar"), gen(2, 2), arr="add", stats=True),
    # ---- 2D: two dense outputs, split at a 16-channel boundary inside one block's tiles; dims = 2 with D > 1 (N * D slices)
    _fwd("g2_out2_32_64_n4m2", 2, 2, G2, 32, 64, (32, 4, 2), "p", gen(4, 2), out="out2", bias=False),
    _fwd("g2_out2_16_32_n2m1", 2, 2, G2, 16, 32, (16, 2, 1), "ar", gen(2, 1), out="out2", stats=True),
    _fwd("g2_slices_16_16", 2, 2, (2,) + G2, 16, 16, (16, 1, 2), "ark", gen(1, 2), stats=True),
    # ---- 2D generic, a second trip per pixel-tile shape: 16 -> 32 at NT 1 (two channel-tile rows: at most CUs x 2 / 2 blocks), 544 pixel tiles
    _fwd("g2_trip_m1", 2, 2, (67, 253), 16, 32, (16, 1, 1), "ar", gen(1, 1), stats=True, trip=True, why="17 x 16 tiles of 4 x 16 per image"),
    _fwd("g2_trip_m2", 2, 2, (133, 253), 16, 32, (16, 1, 2), "p", gen(1, 2), stats=True, trip=True, why="17 x 16 tiles of 8 x 16 per image"),
    _fwd("g2_trip_m4", 2, 2, (267, 253), 16, 32, (16, 1, 4), "p", gen(1, 4), stats=True, trip=True, why="17 x 16 tiles of 16 x 16 per image"),
    # ---- wave-private 2D (bf16, all input channels in one chunk): the five golden instances, LANESEL at NT 2, 64 outputs (two block rows), out2;
    # every block owns eight tiles (two per wave), the base grid has 30
    _fwd("wp_16_16", 2, 2, G2, 16, 16, (16, 1, 1), "ark", WP, route="wp", stats=True, dts=BF, trip=True),
    _fwd("wp_16_32", 2, 2, G2, 16, 32, (16, 2, 1), "p", WP, route="wp", dts=BF, bias=False),
    _fwd("wp_32_16", 2, 2, G2, 32, 16, (32, 1, 1), "sl", WP, route="wp", dts=BF, kind=CD),
    _fwd("wp_cat_16_16_16", 2, 2, G2, (16, 16), 16, (32, 1, 1), ("ar", "p"), WP, route="wp", arr="cat", stats=True, dts=BF, trip=True),
    _fwd("wp_32_32", 2, 2, G2, 32, 32, (32, 2, 1), "ar", WP, route="wp", stats=True, dts=BF, trip=True),
    _fwd("wp_cat_16_16_32", 2, 2, G2, (16, 16), 32, (32, 2, 1), ("ark", "ar"), WP, route="wp", arr="cat", dts=BF),
    _fwd("wp_32_64", 2, 2, G2, 32, 64, (32, 2, 1), "arm", WP, route="wp", stats=True, dts=BF, trip=True),
    _fwd("wp_out2_16_32", 2, 2, G2, 16, 32, (16, 2, 1), "ar", WP, route="wp", out="out2", stats=True, dts=BF, trip=True),
    # ---- K-parallel (bf16, >= 64 K channels): each case also runs with CHAP_CONV_KPAR = 0
    _fwd("kp3_64_64", 3, 2, G3, 64, 64, (16, 2, 1), "ar", KP, route="kpar", cpar=4, stats=True, dts=BF),          # the golden instance
    _fwd("kp3_cat_32_32_48", 3, 2, G3, (32, 32), 48, (16, 2, 1), ("arm", "p"), KP, route="kpar", cpar=4, arr="cat", stats=True, dts=BF),   # Cout % 32 = 16
    _fwd("kp3_96_32", 3, 2, G3, 96, 32, (16, 2, 1), "sl", KP, route="kpar", cpar=2, dts=BF, bias=False),         # 6 chunks: 2 side by side, three rounds
    _fwd("kp3_128_20", 3, 2, G3, 128, 20, (16, 2, 1), "p", KP, route="kpar", cpar=4, stats=True, dts=BF),        # 8 chunks: two rounds; Cout % 16 = 4
    _fwd("kp2_64_32", 2, 2, G2, 64, 32, (32, 2, 2), "ark", KP, route="kpar", cpar=2, stats=True, dts=BF),
    _fwd("kp2_128_48", 2, 2, G2, 128, 48, (32, 2, 2), "ar", KP, route="kpar", cpar=4, dts=BF),
    _fwd("kp2_cat_128_128_32", 2, 2, G2, (128, 128), 32, (32, 2, 2), ("ar", "p"), KP, route="kpar", cpar=4, arr="cat", stats=True, dts=BF),   # two rounds
    _fwd("kp2_slices_64_16", 2, 2, (2,) + G2, 64, 16, (32, 2, 2), "p", KP, route="kpar", cpar=2, stats=True, dts=BF),
    _fwd("kp2_trip", 2, 2, (261, 507), 64, 16, (32, 2, 2), "p", KP, route="kpar", cpar=2, stats=True, dts=BF, trip=True,
         why="33 x 32 tiles of 8 x 16 per image: 2112 tiles for at most 1024 blocks (one statistics slot each)"),
    _fwd("kp3_trip", 3, 2, (5, 55, 237), 64, 16, (16, 2, 1), "p", KP, route="kpar", cpar=4, stats=True, dts=BF, trip=True,
         why="5 x 14 x 15 tiles of 4 x 16 per volume: 2100 tiles for at most 1024 blocks"),
    # ---- 3D slabs (1 x 4 x 16; fp32 and bf16), NT 1 / 2 / 4, with and without add
    _fwd("g3_16_16_n1", 3, 2, G3, 16, 16, (16, 1, 1), "arm", gen(1, 1), stats=True),
    _fwd("g3_32_48_n2", 3, 2, G3, 32, 48, (16, 2, 1), "ar", gen(2, 1), stats=True),                               # 3 channel tiles at NT 2
    _fwd("g3_64_64_n4", 3, 2, G3, 64, 64, (16, 4, 1), "sl", gen(4, 1), bias=False, wlds={"f32": False, "bf16": False}),
    _fwd("g3_cat_16_32_32_n2", 3, 2, G3, (16, 32), 32, (16, 2, 1), ("p", "arm"), gen(2, 1), arr="cat", stats=True),
    _fwd("g3_add_16_16_n1", 3, 2, G3, (16, 16), 16, (16, 1, 1), ("arm", "ar"), gen(1, 1), arr="add", stats=True),
    _fwd("g3_add_64_64_n4", 3, 2, G3, (64, 64), 64, (16, 4, 1), ("ar", "ar"), gen(4, 1), arr="add", stats=True, wlds={"f32": False, "bf16": False}),
    _fwd("g3_16_20_n2", 3, 2, G3, 16, 20, (16, 2, 1), "p", gen(2, 1), kind=CD),                                   # Cout % 16 = 4
    # ---- 3D bricks (4 x 4 x 16, bf16), NT 1 / 2, with and without add
    _fwd("b3_32_16_n1", 3, 2, G3, 32, 16, (16, 1, 4), "p", gen(1, 4), stats=True, dts=BF, wlds={"bf16": True}),
    _fwd("b3_add_16_16_n1", 3, 2, G3, (16, 16), 16, (16, 1, 4), ("ar", "ar"), gen(1, 4), arr="add", stats=True, dts=BF, wlds={"bf16": True}),
    _fwd("b3_32_32_n2", 3, 2, G3, 32, 32, (16, 2, 4), "arm", gen(2, 4), stats=True, dts=BF, wlds={"bf16": True}),
    _fwd("b3_64_64_n2", 3, 2, G3, 64, 64, (16, 2, 4), "ar", gen(2, 4), stats=True, dts=BF, wlds={"bf16": False}),
    _fwd("b3_add_32_32_n2", 3, 2, G3, (32, 32), 32, (16, 2, 4), ("arm", "ar"), gen(2, 4), arr="add", stats=True, dts=BF, wlds={"bf16": True}),
    _fwd("b3_add_64_64_n2", 3, 2, G3, (64, 64), 64, (16, 2, 4), ("ar", "sl"), gen(2, 4), arr="add", bias=False, dts=BF, wlds={"bf16": False}),
    _fwd("b3_cat_16_32_48_n2", 3, 2, G3, (16, 32), 48, (16, 2, 4), ("sl", "ar"), gen(2, 4), arr="cat", stats=True, dts=BF),
    # ---- 3D, a second trip: 16 -> 32 at NT 1 (two channel-tile rows: at most CUs x 4 / 2 blocks)
    _fwd("g3_trip_slab", 3, 2, (5, 27, 237), 16, 32, (16, 1, 1), "p", gen(1, 1), stats=True, trip=True, why="5 x 7 x 15 slabs per volume: 1050"),
    _fwd("b3_trip_brick", 3, 2, (15, 27, 301), 16, 32, (16, 1, 4), "p", gen(1, 4), stats=True, trip=True, dts=BF, why="4 x 7 x 19 bricks per volume: 1064"),
]
BIG = {c["name"] for c in FWD_CASES if math.prod(c["grid"]) * c["N"] > 20000}      # the second-trip cases: the GPU file's alone


# ---- weight-gradient table ------------------------------------------------------------------------------------------------------------------------------------
# fam: slab / brick / wp; plan = (KC, bn, mr); ca: channels per A source; arr one / cat / add; A: kinds per source; nsplit: what the planner must return
# under the knobs (None: the default targets, not pinned); kn_valid / kc_valid: live B / A channels (0 = all); deal: emulate split by split
def _wg(name, dims, N, grid, ca, cb, fam, plan, knobs, *, arr=None, A="p", db=False, kn_valid=0, kc_valid=0, nsplit=None, dts=BOTH, why=""):
    ca = ca if isinstance(ca, tuple) else (ca,)
    A = A if isinstance(A, tuple) else (A,)
    assert len(ca) == len(A) and (len(ca) == 1 or arr in ("cat", "add"))
    return dict(name=name, dims=dims, N=N, grid=tuple(grid), ca=ca, cb=cb, fam=fam, plan=plan, knobs=dict(knobs), arr=arr or "one", A=A, B="p", db=db,
                kn_valid=kn_valid, kc_valid=kc_valid, nsplit=nsplit, dts=dts, why=why)


def slab(blocks=0, **more):
    """the live knobs of a slab case: no wave-private 2D kernel, no 3D bricks; blocks: CHAP_WGRAD_BLOCKS, the split target of the layer"""
    k = dict(CHAP_WGRAD_WP=0, CHAP_WGRAD_BRICK=0)
    if blocks:
        k["CHAP_WGRAD_BLOCKS"] = blocks
    k.update(more)
    return k


def blk(blocks=0, **more):
    k = dict(more)
    if blocks:
        k["CHAP_WGRAD_BLOCKS"] = blocks
    return k


G2_9, G3S_9, G3B_9 = (19, 37), (3, 10, 13), (9, 10, 13)       # with N = 1: nine 8 x 16 tiles; nine 1 x 4 x 16 slabs; nine 4 x 4 x 16 bricks
WGRAD_CASES = [
    # ---- 2D slabs (8 x 16 tiles; fp32 by default, bf16 with CHAP_WGRAD_WP = 0): the four golden (KC, bn), sources, edges
    _wg("w2_16_16", 2, 2, G2, 16, 16, "slab", (16, 16, 0), slab(), A="ar", db=True, nsplit=18),
    _wg("w2_16_40", 2, 2, G2, 16, 40, "slab", (16, 32, 0), slab(), A="ark", db=True),                             # Cb % bn = 8
    _wg("w2_cat_16_16_16", 2, 2, G2, (16, 16), 16, "slab", (32, 16, 0), slab(), arr="cat", A=("ar", "p"), db=True),   # LANESEL
    _wg("w2_32_32", 2, 2, G2, 32, 32, "slab", (32, 32, 0), slab(), A="arm"),
    _wg("w2_cat_32_32_32", 2, 2, G2, (32, 32), 32, "slab", (32, 32, 0), slab(), arr="cat", A=("sl", "ar"), db=True),
    _wg("w2_cat_48_16_32", 2, 2, G2, (48, 16), 32, "slab", (32, 32, 0), slab(), arr="cat", A=("p", "ar")),       # LANESEL: chunk 1 straddles the sources
    _wg("w2_add_32_32", 2, 2, G2, (32, 32), 32, "slab", (32, 32, 0), slab(), arr="add", A=("ark", "ar"), db=True),
    _wg("w2_add_16_16", 2, 2, G2, (16, 16), 16, "slab", (16, 16, 0), slab(), arr="add", A=("arm", "p")),
    _wg("w2_head_16_4", 2, 2, G2, 16, 16, "slab", (16, 16, 0), slab(), A="ar", db=True, kn_valid=4),              # the 16 -> 4 head: a gradient padded to 16
    _wg("w2_kc_valid_8", 2, 2, G2, 16, 32, "slab", (16, 32, 0), slab(), A="sl", kc_valid=8),
    _wg("w2_slices_16_16", 2, 2, (2,) + G2, 16, 16, "slab", (16, 16, 0), dict(), A="ark", db=True),               # dims = 2, D = 2: slabs in either type
    # tile dealing: 18 tiles
    _wg("w2_split1", 2, 2, G2, 16, 16, "slab", (16, 16, 0), slab(1), A="ar", db=True, nsplit=1),
    _wg("w2_split5", 2, 2, G2, 16, 16, "slab", (16, 16, 0), slab(5), A="p", db=True, nsplit=5),                   # 4 / 4 / 4 / 4 / 2 tiles
    _wg("w2_split12", 2, 2, G2, 32, 32, "slab", (32, 32, 0), slab(12), A="ar", nsplit=12),
    _wg("w2_split9_of_9", 2, 1, G2_9, 16, 16, "slab", (16, 16, 0), slab(9), A="ar", db=True, nsplit=9, why="N = 1: 9 tiles, three blocks with none"),
    _wg("w2_reduce8", 2, 2, (60, 67), 16, 16, "slab", (16, 16, 0), slab(), A="p", db=True, nsplit=80, why="80 tiles: >= 64 splits take wgrad_reduce_kernel<8>"),
    # ---- 2D wave-private (bf16): the two golden instances and <16, 1, 16>
    _wg("wp2_16_16", 2, 2, G2, 16, 16, "wp", (16, 16, 2), dict(), A="ar", db=True, dts=BF),
    _wg("wp2_32_32", 2, 2, G2, 32, 32, "wp", (16, 32, 1), dict(), A="ark", db=True, dts=BF),
    _wg("wp2_16_16_mr1", 2, 2, G2, 16, 16, "wp", (16, 16, 1), dict(CHAP_WGRAD_WP_MR=1), A="arm", db=True, dts=BF),
    _wg("wp2_cat_16_16_16", 2, 2, G2, (16, 16), 16, "wp", (16, 16, 2), dict(), arr="cat", A=("ar", "p"), dts=BF),
    _wg("wp2_cat_32_32_40", 2, 2, G2, (32, 32), 40, "wp", (16, 32, 1), dict(), arr="cat", A=("sl", "ar"), db=True, dts=BF),
    _wg("wp2_head_16_4", 2, 2, G2, 16, 16, "wp", (16, 16, 2), dict(), A="ar", db=True, kn_valid=4, dts=BF),
    _wg("wp2_split1", 2, 2, G2, 16, 16, "wp", (16, 16, 2), blk(1), A="ar", db=True, nsplit=1, dts=BF),
    _wg("wp2_split5", 2, 2, G2, 16, 16, "wp", (16, 16, 2), blk(5), A="p", nsplit=5, dts=BF),
    _wg("wp2_split12", 2, 2, G2, 16, 32, "wp", (16, 32, 1), blk(12), A="ar", db=True, nsplit=12, dts=BF),
    _wg("wp2_split9_of_9", 2, 1, G2_9, 16, 16, "wp", (16, 16, 2), blk(9), A="ar", db=True, nsplit=9, dts=BF, why="N = 1: 9 tiles"),
    # ---- 3D slabs (1 x 4 x 16; fp32 by default, bf16 with CHAP_WGRAD_BRICK = 0)
    _wg("w3_16_16", 3, 2, G3, 16, 16, "slab", (16, 16, 0), slab(), A="arm", db=True, nsplit=40),
    _wg("w3_32_32", 3, 2, G3, 32, 32, "slab", (32, 32, 0), slab(), A="ar", db=True),                              # the golden KC 32 slab
    _wg("w3_cat_16_32_24", 3, 2, G3, (16, 32), 24, "slab", (16, 32, 0), slab(), arr="cat", A=("p", "arm")),      # Cb % bn = 24
    _wg("w3_add_32_32", 3, 2, G3, (32, 32), 32, "slab", (32, 32, 0), slab(), arr="add", A=("arm", "ar"), db=True),
    _wg("w3_split1", 3, 2, G3, 16, 16, "slab", (16, 16, 0), slab(1), A="p", db=True, nsplit=1),
    _wg("w3_split5", 3, 2, G3, 16, 16, "slab", (16, 16, 0), slab(5), A="ar", nsplit=5),                           # 8 tiles each
    _wg("w3_split12", 3, 2, G3, 16, 16, "slab", (16, 16, 0), slab(12), A="sl", db=True, nsplit=12),
    _wg("w3_split9_of_9", 3, 1, G3S_9, 16, 16, "slab", (16, 16, 0), slab(9), A="ar", db=True, nsplit=9, why="N = 1, 3 x 10 x 13: 9 slabs"),
    # ---- 3D bricks (bf16; the base grid has 16)
    _wg("wb_32_16", 3, 2, G3, 32, 16, "brick", (16, 16, 0), dict(), A="p", db=True, dts=BF),
    _wg("wb_32_32", 3, 2, G3, 32, 32, "brick", (16, 32, 0), dict(), A="ar", db=True, dts=BF),
    _wg("wb_add_16_16", 3, 2, G3, (16, 16), 16, "brick", (16, 16, 0), dict(), arr="add", A=("ar", "ar"), db=True, dts=BF),
    _wg("wb_add_32_32", 3, 2, G3, (32, 32), 32, "brick", (16, 32, 0), dict(), arr="add", A=("arm", "ar"), dts=BF),
    _wg("wb_cat_16_16_40", 3, 2, G3, (16, 16), 40, "brick", (16, 32, 0), dict(), arr="cat", A=("sl", "arm"), db=True, dts=BF),
    _wg("wb_split1", 3, 2, G3, 16, 16, "brick", (16, 16, 0), blk(1), A="ar", db=True, nsplit=1, dts=BF),          # 16 bricks in one block
    _wg("wb_split5", 3, 2, G3, 16, 16, "brick", (16, 16, 0), blk(5), A="p", db=True, nsplit=5, dts=BF),           # 4 / 4 / 4 / 4 / 0 bricks
    _wg("wb_split12", 3, 2, G3, 16, 16, "brick", (16, 16, 0), blk(12), A="arm", nsplit=12, dts=BF),
    _wg("wb_split9_of_9", 3, 1, G3B_9, 16, 16, "brick", (16, 16, 0), blk(9, CHAP_WGRAD_BRICK=1), A="ar", db=True, nsplit=9, dts=BF,
        why="N = 1, 9 x 10 x 13: 9 bricks, below the default threshold of 16"),
]

BY_NAME = {c["name"]: c for c in FWD_CASES + WGRAD_CASES}
assert len(BY_NAME) == len(FWD_CASES) + len(WGRAD_CASES)
FWD_IDS = [(c["name"], dt) for c in FWD_CASES for dt in c["dts"]]
WGRAD_IDS = [(c["name"], dt) for c in WGRAD_CASES for dt in c["dts"]]


# ---- geometry helpers -----------------------------------------------------------------------------------------------------------------------------------------
def spatial(c):
    """(D, H, W) of the launch's grid"""
    g = c["grid"]
    return g if len(g) == 3 else (1,) + g


def slices(c):
    """dims = 2 with D > 1: the launch walks N * D images"""
    return c["dims"] == 2 and len(c["grid"]) == 3


def images(c):
    """(sample count, spatial shape) of the tensors the references work on: the slices of a dims = 2, D > 1 launch are samples"""
    return (c["N"] * c["grid"][0], c["grid"][1:]) if slices(c) else (c["N"], c["grid"])


def setenv_line(c):
    return "setenv " + " ".join("%s=%s" % kv for kv in c["knobs"].items()) if c["knobs"] else None


def _common_request(c, dt, chans):
    D, H, W = spatial(c)
    f = dict(dims=c["dims"], k=3, s=1, N=c["N"], D=D, H=H, W=W, dtype=DTYPE_ID[dt], combine=int(c["arr"] == "add"), C0=chans[0], C1=chans[1] if len(chans) > 1 else 0)
    kinds = c["src"] if "src" in c else c["A"]
    for i, s in enumerate(kinds):
        f["keep%d" % i], f["cm%d" % i] = int(s == "ark"), int(s == "arm")
    return f


def fwd_request(c, dt):
    f = _common_request(c, dt, c["cin"])
    f.update(Cout=c["cout"], nsrc=len(c["cin"]), planar=int(c["out"] == "planar"), f32out=int(c["out"] == "planar"), stats=int(c["stats"]))
    if c["src"][0] == "sl":
        f["ld0"] = c["cin"][0] + sc.SRC_EXTRA
    return "conv " + " ".join("%s=%s" % kv for kv in f.items())


def wgrad_request(c, dt):
    f = _common_request(c, dt, c["ca"])
    f.update(Cb=c["cb"], na=len(c["ca"]))
    return "wgrad " + " ".join("%s=%s" % kv for kv in f.items())


def k_channels(c):
    ch = c["cin"] if "cin" in c else c["ca"]
    return ch[0] if c["arr"] == "add" else sum(ch)


def launched_tile(c, dt):
    """(MR template argument, ZW, (TD, TH, TW)) of the generic instance CONV_FN (conv_dispatch.inc) launches for plan MR: 2D add-combine is built on the
    8 x 16 tile only; 3D: 4 x 4 x 16 bricks for bf16 with MR 4, else 1 x 4 x 16 slabs"""
    MR = c["plan"][2]
    if c["dims"] == 2:
        MR = 2 if c["arr"] == "add" else MR
        return MR, False, (1, 4 * MR, 16)
    if dt == "bf16" and MR == 4:
        return 4, True, (4, 4, 16)
    return 1, False, (1, 4, 16)


def pixel_tiles(c, dt):
    """pixel tiles of the launch, per route"""
    D, H, W = spatial(c)
    if c["route"] == "wp":
        td, th = 1, 4
    elif c["route"] == "kpar":
        td, th = 1, (4 if c["dims"] == 3 else 8)
    else:
        td, th = launched_tile(c, dt)[2][:2]
    return c["N"] * -(-D // td) * -(-H // th) * -(-W // 16)


def case_lds(c, dt):
    """(WLDS, LDS bytes) of a generic case: small_conv_cases.conv_lds, the restated launch_one, with the launched tile"""
    KC, NT, _ = c["plan"]
    MR, ZW, _ = launched_tile(c, dt)
    return sc.conv_lds(2 if dt == "bf16" else 4, 3, 1, c["dims"] == 3, KC, NT, MR, ZW, k_channels(c) // KC)


def _b(v):
    return "true" if v else "false"


def fwd_instance(c, dt):
    """the kernel instance a forward case launches, in the spelling of tests/golden/launch_plan_parent.csv"""
    KC, NT, _ = c["plan"]
    two, add = len(c["cin"]) == 2, c["arr"] == "add"
    if c["route"] == "wp":                                   # conv_wp_bf16.hip: <KC, NT, LANESEL>
        return "conv_wp_kernel<%d,%d,%s>" % (KC, NT, _b(two))
    if c["route"] == "kpar":                                 # conv_kpar_bf16.hip: 2D with 32-channel chunks takes conv_kpar2d_kernel<NT, CPAR, ONE, KEEPM, SINGLE>
        if c["dims"] == 2 and KC == 32:
            return "conv_kpar2d_kernel<2,%d,%s,%s,%s>" % (c["cpar"], _b(not two), _b("ark" in c["src"]), _b(k_channels(c) // KC == c["cpar"]))
        return "conv_kpar_kernel<bf16,%s,%d,2,%d,%s>" % (_b(c["dims"] == 3), KC, c["cpar"], _b(not two))
    MR, ZW, _ = launched_tile(c, dt)                         # conv_dispatch.inc: <T, KS, ST, D3, KC, NT, MR, ADD2, WLDS, ZW, ONE>
    return "conv_fwd_kernel<%s,3,1,%s,%d,%d,%d,%s,%s,%s,%s>" % (dt, _b(c["dims"] == 3), KC, NT, MR, _b(add), _b(case_lds(c, dt)[0]), _b(ZW), _b(not two))


def wgrad_instance(c, dt):
    KC, bn, mr = c["plan"]
    if c["fam"] == "wp":                                     # wgrad_dispatch.inc: <KC, MR, BN>
        return "wgrad_wp_kernel<%d,%d,%d>" % (KC, mr, bn)
    MR = 4 if c["fam"] == "brick" else (1 if c["dims"] == 3 else 2)      # <T, KS, ST, D3, KC, MR, ADD2, BN, PD, ZW>
    return "wgrad_kernel<%s,3,1,%s,%d,%d,%s,%d,1,%s>" % (dt, _b(c["dims"] == 3), KC, MR, _b(c["arr"] == "add"), bn, _b(c["fam"] == "brick"))


def wgrad_tile(c):
    """wgrad_plan.h: 8 x 16 tiles, 1 x 4 x 16 for the 3D geometries, 4 x 4 x 16 for the bricks: (TD, TH, TW)"""
    if c["fam"] == "brick":
        return 4, 4, 16
    return (1, 4, 16) if c["dims"] == 3 else (1, 8, 16)


def wgrad_tiles(c):
    D, H, W = spatial(c)
    td, th, tw = wgrad_tile(c)
    return c["N"] * -(-D // td) * -(-H // th) * -(-W // tw)


def deal_tiles(ntiles, nsplit):
    """wgrad_kernel.h: up to 8 tile groups own a contiguous share of the tiles each and deal it round-robin to their splits (split s belongs to group
    s % NG).  Returns the tile list of every split."""
    NG = min(nsplit, 8)
    per = -(-ntiles // NG)
    out = []
    for s in range(nsplit):
        x, sj = s % NG, s // NG
        bpx = (nsplit + NG - 1 - x) // NG
        lo, hi = per * x, min(per * x + per, ntiles)
        out.append(list(range(lo + sj, hi, bpx)) if bpx > 0 else [])
    return out


# ---- inputs and references ----------------------------------------------------------------------------------------------------------------------------------------
def _gen(c, dt, lane=0):
    return torch.Generator().manual_seed(sum(map(ord, c["name"])) * 2 + DTYPE_ID[dt] + sc.LANE_SEED * lane)


def _sources(c, dt, kinds, chans, g):
    Ne, sp = images(c)
    return [sc.make_source(kd, Ne, ci, sp, DTYPES[dt], g) for kd, ci in zip(kinds, chans)]


def combined_operand(c, dt, srcs, mask_on_second=False, straddle_from_first=False):
    """(MFMA operand, flip) of the launch's K channels: concatenated sources, or the fp32 sum of an add-combined pair rounded once (kernel_ref.add_f32).
    The two switches are planted faults of the emulations."""
    dtype = DTYPES[dt]
    if c["arr"] == "add":
        lz = [dict(s["lazy"]) for s in srcs]
        if mask_on_second:
            for k in ("keep", "keep_scale", "chan_mul"):
                if k in lz[0]:
                    lz[1][k] = lz[0][k]
        v, dv = kr.add_f32([kr.lazy_f32(s["x"], **z) for s, z in zip(srcs, lz)])
        return kr.mfma_operand(v, dv, dtype)
    ops_ = [sc.source_operand(s, dtype) for s in srcs]
    a, flip = torch.cat([o[0] for o in ops_], 1), torch.cat([o[1] for o in ops_], 1)
    if straddle_from_first:                                  # the straddling chunk's second half: the first source's channels again
        C0, KC = srcs[0]["x"].shape[1], c["plan"][0]
        n = KC - C0 % KC
        assert C0 % KC and C0 >= n
        a = a.clone()
        a[:, C0:C0 + n] = a[:, C0 - n:C0]
    return a, flip


def weight_shape(c):
    K, M = k_channels(c), c["cout"]
    return ((M, K) if c["kind"] == CF else (K, M)) + (3,) * c["dims"]      # CONV_DGRAD: w [cout, cin, k..] of the layer whose input gradient this is


def pack_args(c):
    K, M, taps = k_channels(c), c["cout"], 3 ** c["dims"]
    return (K, M, taps) if c["kind"] == CF else (M, K, taps)


def fwd_inputs(c, dt, lane=0):
    g = _gen(c, dt, lane)
    K, M = k_channels(c), c["cout"]
    srcs = _sources(c, dt, c["src"], c["cin"], g)
    w = torch.randn(weight_shape(c), generator=g) / math.sqrt(K * 3 ** c["dims"])
    bias = torch.randn(M, generator=g) if c["bias"] else None
    shift = torch.randn(M, generator=g) * 0.3 if c["stats"] else None
    return dict(srcs=srcs, w=w, bias=bias, shift=shift)


def fwd_reference(c, dt, inp):
    a, flip = combined_operand(c, dt, inp["srcs"])
    r = kr.conv_ref(c["kind"], a, kr.weight_operand(inp["w"], DTYPES[dt]), inp["bias"], flip=flip)
    r["stats"] = kr.stats_ref(r, inp["shift"]) if c["stats"] else None
    return r


# ---- outputs: small_conv_cases' slot, once (slot), twice (out2) or the planar fp32 tensor, through its layout functions ------------------------------------------------
def out_parts(c):
    """[(layout dict for small_conv_cases.new_out / split_out, first channel, channels), ...]"""
    Ne, sp = images(c)
    base = dict(name=c["name"], op="head" if c["out"] == "planar" else "k3", dims=2 if c["dims"] == 2 else 3, N=Ne, grid=tuple(sp))
    if c["out"] == "out2":
        h = c["cout"] // 2
        return [(dict(base, cout=h), 0, h), (dict(base, cout=h), h, h)]
    return [(dict(base, cout=c["cout"]), 0, c["cout"])]


def store_type(c, dt):
    return torch.float32 if c["out"] == "planar" else DTYPES[dt]


def new_outs(c, dt, device="cpu"):
    """[(flat buffer, view), ...]: NaN everywhere"""
    return [sc.new_out(lc, DTYPES[dt], device) for lc, _, _ in out_parts(c)]


def fwd_check(c, dt, r, flats, stats):
    """per element under conv_bound, the statistics under stats_ref's bounds, the NaN canaries; for the kernel and for its emulation alike.
    flats: the output buffers on the CPU; stats: [2, Cout] totals or None.  Returns the worst error / bound of each check."""
    bnd = kr.conv_bound(r, store_type(c, dt))
    worst = []
    for (lc, lo, n), flat in zip(out_parts(c), flats):
        got, intact = sc.split_out(lc, flat)
        worst.append(kr.check(c["name"] + " out", got, r["y"][:, lo:lo + n], bnd[:, lo:lo + n]))
        assert intact, c["name"] + ": an element outside the output slot was written"
    if c["stats"]:
        (s1, b1), (s2, b2) = r["stats"]
        worst += [kr.check(c["name"] + " stats S", stats[0], s1, b1, dims="c"), kr.check(c["name"] + " stats Q", stats[1], s2, b2, dims="c")]
    return worst


# ---- the fp32 emulation of the forward kernels, with the planted faults -----------------------------------------------------------------------------------------------
FWD_FAULTS = ("edge_replicated", "taps_swapped", "depth_row_taps_swapped", "stats_ragged_edge", "last_row_dropped", "tile_tail_stored", "add_mask_on_second",
              "straddle_from_first")


def _w_conv(kind, w):
    """the weight of the plain correlation the launch computes: CONV_DGRAD flips and transposes the layer's taps (kernel_ref.conv_linear)"""
    return w if kind == CF else w.transpose(0, 1).flip(list(range(2, w.dim())))


def fwd_emulate(c, dt, inp, fault=None):
    """What the kernels do, in fp32 torch: the operands rounded to the MFMA operand type, zero padding, the products summed in fp32 (another order than the
    kernel's), bias, statistics of the unrounded value over the real pixels, one rounding into the slot.  Returns ([flat buffers], stats or None)."""
    dtype, dims = DTYPES[dt], c["dims"]
    a = combined_operand(c, dt, inp["srcs"], mask_on_second=(fault == "add_mask_on_second"), straddle_from_first=(fault == "straddle_from_first"))[0].float()
    w = _w_conv(c["kind"], kr.weight_operand(inp["w"], dtype).float())
    if fault == "taps_swapped":
        w = w.transpose(-1, -2)
    if fault == "depth_row_taps_swapped":
        assert dims == 3
        w = w.transpose(-3, -2)
    nd = a.dim() - 2
    M = c["cout"]
    bias = inp["bias"].float() if inp["bias"] is not None else torch.zeros(M)
    bsh = [1, M] + [1] * nd
    conv = lambda x: kr.conv_taps(F.pad(x, [1] * (2 * nd), mode="replicate" if fault == "edge_replicated" else "constant"), w, stride=1, pad=0) + bias.view(bsh)
    y = conv(a)
    stats = None
    if c["stats"]:
        ys = y
        if fault == "stats_ragged_edge":                     # the rows and columns of the last tiles beyond the grid, computed from zero inputs there
            th = pixel_tile(c, dt)[1]
            ext = [(-a.shape[-1]) % 16, (-a.shape[-2]) % th]
            assert ext[0] and ext[1]
            ys = conv(F.pad(a, [0, ext[0], 0, ext[1]]))
        d = ys.double() - inp["shift"].double().view(bsh)
        red = [0] + list(range(2, y.dim()))
        stats = torch.stack((d.sum(red), (d * d).sum(red)))
    outs = new_outs(c, dt)
    for (lc, lo, n), (flat, view) in zip(out_parts(c), outs):
        part = y[:, lo:lo + n]
        if c["out"] == "planar":
            view.copy_(part)
            if fault == "last_row_dropped":
                view[..., -1, :] = float("nan")
            continue
        ycl = (part if part.dim() == 5 else part.unsqueeze(2)).permute(0, 2, 3, 4, 1)
        view[..., SLOT_COFF:SLOT_COFF + n] = ycl.to(dtype)
        if fault == "tile_tail_stored":                      # the tiles of the last block row beyond Cout land behind the slot
            NT = c["plan"][1]
            tail = 16 * NT * -(-M // (16 * NT)) - M
            assert tail > 0
            view[..., SLOT_COFF + n:SLOT_COFF + n + min(tail, SLOT_EXTRA - SLOT_COFF)] = 0
        if fault == "last_row_dropped":
            view[:, :, -1, :, SLOT_COFF:SLOT_COFF + n] = float("nan")
    return [f for f, _ in outs], stats


def pixel_tile(c, dt):
    """(TD, TH, TW) of the route's pixel tile"""
    if c["route"] == "wp":
        return 1, 4, 16
    if c["route"] == "kpar":
        return 1, (4 if c["dims"] == 3 else 8), 16
    return launched_tile(c, dt)[2]


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------------------------------------------
def wgrad_inputs(c, dt, lane=0):
    g = _gen(c, dt, lane)
    Ne, sp = images(c)
    As = _sources(c, dt, c["A"], c["ca"], g)
    B = sc.make_source("p", Ne, c["cb"], sp, DTYPES[dt], g)
    Ca = k_channels(c)
    knv, kcv = c["kn_valid"] or c["cb"], c["kc_valid"] or Ca
    if knv != c["cb"]:
        B["x"][:, knv:] = 0                                # a head's gradient arrives zero-padded to 16 channels
    taps = 3 ** c["dims"]
    prior_dw = torch.randn(knv, kcv, taps, generator=g) * 0.5
    prior_db = torch.randn(knv, generator=g) * 0.5 if c["db"] else None
    return dict(As=As, B=B, prior_dw=prior_dw, prior_db=prior_db, strides=(1, taps, kcv * taps), knv=knv, kcv=kcv)


def wgrad_reference(c, dt, inp):
    A, fA = combined_operand(c, dt, inp["As"])
    B = sc.source_operand(inp["B"], DTYPES[dt])[0]
    knv, kcv = inp["knv"], inp["kcv"]
    r = kr.wgrad_ref(A, B[:, :knv], ksize=3, stride=1, flipA=fA)
    for k in ("dw", "sabs", "fterm"):
        r[k] = r[k][:, :kcv]
    return r


def wgrad_check(c, dt, rw, inp, dw, db):
    return sc.wgrad_check(c, dt, rw, inp, dw, db)


WGRAD_FAULTS = ("tile_twice", "split_left_out", "empty_split_nan", "edge_replicated", "taps_swapped", "add_mask_on_second", "straddle_from_first")


def _tile_masks(c):
    """one [Ne, 1, *sp] 0 / 1 mask per weight-gradient tile, in the kernel's tile order (sample, plane, row, column)"""
    Ne, sp = images(c)
    D, H, W = spatial(c)
    td, th, tw = wgrad_tile(c)
    masks = []
    for n, z, y, x in itertools.product(range(c["N"]), range(-(-D // td)), range(-(-H // th)), range(-(-W // tw))):
        m = torch.zeros((c["N"], D, H, W))
        m[n, z * td:(z + 1) * td, y * th:(y + 1) * th, x * tw:(x + 1) * tw] = 1
        masks.append(m.reshape((Ne, 1) + tuple(sp)))
    return masks


def wgrad_emulate(c, dt, inp, fault=None, nsplit=None):
    """fp32 torch: the operands as the kernel rounds them, zero padding; nsplit given: one slab per split from the tiles deal_tiles hands it, the slabs
    summed (what the reduction does); dW and db added onto the priors.  Returns (dw, db)."""
    A = combined_operand(c, dt, inp["As"], mask_on_second=(fault == "add_mask_on_second"), straddle_from_first=(fault == "straddle_from_first"))[0].float()
    B = sc.source_operand(inp["B"], DTYPES[dt])[0].float()[:, :inp["knv"]]
    nd = A.dim() - 2
    if fault == "edge_replicated":                           # wgrad_ref pads with zeros: hand it the replicated border as data
        A = F.pad(A, [1] * (2 * nd), mode="replicate")
        B = F.pad(B, [1] * (2 * nd))

    def total(Bm):
        r = kr.wgrad_ref(A, Bm, ksize=3, stride=1)
        dwt = r["dw"]
        if fault == "taps_swapped":
            k = [3] * nd
            dwt = dwt.reshape(k + list(dwt.shape[1:])).transpose(nd - 2, nd - 1).reshape(dwt.shape)
        return dwt[:, :inp["kcv"]], r["db"]

    if nsplit is None:
        assert fault not in ("tile_twice", "split_left_out", "empty_split_nan")
        dwt, dbt = total(B)
    else:
        assert fault != "edge_replicated"
        masks = _tile_masks(c)
        deal = deal_tiles(len(masks), nsplit)
        assert sorted(t for s in deal for t in s) == list(range(len(masks)))
        if fault == "tile_twice":
            deal[0] = deal[0] + [deal[-1][-1] if deal[-1] else deal[0][0]]
        if fault == "split_left_out":
            deal = deal[:-1] if deal[-1] else [s for s in deal if s][:-1]
        slabs = []
        for s in deal:
            if s:
                slabs.append(total(B * sum(masks[t] for t in s)))
            elif fault == "empty_split_nan":
                slabs.append((torch.full_like(slabs[0][0], float("nan")), slabs[0][1]))
        if fault == "empty_split_nan":
            assert any(not s for s in deal)
        dwt, dbt = sum(s[0] for s in slabs), sum(s[1] for s in slabs)
    dw = inp["prior_dw"] + kr.to_layout(dwt, inp["strides"], tuple(inp["prior_dw"].shape))
    db = inp["prior_db"] + dbt if c["db"] else None
    return dw, db
