"""Merged (grouped) launches of every kernel family behind the trampoline of chap_amd/csrc/launch.h, as ONE host-only table (a helper module, not a
conftest; it imports no device).  Between chap_group_begin() and chap_group_end() the library issues the j-th launch of every lane as one grid and block
(x, y, z) runs on argument block G.p[z] (the weight gradient: G.p[z / base_z]); a lane on another lane's arguments, a base_z slip or two lanes on one
workspace fail silently, so every launch site gets at least one case that runs as 2 and as 4 lanes of the same shapes and DIFFERENT data.

ENTRIES names every launch site of chap_amd/csrc -- (file, kernel expression of the chap_launch<> call or `ptr`, launch name argument) as scan_sites()
reads them from the sources -- with the cases that reach it.  Conv and weight-gradient cases are cases of tests/small_conv_cases.py (`sc`) and
tests/k3_conv_cases.py (`kc`) by name, with what the planner must answer for them (tests/plan_probe.py); every other family defines its own small
case here (OTHER), drawn by other_inputs(case, lane).  tests/test_group_cases_cpu.py proves the table against the sources and check_lanes() against
planted faults; tests/test_group_families_gpu.py runs it."""
import math
import os
import re

import torch

from tests import k3_conv_cases as kc
from tests import kernel_ref as kr
from tests import small_conv_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chap_amd", "csrc")
MAX_LANES = 4                                               # CHAP_MAX_LANES of the product build (lab builds with CHAP_TIMELINE merge 3: not tested)
LANES = (2, 4)
GUARD = 64                                                  # elements on either side of an output of the OTHER families
F32, BF = "f32", "bf16"
DT = sc.DTYPES


# ---- the launch sites, from the sources ------------------------------------------------------------------------------------------------------------------
def _split_top(s, opening="<(", closing=">)"):
    """split at the commas outside brackets and quotes"""
    out, depth, cur, quote = [], 0, "", False
    for ch in s:
        if ch == '"':
            quote = not quote
        if not quote:
            if ch in opening:
                depth += 1
            elif ch in closing:
                depth -= 1
            elif ch == "," and depth == 0:
                out.append(cur.strip())
                cur = ""
                continue
        cur += ch
    return out + [cur.strip()]


def _balanced(s, i, open_, close):
    """s[i] == open_: the index just behind its matching close"""
    depth = 0
    for j in range(i, len(s)):
        depth += s[j] == open_
        depth -= s[j] == close
        if depth == 0:
            return j + 1
    raise ValueError("unbalanced: " + s[i:i + 80])


def scan_sites(csrc=CSRC):
    """{(file, kernel, name)}: every chap_launch< / chap_launch_z< / chap_launch_ptr< CALL under csrc (launch.h itself defines them).  kernel: the BODY
    template argument as written (spaces dropped), `ptr` for chap_launch_ptr; name: the launch-name argument, a string's text or an identifier."""
    sites = set()
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".inc", ".h", ".cpp")) or fn == "launch.h":
            continue
        text = open(os.path.join(csrc, fn)).read()
        for m in re.finditer(r"\bchap_launch(_z|_ptr)?<", text):
            t_end = _balanced(text, m.end() - 1, "<", ">")
            targs = _split_top(text[m.end():t_end - 1])
            a0 = text.index("(", t_end)
            assert not text[t_end:a0].strip(), (fn, text[m.start():a0 + 20])
            args = _split_top(text[a0 + 1:_balanced(text, a0, "(", ")") - 1], "(", ")")      # (an argument may hold `->`)
            kernel = "ptr" if m.group(1) == "_ptr" else targs[1].replace(" ", "")
            sites.add((fn, kernel, args[-1].strip('"')))
    return sites


# ---- conv and weight-gradient cases: (module, case, dtype) and what the planner must say ---------------------------------------------------------------------
def conv_case(mod, name):
    return (kc if mod == "kc" else sc).BY_NAME[name]


def _cv(mod, name, dt, **want):
    return dict(id="%s:%s:%s" % (mod, name, dt), mod=mod, name=name, dt=dt, want=want)


# forward: route (generic / head / wp / kpar), geom (conv_plan.h: 1 = 2D k3, 2 = 3D k3, 3 = 1x1, 4 = 2D k2 s2, 5 = 3D k2 s2), kpar2d (32-channel chunks in 2D)
FWD = [
    _cv("kc", "g2_16_20_n2m2", BF, route="generic", geom=1),        # Cout % 16 = 4, statistics, a channel slice as the source
    _cv("kc", "g2_16_16_n1m1", F32, route="generic", geom=1),       # keep mask, statistics
    _cv("kc", "g3_16_16_n1", F32, route="generic", geom=2),         # channel multipliers, statistics
    _cv("kc", "b3_32_16_n1", BF, route="generic", geom=2),          # bricks
    _cv("sc", "k1_64_16", BF, route="generic", geom=3),
    _cv("sc", "k1_cat_16_32_32", F32, route="generic", geom=3),
    _cv("sc", "k2_16_16", BF, route="generic", geom=4),
    _cv("sc", "k2_3d_16_32", F32, route="generic", geom=5),
    _cv("sc", "d2s_3d_256_128", BF, route="generic", geom=3),       # 1x1 + depth-to-space
    _cv("sc", "head_c3_straddle", BF, route="head", geom=3),
    _cv("sc", "head_c3_straddle", F32, route="generic", geom=3),    # the same weights through the generic kernel's planar stores
    _cv("kc", "wp_16_16", BF, route="wp", geom=1),
    _cv("kc", "wp_cat_16_16_16", BF, route="wp", geom=1),
    _cv("kc", "kp3_64_64", BF, route="kpar", geom=2, kpar2d=False),
    _cv("kc", "kp2_64_32", BF, route="kpar", geom=1, kpar2d=True),
]
# weight gradient: fam (generic2d / generic3d / wp / brick / k1 / k2s2), base_z = ceil(Cb / bn) = the kernel's own grid.z, reduce = the reduce instance
WGRAD = [
    _cv("kc", "w2_16_16", F32, fam="generic2d", base_z=1, db=True, reduce=64),
    _cv("kc", "w2_16_40", BF, fam="generic2d", base_z=2, db=True, reduce=64),
    _cv("kc", "w2_head_16_4", BF, fam="generic2d", base_z=1, db=True, reduce=64, valid="kn"),
    _cv("kc", "w2_kc_valid_8", F32, fam="generic2d", base_z=1, db=False, reduce=64, valid="kc"),
    _cv("kc", "w2_reduce8", BF, fam="generic2d", base_z=1, db=True, reduce=8),
    _cv("kc", "w3_16_16", F32, fam="generic3d", base_z=1, db=True, reduce=64),
    _cv("kc", "wp2_cat_32_32_40", BF, fam="wp", base_z=2, db=True, reduce=64),
    _cv("kc", "wb_32_16", BF, fam="brick", base_z=1, db=True, reduce=64),
    _cv("sc", "wg_k1_48_40", F32, fam="k1", base_z=2, db=True, reduce=64),
    _cv("sc", "wg_k2_64_128", BF, fam="k2s2", base_z=4, db=False, reduce=64),
    _cv("sc", "wg_k2_3d_16_32", F32, fam="k2s2", base_z=1, db=True, reduce=64),
]
# the same shapes in the other dtype, for the lane-count rules of tests/test_group_families_gpu.py (another kernel instance: not merged); no site's only case
TWINS = [_cv("kc", "g2_16_20_n2m2", F32), _cv("kc", "w2_16_40", F32)]
CONV_BY_ID = {c["id"]: c for c in FWD + WGRAD + TWINS}
assert len(CONV_BY_ID) == len(FWD) + len(WGRAD) + len(TWINS)


def is_fwd(e):
    return "cout" in conv_case(e["mod"], e["name"])


def plan_request(e):
    """request lines of tests/plan_probe.py for a FWD / WGRAD row: the case's live knobs, then the launch"""
    c = conv_case(e["mod"], e["name"])
    mod = kc if e["mod"] == "kc" else sc
    req = [mod.fwd_request(c, e["dt"]) if is_fwd(e) else mod.wgrad_request(c, e["dt"])]
    if e["mod"] == "kc" and c["knobs"]:
        req.insert(0, kc.setenv_line(c))
    return req


def conv_inputs(e, lane=0):
    c, mod = conv_case(e["mod"], e["name"]), (kc if e["mod"] == "kc" else sc)
    return (mod.fwd_inputs if is_fwd(e) else mod.wgrad_inputs)(c, e["dt"], lane)


def conv_reference(e, inp):
    c, mod = conv_case(e["mod"], e["name"]), (kc if e["mod"] == "kc" else sc)
    return (mod.fwd_reference if is_fwd(e) else mod.wgrad_reference)(c, e["dt"], inp)


def fwd_parts(e):
    """[(layout dict for small_conv_cases.new_out / split_out, first channel, channels)] of a forward case's outputs"""
    c = conv_case(e["mod"], e["name"])
    return kc.out_parts(c) if e["mod"] == "kc" else [(c, 0, c["cout"])]


def fwd_views(e, r, flats, stats):
    """(got, ref, bound) dicts of a forward case: what small_conv_cases.fwd_check / k3_conv_cases.fwd_check compare, by name.  flats: the output buffers
    on the CPU; stats: [2, real channels] totals or None.  `out<i>#guard`: the elements outside the slot, still NaN when nothing wrote there."""
    c = conv_case(e["mod"], e["name"])
    store = kc.store_type(c, e["dt"]) if e["mod"] == "kc" else (torch.float32 if c["op"] == "head" else DT[e["dt"]])
    bnd = kr.conv_bound(r, store)
    got, ref, bd = {}, {}, {}
    for i, ((lc, lo, n), flat) in enumerate(zip(fwd_parts(e), flats)):
        g, intact = sc.split_out(lc, flat)
        k = "out%d" % i
        got[k], ref[k], bd[k] = g, r["y"][:, lo:lo + n], bnd[:, lo:lo + n]
        got[k + "#guard"] = torch.full((1,), float("nan") if intact else 0.0)
    if c["stats"]:
        (s1, b1), (s2, b2) = r["stats"]
        got["S"], ref["S"], bd["S"] = stats[0], s1, b1
        got["Q"], ref["Q"], bd["Q"] = stats[1], s2, b2
    return got, ref, bd


def wgrad_views(e, rw, inp, dw, db, dw_guard, db_guard=None):
    """(got, ref, bound) dicts of a weight-gradient case: what small_conv_cases.wgrad_check compares"""
    c = conv_case(e["mod"], e["name"])
    st, shape = inp["strides"], tuple(inp["prior_dw"].shape)
    prior = inp["prior_dw"].double().as_strided(rw["dw"].shape, st)
    got = {"dw": dw, "dw#guard": dw_guard}
    ref = {"dw": inp["prior_dw"].double() + kr.to_layout(rw["dw"], st, shape)}
    bd = {"dw": kr.to_layout(kr.wgrad_bound(rw, prior), st, shape)}
    if c["db"]:
        got["db"], ref["db"], bd["db"] = db, inp["prior_db"].double() + rw["db"], kr.wgrad_bound(rw, inp["prior_db"], which="db")
        if db_guard is not None:
            got["db#guard"] = db_guard
    return got, ref, bd


# ---- the other families: small ragged cases of their own --------------------------------------------------------------------------------------------------------
# Shapes: the smallest ragged ones of the per-kernel tests (tests/test_pointwise_loads_gpu.py, test_act_bwd_loads_gpu.py, test_residual_kernels_gpu.py):
# N = 2 at 6 x 10, one 2 x 4 x 6 volume, 3 x 5 x 7, C = 8 / 16 / 24 (32 where a kernel wants C / 8 to divide 256: act_bwd, the channel sums).  positions: launches the op records per lane.  Sources: small_conv_cases.make_source kinds.
def _o(name, kind, dt, positions=1, **p):
    return dict(id=name, kind=kind, dt=dt, positions=positions, **p)


OTHER = [
    # first conv (Cin = 1): bf16 takes the MFMA kernel <D3, 16-pixel tiles per block row 4 / 5> (5 when W wastes less: W = 70), fp32 the scalar one
    _o("c1f_2d_t4_bf16", "c1f", BF, shape=(2, 1, 9, 37), dims=2), _o("c1f_2d_t5_bf16", "c1f", BF, shape=(2, 1, 9, 70), dims=2),
    _o("c1f_3d_t4_bf16", "c1f", BF, shape=(2, 3, 5, 37), dims=3), _o("c1f_3d_t5_bf16", "c1f", BF, shape=(1, 3, 5, 70), dims=3),
    _o("c1f_2d_f32", "c1f", F32, shape=(2, 1, 9, 37), dims=2), _o("c1f_3d_f32", "c1f", F32, shape=(2, 3, 5, 19), dims=3),
    # ... and bf16 on the scalar kernel, which only the lab knob CHAP_C1_MFMA=0 picks; the knob is read once per process, so these two run in a child
    # process that has it set from the start (env: the GPU file runs every case with an `env` there)
    _o("c1f_2d_plain_bf16", "c1f", BF, shape=(2, 1, 9, 37), dims=2, env={"CHAP_C1_MFMA": "0"}),
    _o("c1f_3d_plain_bf16", "c1f", BF, shape=(2, 3, 5, 19), dims=3, env={"CHAP_C1_MFMA": "0"}),
    _o("c1b_2d_bf16", "c1b", BF, 2, shape=(2, 1, 9, 37), dims=2), _o("c1b_3d_bf16", "c1b", BF, 2, shape=(2, 3, 5, 19), dims=3),
    _o("c1b_2d_f32", "c1b", F32, 2, shape=(2, 1, 9, 37), dims=2), _o("c1b_3d_f32", "c1b", F32, 2, shape=(2, 3, 5, 19), dims=3),
    _o("bn_finalize_c24_x4", "bnfin", F32, C=24, nsub=4, nslots=3), _o("bn_eval_c70", "bneval", F32, C=70),
    # pool: plain = 2D without mask / multipliers; general = 3D or with them
    _o("pool_plain_bf16", "pool", BF, shape=(2, 1, 6, 10), C=24, src="ar"), _o("pool_plain_f32", "pool", F32, shape=(2, 1, 6, 10), C=8, src="p"),
    _o("pool_keep_bf16", "pool", BF, shape=(2, 1, 6, 10), C=16, src="ark"), _o("pool_3d_f32", "pool", F32, shape=(2, 2, 4, 6), C=8, src="arm"),
    # up-sampling: cell-plain (no mask / multipliers), cell (with them), generic (an axis of length 1), 2D and 3D
    _o("up_cellplain_2d_bf16", "up", BF, shape=(2, 1, 3, 5), C=24, src="ar", dims=2, hp=0, slot=True),
    _o("up_cellplain_3d_f32", "up", F32, shape=(2, 2, 3, 4), C=16, src="p", dims=3, hp=1, slot=False),
    _o("up_cellplain_2d_f32", "up", F32, shape=(2, 1, 3, 5), C=8, src="ar", dims=2, hp=1, slot=False),
    _o("up_cellplain_3d_bf16", "up", BF, shape=(2, 2, 3, 4), C=8, src="ar", dims=3, hp=0, slot=True),
    _o("up_cell_2d_bf16", "up", BF, shape=(2, 1, 3, 5), C=16, src="ark", dims=2, hp=0, slot=True),
    _o("up_cell_2d_f32", "up", F32, shape=(2, 1, 3, 5), C=16, src="arm", dims=2, hp=0, slot=False),
    _o("up_cell_3d_bf16", "up", BF, shape=(2, 2, 3, 4), C=16, src="arm", dims=3, hp=0, slot=False),
    _o("up_cell_3d_f32", "up", F32, shape=(2, 2, 3, 4), C=8, src="arm", dims=3, hp=1, slot=True),
    _o("up_generic_bf16", "up", BF, shape=(2, 1, 1, 5), C=8, src="ar", dims=2, hp=0, slot=False),
    _o("up_generic_f32", "up", F32, shape=(2, 1, 3, 4), C=8, src="ar", dims=3, hp=0, slot=False),
    _o("upbwd_2d_bf16", "upbwd", BF, shape=(2, 1, 3, 5), C=24, dims=2), _o("upbwd_3d_f32", "upbwd", F32, shape=(2, 2, 3, 4), C=8, dims=3),
    _o("upbwd_3d_bf16", "upbwd", BF, shape=(2, 2, 3, 4), C=16, dims=3), _o("upbwd_2d_f32", "upbwd", F32, shape=(2, 1, 3, 5), C=16, dims=2),
    # act_bwd: reduce + sum + apply; the special instance (one gradient, nothing else) and the general one (pooled gradient, multipliers, three gradients)
    _o("actbwd_one_bf16", "actbwd", BF, 3, shape=(2, 1, 6, 10), C=16, ng=1, pool=False, src="ar"),
    _o("actbwd_one_f32", "actbwd", F32, 3, shape=(2, 2, 4, 6), C=8, ng=1, pool=False, src="ark"),
    _o("actbwd_gen_bf16", "actbwd", BF, 3, shape=(2, 1, 6, 10), C=32, ng=2, pool=True, src="arm"),
    _o("actbwd_gen_f32", "actbwd", F32, 3, shape=(2, 1, 6, 10), C=16, ng=3, pool=True, src="ar"),
    # layout copies: the 8-channel vector kernel (max(C, cpad), ld, coff all multiples of 8) and the scalar one
    _o("p2cl8_bf16", "p2cl", BF, C=1, ld=16, coff=0, cpad=16), _o("p2cl8_f32", "p2cl", F32, C=3, ld=32, coff=8, cpad=8),
    _o("p2cl_bf16", "p2cl", BF, C=3, ld=12, coff=4, cpad=5), _o("p2cl_f32", "p2cl", F32, C=3, ld=3, coff=0, cpad=0),
    _o("cl2p_bf16", "cl2p", BF, C=4, src="ar"), _o("cl2p_f32", "cl2p", F32, C=2, src="sl"),
    # channel sums: with mask / multipliers in flight, without; each followed by the final kernel
    _o("chansum_km_bf16", "chansum", BF, 2, shape=(2, 1, 5, 6), C=16, src="ark"), _o("chansum_km_f32", "chansum", F32, 2, shape=(2, 2, 3, 5), C=8, src="arm"),
    _o("chansum_bf16", "chansum", BF, 2, shape=(2, 1, 5, 6), C=32, src="ar"), _o("chansum_f32", "chansum", F32, 2, shape=(2, 1, 5, 6), C=8, src="p"),
    # ... and the form with 64-bit offsets, which only a source of 2^32 bytes reaches (src_fits32: pixels * max(ld, C) * element bytes): ONE raw tensor of
    # 4 GiB with rows of 512 channels, drawn on the device and shared by the lanes; lane k sums the 8 channels from BIG_COFF(k) on (the same shapes,
    # other data), with an affine + LeakyReLU of its own.  A fault of this form shows only at this size.
    _o("chansum_big_bf16", "chansum_big", BF, 2, shape=(4, 1, 1024, 1024), C=8, ld=512), _o("chansum_big_f32", "chansum_big", F32, 2, shape=(2, 1, 1024, 1024), C=8, ld=512),
    _o("keep_mask", "keepmask", F32, n=1003, p=0.3), _o("chan_mask", "chanmask", F32, n=301, p=0.3),
    _o("fold_bf16", "fold", BF, B=4, U=2, C=24), _o("fold_f32", "fold", F32, B=4, U=4, C=8),
    # residual block: forward (up + skip; the image), backward (with and without dxin), gradient sum
    _o("resfwd_bf16", "resfwd", BF, C=32, nsrc=2), _o("resfwd_xin_f32", "resfwd", F32, C=16, nsrc=0),
    _o("resbwd_bf16", "resbwd", BF, C=32, ng=3, cm=True, dxin=False), _o("resbwd_f32", "resbwd", F32, C=16, ng=2, cm=False, dxin=False),
    _o("resbwd_dxin_bf16", "resbwd", BF, C=16, ng=1, cm=False, dxin=True), _o("resbwd_dxin_f32", "resbwd", F32, C=16, ng=3, cm=True, dxin=True),
    _o("gradsum_bf16", "gradsum", BF, C=32, ng=4), _o("gradsum_f32", "gradsum", F32, C=16, ng=2),
]
OTHER_BY_ID = {c["id"]: c for c in OTHER}
assert len(OTHER_BY_ID) == len(OTHER)
OTHER_BY_ID["actbwd_gen_twin_f32"] = dict(OTHER_BY_ID["actbwd_gen_bf16"], id="actbwd_gen_twin_f32", dt=F32)      # (a twin as TWINS above)
BIG_SEED = 4242
BIG_COFF = lambda lane: 8 + 64 * lane                      # lane k's channel slice of the shared 512-channel rows
RES_SP = (3, 5, 7)                                          # the residual kernels' grid (odd: ragged last wave and block), N = 2


def _g(case, lane):
    return torch.Generator().manual_seed(sum(map(ord, case["id"])) * 2 + sc.LANE_SEED * lane)


def _rq(x, dt):
    return x.to(DT[dt]).float()


def _sp(shape):
    N, D, H, W = shape
    return (D, H, W)


def other_inputs(case, lane=0):
    """CPU tensors of one lane of an OTHER case: activations NCDHW fp32 holding storage-type values; sources as small_conv_cases.make_source draws them"""
    c, g, dt = case, _g(case, lane), case["dt"]
    k = c["kind"]
    r = lambda *s: torch.randn(*s, generator=g)
    if k in ("c1f", "c1b"):
        N, D, H, W = c["shape"]
        taps = 3 ** c["dims"]
        d = dict(x=r(N, D, H, W), w=r(16, 1, *([3] * c["dims"])) / taps ** 0.5, b=r(16), c0=r(16) * 0.3)
        if k == "c1b":
            d.update(g=_rq(r(N, 16, D, H, W), dt), prior_dw=r(16, 1, *([3] * c["dims"])) * 0.5, prior_db=r(16) * 0.5)
        return d
    if k == "bnfin":                                        # tests/test_eval_plumbing_kernels_gpu.py _bn_buffer: multiples of 2^-6, channel 0 with Q / n < (S / n)^2
        C, nsub, ns = c["C"], c["nsub"], c["nslots"]
        q = lambda *s: torch.randint(-256, 256, s, generator=g).float() / 64
        S, Q = q(ns, C * nsub) * 4, q(ns, C * nsub).abs() * 64 + 40
        S.view(ns, nsub, C)[:, :, 0], Q.view(ns, nsub, C)[:, :, 0] = 8.0, 0.5
        return dict(S=S, Q=Q, count=64 * ns * nsub, gamma=torch.rand(C, generator=g) + 0.5, beta=r(C) * 0.2, shift=r(C) * 0.5, rm=r(C) * 0.1,
                    rv=torch.rand(C, generator=g) + 0.5)
    if k == "bneval":
        C = c["C"]
        return dict(gamma=torch.rand(C, generator=g) + 0.5, beta=r(C), rm=r(C), rv=torch.rand(C, generator=g) * 2)
    if k in ("pool", "up", "chansum"):
        N = c["shape"][0]
        d = dict(src=sc.make_source(c["src"], N, c["C"], _sp(c["shape"]), DT[dt], g))
        if k == "chansum":
            d["prior"] = r(c["C"])
        return d
    if k == "upbwd":
        N, D, H, W = c["shape"]
        fine = ((2 * D) if c["dims"] == 3 else D, 2 * H, 2 * W)
        return dict(g=_rq(r(N, c["C"], *fine), dt))
    if k == "actbwd":
        N, D, H, W = c["shape"]
        C = c["C"]
        d = dict(src=sc.make_source(c["src"], N, C, (D, H, W), DT[dt], g), grads=[_rq(r(N, C, D, H, W), dt) for _ in range(c["ng"])],
                 mean=r(C) * 0.1, invstd=torch.rand(C, generator=g) + 0.5, gamma=torch.rand(C, generator=g) + 0.5, prior=r(2, C) * 0.5, count=N * D * H * W)
        if c["pool"]:
            d.update(gp=_rq(r(N, C, D, H // 2, W // 2), dt), idx=torch.randint(0, 4, (N, C, D, H // 2, W // 2), generator=g).to(torch.uint8))
        return d
    if k == "p2cl":
        return dict(x=r(2, c["C"], 3, 9, 7))
    if k == "cl2p":
        return dict(src=sc.make_source(c["src"], 2, c["C"], RES_SP, DT[dt], g))
    if k == "chansum_big":                                  # (the raw tensor: BIG_SEED, on the device)
        C = c["C"]
        return dict(coff=BIG_COFF(lane), scale=torch.rand(C, generator=g) + 0.5, shift=r(C) * 0.2, prior=r(C))
    if k in ("keepmask", "chanmask"):
        return dict(seed=77 + 1000 * lane)
    if k == "fold":
        B, U, C = c["B"], c["U"], c["C"]
        return dict(g=_rq(r(B + U, C, 1, 5, 7), dt), mul=torch.cat((torch.full((B, C), float("nan")), (torch.rand(U, C, generator=g) > 0.4).float() * 1.7)))
    if k == "resfwd":
        C, sh = c["C"], (2, c["C"]) + RES_SP
        d = dict(r=_rq(r(*sh), dt), rs=torch.rand(C, generator=g) + 0.5, rb=r(C) * 0.3)
        if c["nsrc"] == 0:
            d["xin"] = r(2, 1, *RES_SP)
        else:
            d.update(a=sc.make_source("arm", 2, C, RES_SP, DT[dt], g), b=sc.make_source("sl", 2, C, RES_SP, DT[dt], g))
        return d
    if k in ("resbwd", "gradsum"):
        C, sh = c["C"], (2, c["C"]) + RES_SP
        d = dict(grads=[_rq(r(*sh), dt) for _ in range(c["ng"])])
        if k == "resbwd":
            d.update(o=_rq(r(*sh).clamp_min(0), dt), cm=(torch.rand(2, C, generator=g) >= 0.5).float() * 2.0 if c["cm"] else None)
        return d
    raise KeyError(k)


# ---- the table: one entry per launch site ------------------------------------------------------------------------------------------------------------------------
def _e(file, kernel, name, cases, note=""):
    return dict(site=(file, kernel, name), cases=list(cases), note=note)


def _ids(rows, **want):
    return [r["id"] for r in rows if all(r["want"].get(k) == v for k, v in want.items())]


def _oth(kind, dt=None, **p):
    return [c["id"] for c in OTHER if c["kind"] == kind and (dt is None or c["dt"] == dt) and all(c.get(k) == v for k, v in p.items())]


PW = "pointwise.hip"
ENTRIES = [
    # conv forward: the generic kernel of every geometry family, the 1x1x1 head, the wave-private and K-parallel kernels
    _e("conv_dispatch.inc", "ptr", "chap_conv_fwd", _ids(FWD, route="generic")),
    _e("conv_inst_bf16_g3.hip", "conv_head1x1_kernel<bf16_t>", "chap_conv_fwd(head)", _ids(FWD, route="head")),
    _e("conv_wp_bf16.hip", "ptr", "chap_conv_fwd(wp)", _ids(FWD, route="wp")),
    _e("conv_kpar_bf16.hip", "ptr", "name", _ids(FWD, route="kpar")),
    # weight gradient (chap_grouped_z: the group index is blockIdx.z / base_z) and its two reduce instances
    _e("wgrad_dispatch.inc", "ptr", "who", [r["id"] for r in WGRAD]),
    _e("wgrad_api.hip", "wgrad_reduce_kernel<64>", "chap_wgrad(reduce)", _ids(WGRAD, reduce=64)),
    _e("wgrad_api.hip", "wgrad_reduce_kernel<8>", "chap_wgrad(reduce)", _ids(WGRAD, reduce=8)),
    # first conv
    _e(PW, "conv_c1_mfma_kernel<true,5>", "chap_conv_c1_fwd(mfma)", ["c1f_3d_t5_bf16"]), _e(PW, "conv_c1_mfma_kernel<true,4>", "chap_conv_c1_fwd(mfma)", ["c1f_3d_t4_bf16"]),
    _e(PW, "conv_c1_mfma_kernel<false,5>", "chap_conv_c1_fwd(mfma)", ["c1f_2d_t5_bf16"]), _e(PW, "conv_c1_mfma_kernel<false,4>", "chap_conv_c1_fwd(mfma)", ["c1f_2d_t4_bf16"]),
    _e(PW, "conv_c1_fwd_kernel<bf16_t,true,16>", "chap_conv_c1_fwd", ["c1f_3d_plain_bf16"]), _e(PW, "conv_c1_fwd_kernel<bf16_t,false,16>", "chap_conv_c1_fwd", ["c1f_2d_plain_bf16"]),
    _e(PW, "conv_c1_fwd_kernel<float,true,16>", "chap_conv_c1_fwd", ["c1f_3d_f32"]), _e(PW, "conv_c1_fwd_kernel<float,false,16>", "chap_conv_c1_fwd", ["c1f_2d_f32"]),
    _e(PW, "conv_c1_bwd_kernel<bf16_t,true,16>", "chap_conv_c1_bwd", ["c1b_3d_bf16"]), _e(PW, "conv_c1_bwd_kernel<bf16_t,false,16>", "chap_conv_c1_bwd", ["c1b_2d_bf16"]),
    _e(PW, "conv_c1_bwd_kernel<float,true,16>", "chap_conv_c1_bwd", ["c1b_3d_f32"]), _e(PW, "conv_c1_bwd_kernel<float,false,16>", "chap_conv_c1_bwd", ["c1b_2d_f32"]),
    _e(PW, "conv_c1_reduce_kernel<16>", "chap_conv_c1_bwd(reduce)", _oth("c1b")),
    _e(PW, "bn_finalize_kernel", "chap_bn_finalize", _oth("bnfin")), _e(PW, "bn_eval_kernel", "chap_bn_eval_affine", _oth("bneval")),
    _e(PW, "act_pool2_plain_kernel<T>", "chap_act_pool2", ["pool_plain_bf16", "pool_plain_f32"]),
    _e(PW, "act_pool2_kernel<T>", "chap_act_pool2", ["pool_keep_bf16", "pool_3d_f32"]),
    _e(PW, "upsample2x_cell_kernel<T,D3>", "chap_upsample2x", ["up_cell_2d_bf16", "up_cell_2d_f32", "up_cell_3d_bf16", "up_cell_3d_f32"]),
    _e(PW, "upsample2x_cell_plain_kernel<T,false,true,D3>", "chap_upsample2x", ["up_cellplain_2d_bf16", "up_cellplain_2d_f32", "up_cellplain_3d_bf16", "up_cellplain_3d_f32"]),
    _e(PW, "upsample2x_kernel<bf16_t>", "chap_upsample2x", ["up_generic_bf16"]), _e(PW, "upsample2x_kernel<float>", "chap_upsample2x", ["up_generic_f32"]),
    _e(PW, "upsample2x_bwd_kernel<bf16_t>", "chap_upsample2x_bwd", _oth("upbwd", BF)), _e(PW, "upsample2x_bwd_kernel<float>", "chap_upsample2x_bwd", _oth("upbwd", F32)),
    _e(PW, "act_bwd_kernel<T,APPLY,false>", "name", ["actbwd_one_bf16", "actbwd_one_f32"]), _e(PW, "act_bwd_kernel<T,APPLY,true>", "name", ["actbwd_gen_bf16", "actbwd_gen_f32"]),
    _e(PW, "act_bwd_sum_kernel", "chap_act_bwd_reduce(sum)", _oth("actbwd")),
    _e(PW, "planar_to_cl8_kernel<bf16_t>", "chap_planar_to_cl", ["p2cl8_bf16"]), _e(PW, "planar_to_cl8_kernel<float>", "chap_planar_to_cl", ["p2cl8_f32"]),
    _e(PW, "planar_to_cl_kernel<bf16_t>", "chap_planar_to_cl", ["p2cl_bf16"]), _e(PW, "planar_to_cl_kernel<float>", "chap_planar_to_cl", ["p2cl_f32"]),
    _e(PW, "cl_to_planar_kernel<bf16_t>", "chap_cl_to_planar", ["cl2p_bf16"]), _e(PW, "cl_to_planar_kernel<float>", "chap_cl_to_planar", ["cl2p_f32"]),
    _e(PW, "channel_sum_kernel<T,true,false>", "chap_channel_sum", ["chansum_big_bf16", "chansum_big_f32"]),
    _e(PW, "channel_sum_kernel<T,true,true>", "chap_channel_sum", ["chansum_km_bf16", "chansum_km_f32"]),
    _e(PW, "channel_sum_kernel<T,false,true>", "chap_channel_sum", ["chansum_bf16", "chansum_f32"]),
    _e(PW, "channel_sum_final_kernel", "chap_channel_sum(final)", _oth("chansum") + _oth("chansum_big")),
    _e("aux.hip", "keepmask_kernel", "chap_keep_mask", ["keep_mask"]), _e("aux.hip", "chanmask_kernel", "chap_chan_mask", ["chan_mask"]),
    _e("chandrop.hip", "fold_perturbed_kernel<bf16_t>", "chap_fold_perturbed", ["fold_bf16"]), _e("chandrop.hip", "fold_perturbed_kernel<float>", "chap_fold_perturbed", ["fold_f32"]),
    _e("residual.hip", "residual_fwd_kernel<bf16_t>", "chap_residual_fwd", _oth("resfwd", BF)), _e("residual.hip", "residual_fwd_kernel<float>", "chap_residual_fwd", _oth("resfwd", F32)),
    _e("residual.hip", "residual_bwd_kernel<bf16_t,true>", "chap_residual_bwd(dxin)", ["resbwd_dxin_bf16"]),
    _e("residual.hip", "residual_bwd_kernel<float,true>", "chap_residual_bwd(dxin)", ["resbwd_dxin_f32"]),
    _e("residual.hip", "residual_bwd_kernel<bf16_t,false>", "chap_residual_bwd", ["resbwd_bf16"]), _e("residual.hip", "residual_bwd_kernel<float,false>", "chap_residual_bwd", ["resbwd_f32"]),
    _e("residual.hip", "grad_sum_kernel<bf16_t>", "chap_grad_sum", ["gradsum_bf16"]), _e("residual.hip", "grad_sum_kernel<float>", "chap_grad_sum", ["gradsum_f32"]),
]
ALL_CASE_IDS = [r["id"] for r in FWD + WGRAD] + [c["id"] for c in OTHER]
ENV_CASE_IDS = [c["id"] for c in OTHER if c.get("env")]      # need a process of their own (a read-once knob)
HERE_CASE_IDS = [i for i in ALL_CASE_IDS if i not in ENV_CASE_IDS]


def uncovered():
    """the launch sites without a merged-grid case, with the reason (DESIGN.md lists them)"""
    return {e["site"]: e["note"] for e in ENTRIES if not e["cases"]}


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def check_lanes(single, grouped, refs, bounds, who="", differ=True):
    """The one check of a merged launch.  single / grouped: per lane, {name: CPU tensor} of what the one-by-one launches and the merged grid(s) left;
    refs / bounds: per lane, {name: fp64 reference / per-element bound (None: equal exactly)} for the names that have one.
      - every tensor of the merged run equals the single launch's, bit for bit;
      - every referenced tensor is per element within its bound of ITS lane's reference (a NaN prefill left standing fails: kernel_ref.check);
      - `<name>#guard` tensors are still all NaN (uint8: still 0xAB);
      - every referenced tensor differs between any two lanes (the lanes have different data: a lane run on another lane's arguments shows).
    Returns the worst error / bound."""
    n = len(grouped)
    assert n >= 2 and len(single) == len(refs) == len(bounds) == n, (who, n, len(single), len(refs), len(bounds))
    worst = 0.0
    for k in range(n):
        assert set(single[k]) == set(grouped[k]) and set(refs[k]) <= set(grouped[k]) and set(refs[k]) == set(bounds[k]), (who, k)
        assert refs[k], (who, k, "nothing to compare")
        for name, t in grouped[k].items():
            tag = "%s lane %d %s" % (who, k, name)
            assert t is not None and same_bits(single[k][name], t), tag + ": the merged launch and the single launch differ"
            if name.endswith("#guard"):
                ok = (t == 0xAB).all() if t.dtype == torch.uint8 else torch.isnan(t).all()
                assert bool(ok), tag + ": written outside the output"
            elif name in refs[k]:
                if bounds[k][name] is None:
                    assert same_bits(t, refs[k][name].to(t.dtype)), tag + ": not the reference's value"
                else:
                    worst = max(worst, kr.check(tag, t, refs[k][name], bounds[k][name], dims="?" * t.dim()))
    if differ:
        for i in range(n):
            for j in range(i + 1, n):
                for name in refs[i]:
                    if name in refs[j] and grouped[i][name].shape == grouped[j][name].shape:
                        assert not same_bits(grouped[i][name], grouped[j][name]), "%s: lanes %d and %d hold the same %s" % (who, i, j, name)
    return worst


# ---- planted faults of a merged weight-gradient launch, for the checker's own proof (tests/test_group_cases_cpu.py) ------------------------------------------------------
FAULTS = ("lane_on_lane0_args", "lanes_swapped", "base_z_slip", "shared_workspace", "lane_dropped_beyond_4", "guard_written")


def plant(fault, results, bn):
    """results: per lane {dw [kn, kc, taps], dw#guard, db, db#guard} of a fault-free run (clones are changed); bn: the B tile width (base_z = ceil(kn / bn) > 1)"""
    res = [{k: v.clone() for k, v in lane.items()} for lane in results]
    nan = float("nan")
    if fault == "lane_on_lane0_args":                       # every block ran on G.p[0]: lane 0 written twice, the others left at their prefill
        for lane in res[1:]:
            lane["dw"].fill_(nan)
            lane["db"].fill_(nan)
    elif fault == "lanes_swapped":
        res[0], res[1] = res[1], res[0]
    elif fault == "base_z_slip":                            # group = blockIdx.z / base_z off by one: lane 1's first B chunk lands in lane 0's second
        assert res[0]["dw"].shape[0] > bn
        hi = min(2 * bn, res[0]["dw"].shape[0])
        res[0]["dw"][bn:hi] = res[1]["dw"][:hi - bn]
    elif fault == "shared_workspace":                       # two lanes' partial slabs in one workspace: both reductions total both
        tot = {k: res[0][k] + res[1][k] for k in ("dw", "db")}
        for lane in res[:2]:
            lane["dw"], lane["db"] = tot["dw"].clone(), tot["db"].clone()
    elif fault == "lane_dropped_beyond_4":
        assert len(res) > MAX_LANES
        res[MAX_LANES]["dw"].fill_(nan)
        res[MAX_LANES]["db"].fill_(nan)
    elif fault == "guard_written":
        res[-1]["dw#guard"][3] = 0.0
    else:
        raise KeyError(fault)
    return res
