"""The launch planners of chap_conv_fwd / chap_wgrad (chap_amd/csrc/conv_plan.h, wgrad_plan.h) without a GPU: a small stand-alone
program (tests/plan_probe.py), built with the host compiler from the two headers and error.cpp, prints the plan for a list of params.

The expected plans of the bench layers (tests/golden/launch_plan_parent.csv) were read off a kernel trace of the commit BEFORE the planners
existed (310a87c): one eager bench-shaped step per configuration under `rocprofv3 --kernel-trace -- python3 tools/shape_table.py
--config C --dtype D --trace-plan ...`, joined with tools/shape_join.py (profiles/r06_plan_parent_*.csv; the golden file keeps the conv_fwd
and wgrad rows' op / shape / launch columns).  A kernel's instance name carries the template arguments the dispatch picked (KC, NT, MR,
CPAR, BN, ...), its grid the split count."""
import csv
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chap_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_parent.csv")
F32, BF16 = 0, 1
EINVAL, EUNSUPPORTED = -1, -2

from tests.plan_probe import probe                         # noqa: F401 (the fixture: one copy of the probe for every test that plans)


# ---- the bench layers -------------------------------------------------------------------------------------------------------------------
def _spatial(dims, at):
    v = [int(x) for x in at.split("x")]
    return dict(zip("DHW", v)) if dims == 3 else dict(D=1, H=v[0], W=v[1])


def _conv_request(shape, dtype):
    """tools/shape_table.py's conv_fwd shape string -> (request line, Ck, taps)"""
    m = re.match(r"(\d)D k(\d) s(\d) (\S+)->(\d+) @(\S+) N=(\d+)(.*) src=(\S+)$", shape)
    dims, k, s, srcs, cout, at, n, flags, lazy = m.groups()
    dims, k = int(dims), int(k)
    add = "add" in srcs
    cs = [int(c) for c in re.split(r"add|\+", srcs)]
    keep = ["k" in f for f in lazy.split(",")]
    f = dict(dims=dims, k=k, s=s, N=n, Cout=cout, nsrc=len(cs), combine=int(add), C0=cs[0], C1=cs[1] if len(cs) > 1 else 0, dtype=dtype,
             keep0=int(keep[0]), keep1=int(len(keep) > 1 and keep[1]), d2s=int(" d2s" in flags), Cn=int(cout) // 2 ** dims,
             planar=int(" planar" in flags), stats=int(" stats" in flags), f32out=int(" f32out" in flags), **_spatial(dims, at))
    return "conv " + " ".join("%s=%s" % kv for kv in f.items()), (cs[0] if add else sum(cs)), k ** dims


def _wgrad_request(shape, dtype, add2):
    m = re.match(r"(\d)D k(\d) s(\d) A=(\S+) B=(\d+) @(\S+) N=(\d+) ", shape)
    dims, k, s, a, cb, at, n = m.groups()
    cs = [int(c) for c in a.split("+")]
    f = dict(dims=int(dims), k=k, s=s, N=n, Cb=cb, na=len(cs), combine=int(add2), C0=cs[0], C1=cs[1] if len(cs) > 1 else 0, dtype=dtype, **_spatial(int(dims), at))
    return "wgrad " + " ".join("%s=%s" % kv for kv in f.items())


def _instance(launch, body):
    """`body<a,b,...>: grid=XxYxZ lds=L` of the launch column -> (template arguments, grid) or None"""
    m = re.search(body + r"<([^>]*)>: grid=(\d+)x(\d+)x(\d+) lds=\d+(?:$| \|)", launch)
    if not m:
        return None
    conv = {"true": 1, "false": 0, "bf16": BF16, "f32": F32}
    return [conv[a] if a in conv else int(a) for a in m.group(1).split(",")], tuple(int(x) for x in m.group(2, 3, 4))


def _expected_conv(launch):
    """what the parent's dispatch instantiated, in plan terms"""
    i = _instance(launch, "conv_fwd_kernel")        # <T, KS, ST, D3, KC, NT, MR, ADD2, WLDS, ZW, ONE>
    if i:
        return dict(route="generic", KC=i[0][4], NT=i[0][5], MR=i[0][6], cpar=0)
    i = _instance(launch, "conv_wp_kernel")         # <KC, NT, LANESEL>, 4 x 16 tiles
    if i:
        return dict(route="wp", KC=i[0][0], NT=i[0][1], MR=1, cpar=0)
    i = _instance(launch, "conv_kpar_kernel")       # <T, D3, KC, NT, CPAR, ONE>, 3D: 4 x 16 tiles, 2D: 8 x 16
    if i:
        return dict(route="kpar", KC=i[0][2], NT=i[0][3], MR=1 if i[0][1] else 2, cpar=i[0][4])
    i = _instance(launch, "conv_kpar2d_kernel")     # <NT, CPAR, ONE, KEEPM, SINGLE>, 32-channel chunks
    if i:
        return dict(route="kpar", KC=32, NT=i[0][0], MR=2, cpar=i[0][1])
    assert "conv_head1x1_kernel" in launch, launch
    return dict(route="head")


def _expected_wgrad(launch):
    i = _instance(launch, "wgrad_kernel")           # <T, KS, ST, D3, KC, MR, ADD2, BN, PD, ZW>; grid = (nsplit, Ca / KC, ceil(Cb / BN))
    if i:
        return dict(brick=i[0][9], KC=i[0][4], bn=i[0][7], mr=0, nsplit=i[1][0]), i[1], i[0][6]
    i = _instance(launch, "wgrad_wp_kernel")        # <KC, MR, BN>
    assert i, launch
    return dict(brick=2, KC=i[0][0], bn=i[0][2], mr=i[0][1], nsplit=i[1][0]), i[1], 0


@pytest.fixture(scope="module")
def bench_layers(probe):
    """every conv / weight-gradient layer of the traced bench steps with the plan of today's planner: [(row, request, plan), ...]"""
    rows = list(csv.DictReader(open(GOLDEN)))
    reqs = []
    for r in rows:
        dtype = F32 if r["config"].endswith("fp32") else BF16
        if r["op"] == "conv_fwd":
            reqs.append(_conv_request(r["shape"], dtype)[0])
        else:
            reqs.append(_wgrad_request(r["shape"], dtype, _expected_wgrad(r["launch"])[2]))
    return list(zip(rows, reqs, probe(reqs)))


def test_bench_layers_plan_as_the_parent_trace(bench_layers):
    configs = {r["config"] for r, _, _ in bench_layers}
    assert configs == {"2d_bf16", "3d_bf16", "2d_fp32"}
    assert sum(r["op"] == "conv_fwd" for r, _, _ in bench_layers) >= 60 and sum(r["op"] == "wgrad" for r, _, _ in bench_layers) >= 40
    bad = []
    for r, req, plan in bench_layers:
        assert plan["rc"] == 0, (req, plan)
        if r["op"] == "conv_fwd":
            want = _expected_conv(r["launch"])
        else:
            want, grid, _ = _expected_wgrad(r["launch"])
            if grid != (plan["nsplit"], plan["Ca"] // plan["KC"], -(-plan["Cb"] // plan["bn"])):
                bad.append((r["config"], r["shape"], "grid", grid, plan))
        got = {k: plan[k] for k in want}
        if got != want:
            bad.append((r["config"], r["shape"], want, got))
    assert not bad, bad


def test_anchor_layers(probe):
    """the routes the comments of conv_plan.h state"""
    full16 = "conv dims=2 k=3 s=1 N=12 H=256 W=256 Cout=16 C0=16"
    a, b, c, d = probe([full16, full16 + " dtype=0",
                        "conv dims=3 k=3 s=1 N=2 D=5 H=7 W=7 Cout=256 C0=256",
                        "conv dims=3 k=3 s=1 N=2 D=20 H=28 W=28 Cout=64 C0=64"])
    assert (a["route"], a["KC"], a["ntiles"], a["NT"]) == ("wp", 16, 1, 1)
    assert (b["route"], b["geom"]) == ("generic", 1)
    assert c["route"] == "kpar" and c["cpar"] == 4
    assert d["route"] == "generic"


# ---- dims = 2 with D > 1 ----------------------------------------------------------------------------------------------------------------
def test_depth_slices_never_take_a_wave_private_kernel(probe):
    conv = "conv dims=2 k=3 s=1 N=3 D=2 H=64 W=64 Cout=16 C0=16"
    conv32 = "conv dims=2 k=3 s=1 N=3 D=2 H=64 W=64 Cout=32 C0=16 C1=16 nsrc=2"
    wg = "wgrad dims=2 k=3 s=1 N=3 D=2 H=64 W=64 C0=16 Cb=16"
    wg32 = "wgrad dims=2 k=3 s=1 N=3 D=2 H=64 W=64 C0=32 Cb=32"
    forced = "setenv CHAP_CONV_WP=1 CHAP_WGRAD_WP=1 CHAP_WGRAD_WP_MR=1"
    res = probe([conv, conv32, wg, wg32, forced, conv, conv32, wg, wg32])
    for r in res:
        assert r["rc"] == 0 and r.get("route", "generic") == "generic" and r.get("brick", 0) == 0 and r.get("mr", 0) == 0, r
    # the same layers with D = 1 do (the guard is what keeps them off, not the shape)
    for r in probe([x.replace("D=2", "D=1") for x in (conv, conv32, wg, wg32)]):
        assert r.get("route") == "wp" or r.get("brick") == 2, r


# ---- knob liveness ----------------------------------------------------------------------------------------------------------------------
def test_live_knobs_are_read_per_call_and_read_once_knobs_once(probe):
    full16 = "conv dims=2 k=3 s=1 N=12 H=256 W=256 Cout=16 C0=16"
    deep2d = "conv dims=2 k=3 s=1 N=12 H=16 W=16 Cout=256 C0=256"
    wg16 = "wgrad dims=2 k=3 s=1 N=12 H=256 W=256 C0=16 Cb=16"
    r = probe([full16, deep2d, wg16,
               "setenv CHAP_CONV_WP=0 CHAP_CONV_KPAR=1 CHAP_WGRAD_WP=0", full16, deep2d, wg16,
               "setenv CHAP_WGRAD_WP=1 CHAP_WGRAD_WP_MR=1", wg16,
               "unsetenv CHAP_CONV_WP CHAP_CONV_KPAR CHAP_WGRAD_WP CHAP_WGRAD_WP_MR", full16, deep2d, wg16])
    assert [r[0]["route"], r[1]["route"], r[2]["brick"], r[2]["mr"]] == ["wp", "generic", 2, 2]
    assert [r[3]["route"], r[4]["route"], r[5]["brick"]] == ["generic", "kpar", 0]
    assert (r[6]["brick"], r[6]["mr"]) == (2, 1)
    assert r[7:] == r[:3]
    # read once: CHAP_CONV_KC16_MAXC2D (16-channel chunks for 2D layers up to that many K channels; default 0) and
    # CHAP_WGRAD_BN16_MAXC hold the value of their first use
    c64 = "conv dims=2 k=3 s=1 N=12 H=64 W=64 Cout=64 C0=64"
    p64 = "pack kind=0 Cin=64 Cout=64 taps=9"
    wg3d = "wgrad dims=3 k=3 s=1 N=2 D=40 H=56 W=56 C0=32 Cb=32"
    a = probe([c64, p64, wg3d, "setenv CHAP_CONV_KC16_MAXC2D=64 CHAP_WGRAD_BN16_MAXC=32", c64, p64, wg3d])
    assert [a[0]["KC"], a[1]["KC"], a[2]["bn"]] == [32, 32, 32] and a[3:] == a[:3]
    b = probe(["setenv CHAP_CONV_KC16_MAXC2D=64 CHAP_WGRAD_BN16_MAXC=32", c64, p64, wg3d, "unsetenv CHAP_CONV_KC16_MAXC2D CHAP_WGRAD_BN16_MAXC", c64, p64, wg3d])
    assert [b[0]["KC"], b[1]["KC"], b[2]["bn"]] == [16, 16, 16] and b[3:] == b[:3]


# ---- packer and conv, workspace and dispatch --------------------------------------------------------------------------------------------
def test_packer_blocking_is_the_conv_plans(probe, bench_layers):
    convs = [(r, req, plan) for r, req, plan in bench_layers if r["op"] == "conv_fwd"]
    reqs, want = [], []
    for r, req, plan in convs:
        dtype = F32 if r["config"].endswith("fp32") else BF16
        _, ck, taps = _conv_request(r["shape"], dtype)
        cout = int(re.search(r"Cout=(\d+)", req).group(1))
        if " d2s" in r["shape"]:        # 1x1 conv + depth-to-space: transposed conv forward (2), k2 s2 conv input gradient (4)
            nsub = 2 ** int(r["shape"][0])
            kinds = ["kind=2 Cin=%d Cout=%d taps=%d" % (ck, cout // nsub, nsub), "kind=4 Cout=%d Cin=%d taps=%d" % (ck, cout // nsub, nsub)]
        else:                           # conv forward (0), its input gradient (1), transposed conv input gradient (3)
            kinds = ["kind=0 Cin=%d Cout=%d taps=%d" % (ck, cout, taps), "kind=1 Cout=%d Cin=%d taps=%d" % (ck, cout, taps),
                     "kind=3 Cout=%d Cin=%d taps=%d" % (ck, cout, taps)]
        for kd in kinds:
            reqs.append("pack %s dtype=%d" % (kd, dtype))
            want.append({k: plan[k] for k in ("rc", "KC", "GPT", "NP", "STEPS", "nchunks", "ntiles")})
    assert probe(reqs) == want


def test_workspace_is_sized_for_the_b_tile_the_dispatch_instantiates(bench_layers):
    for r, req, plan in bench_layers:
        if r["op"] != "wgrad":
            continue
        want, grid, _ = _expected_wgrad(r["launch"])
        assert plan["bn"] == want["bn"] and grid[2] == -(-plan["Cb"] // plan["bn"]), (r["shape"], plan)
        # nsplit slabs of taps x Ca x Cb floats + nsplit bias-gradient rows: what the kernel's grid.x blocks write and the reduction reads
        assert plan["bytes"] == grid[0] * (plan["taps"] * plan["Ca"] * plan["Cb"] + plan["Cb"]) * 4, (r["shape"], plan)


# ---- add-combine: dropout on the first source only --------------------------------------------------------------------------------------
def test_add_combine_refuses_dropout_on_the_second_source(probe):
    """The staging of an add-combined pair (conv_kernel.h halo_commit_impl, shared by the weight gradient) applies the keep mask and the channel
    multipliers of the FIRST source; on the second they used to be ignored without a word.  The nets never ask for it (2D additive skips pass
    [skip, up], the V-Net [up, skip] with dropout-free skips); now it is an error."""
    conv = "conv dims=3 k=3 s=1 N=2 D=10 H=14 W=14 Cout=64 C0=64 C1=64 nsrc=2 combine=1"
    conv2 = "conv dims=2 k=3 s=1 N=2 H=32 W=32 Cout=64 C0=64 C1=64 nsrc=2 combine=1"
    wg = "wgrad dims=3 k=3 s=1 N=2 D=10 H=14 W=14 C0=64 C1=64 na=2 combine=1 Cb=64"
    wg2 = "wgrad dims=2 k=3 s=1 N=2 H=32 W=32 C0=64 C1=64 na=2 combine=1 Cb=64"
    r = probe([conv, conv + " cm0=1", conv2 + " keep0=1", wg + " cm0=1", wg2 + " keep0=1", conv + " cm1=1", conv2 + " keep1=1", wg + " cm1=1", wg2 + " keep1=1",
               conv.replace("combine=1", "combine=0") + " cm1=1", wg.replace("combine=1", "combine=0") + " cm1=1"])
    assert [x["rc"] for x in r[:5]] == [0] * 5
    assert r[5] == r[6] == dict(rc=EUNSUPPORTED, error="chap_conv_fwd: add-combine takes a keep mask / channel multipliers on the first source only")
    assert r[7] == r[8] == dict(rc=EUNSUPPORTED, error="chap_wgrad: add-combine takes a keep mask / channel multipliers on the first source only")
    assert r[9]["rc"] == 0 and r[10]["rc"] == 0             # concatenated sources carry their own


# ---- the shapes the residual-path GPU tests chose on the CPU -------------------------------------------------------------------------------
def test_residual_source_cases_reach_the_routes_they_name(probe):
    """tests/test_kernels_gpu.py::test_conv3d_residual_sources names a route per case and tests/test_step_launches_gpu.py's residual step a
    route table: both are plans, so they are checked here (under the knobs the GPU test sets)."""
    import torch
    from tests.test_kernels_gpu import CONV3D_ROUTES
    from tests.test_step_launches_gpu import RESIDUAL_SP
    want = {"slab16": ("generic", 1, 1, 1), "brick16": ("generic", 1, 4, 1), "brick32": ("generic", 2, 4, 2), "brick64": ("generic", 2, 4, 4),
            "slab64": ("generic", 4, 1, 4), "kpar128": ("kpar", 2, 1, 8), "slab16_f32": ("generic", 1, 1, 1), "slab64_f32": ("generic", 4, 1, 4)}
    assert set(want) == set(CONV3D_ROUTES)
    for route, (dtype, (N, D, H, W), c, knobs) in CONV3D_ROUTES.items():
        base = "conv dims=3 k=3 s=1 N=%d D=%d H=%d W=%d Cout=%d C0=%d stats=1 dtype=%d" % (N, D, H, W, c, c, BF16 if dtype == torch.bfloat16 else F32)
        pre = ["setenv " + " ".join("%s=%s" % kv for kv in knobs.items())] if knobs else []
        one, add = probe(pre + [base + " cm0=1", base + " C1=%d nsrc=2 combine=1 cm0=1" % c])
        assert (one["route"], one["NT"], one["MR"], one["nchunks"]) == want[route], (route, one)
        # an add-combined launch never takes the K-parallel kernel: slabs with NT = 4 there; everywhere else the route of the single source
        assert (add["route"], add["NT"], add["MR"]) == (("generic", 4, 1) if route == "kpar128" else want[route][:3]), (route, add)
    # the residual step's shape: conv bricks and 16-wide weight-gradient bricks at level 0, 32-wide weight-gradient bricks and conv slabs at level 1,
    # the K-parallel route and weight-gradient slabs from level 2 down, the head; the next smaller shape loses the 32-wide bricks
    def level(sp, l, what):
        d, h, w = (x >> l for x in sp)
        c = 16 << l
        return "%s dims=3 k=3 s=1 N=2 D=%d H=%d W=%d C0=%d %s=%d" % (what, d, h, w, c, "Cout" if what == "conv" else "Cb", c)
    sp = RESIDUAL_SP
    assert all(x % 16 == 0 for x in sp)
    r = probe([level(sp, l, what) for l in range(5) for what in ("conv", "wgrad")] + ["conv dims=3 k=1 s=1 N=2 D=%d H=%d W=%d Cout=2 C0=16 planar=1 f32out=1" % sp])
    convs, wgs = r[0:10:2], r[1:10:2]
    assert [(x["route"], x["NT"], x["MR"]) for x in convs] == [("generic", 1, 4), ("generic", 2, 1), ("kpar", 2, 1), ("kpar", 2, 1), ("kpar", 2, 1)]
    assert [(x["brick"], x["bn"]) for x in wgs] == [(1, 16), (1, 32), (0, 32), (0, 32), (0, 32)]
    assert r[10]["route"] == "head"
    smaller = (16, 16, 32)
    assert probe([level(smaller, 1, "wgrad")])[0]["brick"] == 0


# ---- invalid params ---------------------------------------------------------------------------------------------------------------------
def test_invalid_params_keep_their_codes_and_messages(probe):
    ok = "conv dims=2 k=3 s=1 N=12 H=256 W=256 Cout=16 C0=16"
    r = probe([ok + " nsrc=3", ok + " nsrc=0", ok + " ld0=20", "conv dims=3 k=3 s=1 N=2 D=20 H=28 W=28 Cout=64 C0=64 keep0=1",
               "conv dims=3 k=3 s=1 N=2 D=20 H=28 W=28 Cout=64 C0=32 C1=32 nsrc=2 keep1=1", "conv dims=2 k=3 s=2 N=1 H=8 W=8 Cout=16 C0=16",
               "wgrad dims=2 k=3 s=1 N=1 H=8 W=8 C0=16 Cb=16 na=3", "pack kind=7 Cin=16 Cout=16 taps=9"])
    assert r[0] == dict(rc=EINVAL, error="chap_conv_fwd: nsrc=3")
    assert r[1] == dict(rc=EINVAL, error="chap_conv_fwd: nsrc=0")
    assert r[2] == dict(rc=EINVAL, error="chap_conv_fwd src: ld=20 coff=0 C=16 not 8-aligned / too small")
    assert r[3] == r[4] == dict(rc=EUNSUPPORTED, error="chap_conv_fwd: element keep masks are built for 2D only (3D: channel multipliers)")
    assert r[5] == dict(rc=EUNSUPPORTED, error="chap_conv_fwd: unsupported (ksize=3, stride=2)")
    assert r[6] == dict(rc=EINVAL, error="chap_wgrad: na=3")
    assert r[7] == dict(rc=EINVAL, error="chap_pack: kind=7")
