"""The table of merged-launch cases (tests/group_cases.py) against the sources, and its checker against planted faults; no device.

Coverage: every chap_launch< / chap_launch_z< / chap_launch_ptr< call site of chap_amd/csrc is claimed by a table entry, no entry names a site that
does not exist, and an entry without a case says why.  A kernel added behind the trampoline fails this file until it has a merged-grid case.  The conv
and weight-gradient rows reach the route, geometry family, tile family and base_z they are listed under (the planner probe of tests/plan_probe.py);
the other families' rows reach their instance by the launchers' own conditions, restated here.  check_lanes() rejects every planted fault of a merged
weight-gradient launch and accepts the fault-free set.  lane = 0 of the conv case files draws what it drew before `lane` existed."""
import math
import os
import re

import pytest
import torch

from tests import group_cases as gc
from tests import k3_conv_cases as kc
from tests import kernel_ref as kr
from tests import small_conv_cases as sc
from tests.plan_probe import probe      # noqa: F401 (fixture)


def coverage_errors(entries, sites):
    claimed = [e["site"] for e in entries]
    errs = ["launch site without a table entry: %s" % (s,) for s in sorted(sites - set(claimed))]
    errs += ["table entry for a site that does not exist: %s" % (s,) for s in sorted(set(claimed) - sites)]
    errs += ["site claimed twice: %s" % (s,) for s in sorted({s for s in claimed if claimed.count(s) > 1})]
    errs += ["entry with neither a case nor a reason: %s" % (e["site"],) for e in entries if not e["cases"] and not e["note"]]
    return errs


def test_every_launch_site_has_a_merged_grid_case():
    sites = gc.scan_sites()
    assert len(sites) >= 50 and ("pointwise.hip", "bn_finalize_kernel", "chap_bn_finalize") in sites, len(sites)
    assert not coverage_errors(gc.ENTRIES, sites), coverage_errors(gc.ENTRIES, sites)
    known = set(gc.ALL_CASE_IDS)
    used = {c for e in gc.ENTRIES for c in e["cases"]}
    assert used == known, (sorted(used - known), sorted(known - used))                        # every named case exists, every case sits under a site
    # the checks see what they are for: a site the table does not know, a site that is gone, an entry emptied
    assert coverage_errors(gc.ENTRIES, sites | {("pointwise.hip", "dummy_kernel", "chap_dummy")})
    assert coverage_errors(gc.ENTRIES[1:], sites) and coverage_errors(gc.ENTRIES + [gc._e("aux.hip", "gone_kernel", "chap_gone", ["keep_mask"])], sites)
    assert not gc.uncovered()                               # no site is left without a case
    # a case that needs a knob which is read once per process says so, and only such knobs are named (the GPU file gives them a child process)
    assert {k for i in gc.ENV_CASE_IDS for k in gc.OTHER_BY_ID[i]["env"]} == {"CHAP_C1_MFMA"} and len({str(gc.OTHER_BY_ID[i]["env"]) for i in gc.ENV_CASE_IDS}) == 1
    knobs = open(os.path.join(gc.CSRC, "knobs.h")).read()
    assert re.search(r"X\(C1_MFMA,\s*ANY,\s*1,\s*ONCE\)", knobs)


def test_a_site_added_to_a_copy_of_the_sources_fails_the_coverage(tmp_path):
    """the scanner on a modified tree: a copy of csrc with one more chap_launch< call in aux.hip has a site the table does not know"""
    import os
    import shutil
    for fn in os.listdir(gc.CSRC):
        if fn.endswith((".hip", ".inc", ".h", ".cpp")):
            shutil.copy(os.path.join(gc.CSRC, fn), tmp_path / fn)
    assert gc.scan_sites(str(tmp_path)) == gc.scan_sites()
    with open(tmp_path / "aux.hip", "a") as f:
        f.write('\nstatic int dummy(hipStream_t s, const chap_keepmask_params* p) {\n'
                '    return chap_launch<chap_keepmask_params, dummy_kernel, 256>(dim3(1), dim3(256), 0, s, *p, "chap_dummy");\n}\n')
    assert coverage_errors(gc.ENTRIES, gc.scan_sites(str(tmp_path))) == ["launch site without a table entry: ('aux.hip', 'dummy_kernel', 'chap_dummy')"]


def test_scanner_reads_a_site_as_written(tmp_path):
    (tmp_path / "x.hip").write_text('int f() {\n    if (a) return chap_launch<my_params, my_kernel<bf16_t, true>, 256, 2>(dim3(g(1, 2)), dim3(256), 0, s, *p, "chap_my(op)");\n'
                                    '    return chap_launch_ptr<my_params>(kern, grid,\n        dim3(256), lds, stream, a, who);\n}\n')
    (tmp_path / "launch.h").write_text("static int chap_launch(int) { return chap_launch_ptr<A>(k, g, b, l, s, a, name); }\n")
    assert gc.scan_sites(str(tmp_path)) == {("x.hip", "my_kernel<bf16_t,true>", "chap_my(op)"), ("x.hip", "ptr", "who")}


def test_required_conv_cases_are_in_the_table():
    """what the table must hold: every forward route, every weight-gradient family, base_z 1 / 2 / >= 3, db, kn_valid and kc_valid"""
    fw = [(r["want"]["route"], r["want"]["geom"]) for r in gc.FWD]
    assert {("generic", g) for g in (1, 2, 3, 4, 5)} <= set(fw) and {"head", "wp", "kpar"} <= {r for r, _ in fw}
    assert {r["want"].get("kpar2d") for r in gc.FWD if r["want"]["route"] == "kpar"} == {True, False}
    assert {r["want"]["fam"] for r in gc.WGRAD} == {"generic2d", "generic3d", "wp", "brick", "k1", "k2s2"}
    bz = {r["want"]["base_z"] for r in gc.WGRAD}
    assert 1 in bz and 2 in bz and any(b >= 3 for b in bz)
    assert any(r["want"]["db"] for r in gc.WGRAD) and {"kn", "kc"} <= {r["want"].get("valid") for r in gc.WGRAD}
    assert {r["want"]["reduce"] for r in gc.WGRAD} == {8, 64}
    for r in gc.FWD + gc.WGRAD:                                # the rows say what the cases are: dtype built, db, valid channels, ragged grid, guards
        c = gc.conv_case(r["mod"], r["name"])
        assert r["dt"] in c.get("dts", ("f32", "bf16")), r["id"]
        if r in gc.WGRAD:
            assert bool(c["db"]) == r["want"]["db"], r["id"]
            assert (r["want"].get("valid") == "kn") == bool(c["kn_valid"]) and (r["want"].get("valid") == "kc") == bool(c.get("kc_valid", 0)), r["id"]
        assert any(s % 16 for s in c["grid"][-1:]) or c["grid"][-2] % 4, (r["id"], "not ragged")


def test_conv_rows_reach_their_route(probe):
    for r in gc.FWD:
        c, w = gc.conv_case(r["mod"], r["name"]), r["want"]
        p = probe(gc.plan_request(r))[0]
        assert p["rc"] == 0, (r["id"], p)
        assert (p["route"], p["geom"]) == (w["route"], w["geom"]), (r["id"], p)
        if w["route"] != "head":
            assert (p["KC"], p["NT"], p["MR"]) == tuple(c["plan"]), (r["id"], p)
        if w["route"] == "kpar":                                # conv_kpar_bf16.hip: 2D with 32-channel chunks takes conv_kpar2d_kernel
            assert (c["dims"] == 2 and p["KC"] == 32) == w["kpar2d"] and p["cpar"] == c["cpar"], (r["id"], p)


def test_weight_gradient_rows_reach_their_family_and_base_z(probe):
    for r in gc.WGRAD:
        c, w = gc.conv_case(r["mod"], r["name"]), r["want"]
        p = probe(gc.plan_request(r))[0]
        assert p["rc"] == 0, (r["id"], p)
        ks = c.get("ks", 3)
        fam = {2: "wp", 1: "brick"}.get(p["brick"]) or {1: "k1", 2: "k2s2"}.get(ks) or ("generic3d" if c["dims"] == 3 else "generic2d")
        assert fam == w["fam"], (r["id"], p)
        assert -(-p["Cb"] // p["bn"]) == w["base_z"], (r["id"], p)      # wgrad_dispatch.inc wg_issue: grid.z = base_z = ceil(Cb / BN)
        assert (8 if p["nsplit"] >= 64 else 64) == w["reduce"], (r["id"], p)      # wgrad_api.hip: 64 slabs and more take wgrad_reduce_kernel<8>


def test_other_rows_reach_their_instance():
    """the launchers' conditions (pointwise.hip, residual.hip), restated, against the sites the cases are listed under"""
    site_of = {cid: e["site"] for e in gc.ENTRIES for cid in e["cases"] if e["site"][1] not in ("conv_c1_reduce_kernel<16>", "act_bwd_sum_kernel", "channel_sum_final_kernel")}
    T = {"bf16": "bf16_t", "f32": "float"}
    km = lambda c: c["src"] in ("ark", "arm")                  # src_has_km: a keep mask or channel multipliers
    for c in gc.OTHER:
        k, kern = c["kind"], site_of[c["id"]][1]
        if k == "c1f":
            W, d3 = c["shape"][3], c["dims"] == 3
            waste = lambda txt: -(-W // (16 * txt)) * 16 * txt - W
            mfma = c["dt"] == "bf16" and c.get("env", {}).get("CHAP_C1_MFMA") != "0"      # (the knob's default is 1)
            want = "conv_c1_mfma_kernel<%s,%d>" % (str(d3).lower(), 5 if waste(5) < waste(4) else 4) if mfma else "conv_c1_fwd_kernel<%s,%s,16>" % (T[c["dt"]], str(d3).lower())
        elif k == "c1b":
            want = "conv_c1_bwd_kernel<%s,%s,16>" % (T[c["dt"]], str(c["dims"] == 3).lower())
        elif k == "pool":
            want = "act_pool2_plain_kernel<T>" if c["shape"][1] <= 1 and not km(c) else "act_pool2_kernel<T>"
        elif k == "up":
            N, D, H, W = c["shape"]
            cell = H >= 2 and W >= 2 and (c["dims"] != 3 or D >= 2)
            want = ("upsample2x_cell_kernel<T,D3>" if km(c) else "upsample2x_cell_plain_kernel<T,false,true,D3>") if cell else "upsample2x_kernel<%s>" % T[c["dt"]]
        elif k == "actbwd":
            want = "act_bwd_kernel<T,APPLY,%s>" % str(not (c["ng"] == 1 and not c["pool"] and c["src"] != "arm")).lower()
        elif k == "p2cl":
            v8 = max(c["C"], c["cpad"]) % 8 == 0 and c["ld"] % 8 == 0 and c["coff"] % 8 == 0
            want = "planar_to_cl%s_kernel<%s>" % ("8" if v8 else "", T[c["dt"]])
        elif k == "chansum":
            want = "channel_sum_kernel<T,%s,true>" % str(km(c)).lower()
        elif k == "chansum_big":                                # src_fits32 false: 64-bit offsets, the form for any source
            assert math.prod(c["shape"]) * max(c["ld"], c["C"]) * (2 if c["dt"] == "bf16" else 4) == 1 << 32 and gc.BIG_COFF(4) + c["C"] <= c["ld"], c["id"]
            want = "channel_sum_kernel<T,true,false>"
        elif k == "resbwd":
            want = "residual_bwd_kernel<%s,%s>" % (T[c["dt"]], str(c["dxin"]).lower())
        else:
            continue
        assert kern == want, (c["id"], kern, want)
    # both dtypes of every kernel written with a template parameter T
    for e in gc.ENTRIES:
        if "<T" in e["site"][1] and e["cases"]:
            assert {gc.OTHER_BY_ID[cid]["dt"] for cid in e["cases"]} == {"bf16", "f32"}, e["site"]
    assert {c["positions"] for c in gc.OTHER if c["kind"] in ("actbwd",)} == {3} and {c["positions"] for c in gc.OTHER if c["kind"] in ("c1b", "chansum", "chansum_big")} == {2}


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and gc.same_bits(a, b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("mod", [sc, kc], ids=["small_conv_cases", "k3_conv_cases"])
def test_lane_0_draws_what_the_case_file_drew_before(mod, monkeypatch):
    """the generator of the case files as it was before `lane`: the same inputs from it and from lane = 0, other inputs from lane = 1"""
    old = lambda c, dt, lane=0: torch.Generator().manual_seed(sum(map(ord, c["name"])) * 2 + mod.DTYPE_ID[dt])
    fwd = [c for c in (mod.FWD_CASES if mod is kc else mod.ALL_FWD) if c["name"] not in getattr(mod, "BIG", ()) and c["name"] != getattr(mod, "SECOND_TRIP", None)]
    for c in fwd[::3] + mod.WGRAD_CASES[::2]:
        make = mod.fwd_inputs if c in fwd else mod.wgrad_inputs
        for dt in c.get("dts", ("f32", "bf16")):
            now, other = make(c, dt), make(c, dt, lane=1)
            with monkeypatch.context() as m:
                m.setattr(mod, "_gen", old)
                before = make(c, dt)
            assert _same(now, before), (c["name"], dt)
            assert not _same(now, other) and _same(other, make(c, dt, 1)), (c["name"], dt)


def test_lanes_of_the_other_families_differ():
    for c in gc.OTHER:
        a, b = gc.other_inputs(c, 0), gc.other_inputs(c, 1)
        assert _same(a, gc.other_inputs(c)) and not _same(a, b), c["id"]
        assert len({str(gc.other_inputs(c, k)) for k in range(5)}) == 5, c["id"]


# ---- the checker's own proof: a merged weight gradient of five lanes with base_z = 2, built from the fp64 references ------------------------------------------------
@pytest.fixture(scope="module")
def five_lanes():
    e = gc.CONV_BY_ID["kc:w2_16_40:bf16"]
    c = gc.conv_case(e["mod"], e["name"])
    res, refs, bounds = [], [], []
    for lane in range(5):
        inp = gc.conv_inputs(e, lane)
        rw = gc.conv_reference(e, inp)
        nan = lambda: torch.full((sc.GUARD,), float("nan"))
        _, ref, bd = gc.wgrad_views(e, rw, inp, None, None, None)
        res.append({"dw": ref["dw"].float(), "db": ref["db"].float(), "dw#guard": nan(), "db#guard": nan()})
        refs.append(ref)
        bounds.append(bd)
    return c["plan"][1], res, refs, bounds


def test_checker_accepts_the_fault_free_lanes(five_lanes):
    bn, res, refs, bounds = five_lanes
    assert bn == 32 and res[0]["dw"].shape[0] == 40                                            # two B tiles: base_z = 2
    assert gc.check_lanes(res, [{k: v.clone() for k, v in l.items()} for l in res], refs, bounds, "fault-free") <= 1.0
    assert gc.check_lanes(res[:2], res[:2], refs[:2], bounds[:2]) <= 1.0


@pytest.mark.parametrize("both", [False, True], ids=["merged_run_only", "single_run_too"])
@pytest.mark.parametrize("fault", gc.FAULTS)
def test_checker_rejects_a_planted_fault(five_lanes, fault, both):
    """in the merged run alone (the bit comparison with the single launches sees it), and in both runs (only the reference, the guards and the
    lane-against-lane comparison are left to see it)"""
    bn, res, refs, bounds = five_lanes
    bad = gc.plant(fault, res, bn)
    assert not all(_same(a, b) for a, b in zip(res, bad))
    with pytest.raises(AssertionError):
        gc.check_lanes(bad if both else res, bad, refs, bounds, fault)


def test_checker_rejects_a_lane_without_a_reference_and_a_single_lane(five_lanes):
    bn, res, refs, bounds = five_lanes
    with pytest.raises(AssertionError):
        gc.check_lanes(res[:1], res[:1], refs[:1], bounds[:1])
    with pytest.raises(AssertionError):
        gc.check_lanes(res[:2], res[:2], [refs[0], {}], [bounds[0], {}])
    exact = [{"m": torch.arange(5, dtype=torch.uint8) + k, "m#guard": torch.full((4,), 0xAB, dtype=torch.uint8)} for k in range(2)]
    ref = [{"m": l["m"].clone()} for l in exact]
    assert gc.check_lanes(exact, exact, ref, [{"m": None}] * 2) == 0.0                         # exact outputs (masks): equality with the reference
    with pytest.raises(AssertionError):
        gc.check_lanes(exact, exact, [ref[1], ref[0]], [{"m": None}] * 2)
    exact[1]["m#guard"][0] = 0
    with pytest.raises(AssertionError):
        gc.check_lanes(exact, exact, ref, [{"m": None}] * 2)
