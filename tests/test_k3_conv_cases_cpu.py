"""The case table of tests/k3_conv_cases.py without a GPU.

First half: the planner probe (tests/plan_probe.py) over the table, one process per (case, dtype) under the case's LIVE knobs -- every case plans what it
names (route, KC, NT, MR, cpar; weight gradients: family, KC, bn, mr, nsplit, and the tile count of the restated wgrad_tile); the restated dispatch
rules turn plan and case into a kernel instance name in the spelling of tests/golden/launch_plan_parent.csv, and EVERY k3 instance name of that file
must be reached by some case (the map is printed; nothing is filtered).  The WLDS argument inside those names comes from the restated launch_one
(small_conv_cases.conv_lds), which tests/test_small_conv_cases_cpu.py pins against every generic conv row of the golden file.

Second half: an fp32 torch emulation of each op passes the very checks the GPU test makes (k3_conv_cases.fwd_check / wgrad_check), and an emulation with
one planted fault fails the check the fault is aimed at."""
import csv
import re

import pytest
import torch

from tests import k3_conv_cases as kc
from tests import small_conv_cases as sc
from tests.plan_probe import KNOBS, probe                  # noqa: F401 (fixture)
from tests.test_launch_plan_cpu import GOLDEN

ONCE = {"CHAP_CONV_KC16_MAXC", "CHAP_CONV_KC16_MAXC2D", "CHAP_CONV_OCC_CAP", "CHAP_CONV_WLDS_KB", "CHAP_WGRAD_WP_BLOCKS", "CHAP_WGRAD_BN16_MAXC"}      # knobs.h


@pytest.fixture(scope="module")
def plans(probe):
    """{(case name, dtype name): plan dict}; kpar cases also under (name, dtype, "kpar0"): the plan with CHAP_CONV_KPAR = 0"""
    out = {}
    for c in kc.FWD_CASES + kc.WGRAD_CASES:
        req = kc.fwd_request if "cin" in c else kc.wgrad_request
        pre = [kc.setenv_line(c)] if c["knobs"] else []
        for dt in c["dts"]:
            out[(c["name"], dt)] = probe(pre + [req(c, dt)])[0]
            if c.get("route") == "kpar":
                out[(c["name"], dt, "kpar0")] = probe(["setenv CHAP_CONV_KPAR=0", req(c, dt)])[0]
    return out


# ---- (a) every case plans what it names, under live knobs only ----------------------------------------------------------------------------------------------
def test_knobs_are_live():
    for c in kc.FWD_CASES + kc.WGRAD_CASES:
        assert set(c["knobs"]) <= set(KNOBS) - ONCE, (c["name"], c["knobs"])


def test_every_forward_case_plans_what_it_names(plans):
    for name, dt in kc.FWD_IDS:
        c, p = kc.BY_NAME[name], plans[(name, dt)]
        assert p["rc"] == 0, (name, dt, p)
        assert (p["route"], p["geom"], p["KC"], p["NT"], p["MR"], p["cpar"]) == (c["route"], c["dims"] - 1) + c["plan"] + (c["cpar"],), (name, dt, p)
        assert p["nchunks"] == kc.k_channels(c) // c["plan"][0] and p["ntiles"] == -(-c["cout"] // 16)
        if c["route"] == "kpar":
            assert plans[(name, dt, "kpar0")]["route"] == "generic" and p["nchunks"] % c["cpar"] == 0


def test_every_weight_gradient_case_plans_what_it_names(plans):
    fam = {0: "slab", 1: "brick", 2: "wp"}
    for name, dt in kc.WGRAD_IDS:
        c, p = kc.BY_NAME[name], plans[(name, dt)]
        assert p["rc"] == 0, (name, dt, p)
        assert (fam[p["brick"]], p["KC"], p["bn"], p["mr"]) == (c["fam"],) + c["plan"], (name, dt, p)
        assert p["taps"] == 3 ** c["dims"] and p["Ca"] == kc.k_channels(c)
        assert p["ntiles"] == kc.wgrad_tiles(c), (name, dt, p, kc.wgrad_tiles(c))
        if c["nsplit"] is not None:
            assert p["nsplit"] == c["nsplit"], (name, dt, p)
        assert 1 <= p["nsplit"] <= p["ntiles"]


# ---- (b) the instance map -----------------------------------------------------------------------------------------------------------------------------------------
K3 = re.compile(r"((?:conv_fwd_kernel<(?:bf16|f32),3,1|wgrad_kernel<(?:bf16|f32),3,1|conv_wp_kernel<|conv_kpar_kernel<|conv_kpar2d_kernel<|wgrad_wp_kernel<)[^>]*>)")


def _golden_k3():
    names = {}
    for r in csv.DictReader(open(GOLDEN)):
        if " k3 s1 " not in r["shape"]:
            continue
        for n in K3.findall(r["launch"]):
            names.setdefault(n, []).append(r["config"] + " " + r["shape"])
    return names


def test_table_reaches_every_k3_instance_of_the_golden_plan(plans):
    gold = _golden_k3()
    count = lambda pre: sum(n.startswith(pre) for n in gold)
    assert (count("conv_fwd_kernel"), count("conv_wp_kernel"), count("conv_kpar_kernel"), count("wgrad_kernel"), count("wgrad_wp_kernel")) == (26, 5, 1, 9, 2)
    assert len(gold) == 43
    reach = {}
    for name, dt in kc.FWD_IDS:
        reach.setdefault(kc.fwd_instance(kc.BY_NAME[name], dt), []).append(name)
    for name, dt in kc.WGRAD_IDS:
        reach.setdefault(kc.wgrad_instance(kc.BY_NAME[name], dt), []).append(name)
    print("k3 instance <- cases (golden layers)")
    for n in sorted(set(gold) | set(reach)):
        print("  %-72s %-70s %s" % (n, ", ".join(reach.get(n, ["-- none --"])), "golden x%d" % len(gold[n]) if n in gold else "not in the golden file"))
    print("instances reached: %d (%d of the golden file's %d)" % (len(reach), len(set(reach) & set(gold)), len(gold)))
    missing = sorted(n for n in gold if n not in reach)
    assert not missing, missing


def test_resident_weights_and_single_source_both_ways():
    """WLDS (resident against staged weights) and ONE (single source), both values per geometry and dtype, in the generic kernel; the pinned cases hold"""
    got = {}
    for name, dt in kc.FWD_IDS:
        c = kc.BY_NAME[name]
        if c["route"] != "generic":
            continue
        wlds, nbytes = kc.case_lds(c, dt)
        assert nbytes <= 160 * 1024, (name, dt, nbytes)
        if c["wlds"] is not None:
            assert c["wlds"][dt] == wlds, (name, dt, wlds, nbytes)
        zw = kc.launched_tile(c, dt)[1]
        g = (c["dims"], zw, dt)
        got.setdefault(g + ("wlds",), set()).add(wlds)
        if c["arr"] != "add":
            got.setdefault(g + ("one",), set()).add(len(c["cin"]) == 1)
    want = [(2, False, "f32"), (2, False, "bf16"), (3, False, "f32"), (3, False, "bf16"), (3, True, "bf16")]
    assert all(got[g + (k,)] == {True, False} for g in want for k in ("wlds", "one")), got


# ---- (c) what the table must hold ------------------------------------------------------------------------------------------------------------------------------
def test_grids_are_ragged_and_small():
    for name, dt in kc.FWD_IDS:
        c = kc.BY_NAME[name]
        D, H, W = kc.spatial(c)
        td, th, tw = kc.pixel_tile(c, dt)
        assert W % tw and H % th and (td == 1 or D % td), (name, c["grid"], (td, th, tw))
        assert c["trip"] or name not in kc.BIG, name
        assert c["grid"] in (kc.G2, kc.G3) or c["why"] or kc.slices(c), name
    for c in kc.WGRAD_CASES:
        D, H, W = kc.spatial(c)
        td, th, tw = kc.wgrad_tile(c)
        assert W % tw and H % th and (td == 1 or D % td), (c["name"], c["grid"])
        assert c["grid"] in (kc.G2, kc.G3) or c["why"] or kc.slices(c), c["name"]


def test_forward_table_holds_what_the_families_need():
    gen = [c for c in kc.FWD_CASES if c["route"] == "generic"]
    # every (KC, NT, MR) of the 2D generic kernel in both types; 3D slabs NT 1 / 2 / 4 in both, bricks NT 1 / 2 with and without add
    assert {c["plan"] for c in gen if c["dims"] == 2 and c["dts"] == kc.BOTH and c["arr"] != "add"} == {(k, n, m) for k in (16, 32) for n in (1, 2, 4) for m in (1, 2, 4)}
    assert {c["plan"][1] for c in gen if c["dims"] == 3 and c["plan"][2] == 1 and c["dts"] == kc.BOTH} == {1, 2, 4}
    assert {(c["plan"][1], c["arr"] == "add") for c in gen if c["dims"] == 3 and c["plan"][2] == 4} == {(n, a) for n in (1, 2) for a in (False, True)}
    # channel-tile tails at NT 2 and 4, a Cout that is a multiple of 4 but not of 16
    tails = {c["plan"][1] for c in gen if -(-c["cout"] // 16) % c["plan"][1]}
    assert tails >= {2, 4} and any(c["cout"] % 16 == 4 for c in gen) and any(c["cout"] % 32 == 16 for c in kc.FWD_CASES if c["route"] == "kpar")
    # sources: every kind per geometry and KC; cat with and without a straddling chunk in the generic and the wave-private kernel; add in 2D and 3D
    seen = {}
    for c in gen:
        for s in c["src"]:
            seen.setdefault((c["dims"], c["plan"][0]), set()).add("masked" if s in ("ark", "arm") else s)
    assert all(seen[k] == {"p", "ar", "masked", "sl"} for k in ((2, 16), (2, 32), (3, 16))), seen
    lanesel = lambda c: c["arr"] == "cat" and c["cin"][0] % c["plan"][0] != 0
    for route in ("generic", "wp"):
        cats = [c for c in kc.FWD_CASES if c["route"] == route and c["arr"] == "cat"]
        assert any(lanesel(c) for c in cats) and (route == "wp" or any(not lanesel(c) for c in cats))
    assert any(c["cin"] == (48, 16) and c["plan"][0] == 32 for c in gen)
    assert {c["dims"] for c in gen if c["arr"] == "add"} == {2, 3}
    assert all(c["src"][1] not in ("ark", "arm") for c in kc.FWD_CASES if c["arr"] == "add") and any(c["src"][0] in ("ark", "arm") for c in gen if c["arr"] == "add")
    assert {c["route"] for c in kc.FWD_CASES if kc.slices(c)} == {"generic", "kpar"}
    # outputs
    assert {c["out"] for c in kc.FWD_CASES} == {"slot", "out2", "planar"} and {c["bias"] for c in gen} == {True, False}
    assert any(c["out"] == "out2" and c["plan"][1] * 16 > c["cout"] // 2 for c in gen)      # the split inside one block's tiles
    # routes: K-parallel in 2D and 3D, 4 and 2 chunks side by side, two rounds
    kp = [c for c in kc.FWD_CASES if c["route"] == "kpar"]
    assert {(c["dims"], c["cpar"]) for c in kp} == {(d, p) for d in (2, 3) for p in (2, 4)}
    assert {c["dims"] for c in kp if kc.k_channels(c) // c["plan"][0] == 2 * c["cpar"]} == {2, 3}
    # a second trip per route and pixel-tile shape
    trips = {(c["route"], kc.pixel_tile(c, c["dts"][-1])) for c in kc.FWD_CASES if c["trip"]}
    assert trips >= {("generic", (1, 4, 16)), ("generic", (1, 8, 16)), ("generic", (1, 16, 16)), ("generic", (4, 4, 16)), ("wp", (1, 4, 16)), ("kpar", (1, 8, 16)),
                     ("kpar", (1, 4, 16))}, trips
    assert any(c["trip"] and c["dims"] == 3 and c["plan"][2] == 1 for c in gen)


def test_weight_gradient_table_holds_what_the_families_need():
    wg = kc.WGRAD_CASES
    fams = {"slab2": [c for c in wg if c["fam"] == "slab" and c["dims"] == 2], "slab3": [c for c in wg if c["fam"] == "slab" and c["dims"] == 3],
            "brick": [c for c in wg if c["fam"] == "brick"], "wp": [c for c in wg if c["fam"] == "wp"]}
    for f, cs in fams.items():
        ns = {c["nsplit"] for c in cs}
        assert ns >= {1, 5, 9, 12}, (f, ns)
        nine = [c for c in cs if c["nsplit"] == 9][0]
        assert kc.wgrad_tiles(nine) == 9 and sum(not s for s in kc.deal_tiles(9, 9)) == 3
        five = [c for c in cs if c["nsplit"] == 5][0]
        assert max(len(s) for s in kc.deal_tiles(kc.wgrad_tiles(five), 5)) >= 3
    assert {(c["dims"], c["fam"]) for c in wg if c["arr"] == "add"} == {(2, "slab"), (3, "slab"), (3, "brick")}
    assert any(c["arr"] == "add" and c["dims"] == 2 and "bf16" in c["dts"] and "f32" in c["dts"] for c in wg)
    lanesel = lambda c: c["arr"] == "cat" and c["ca"][0] % c["plan"][0] != 0
    assert any(lanesel(c) for c in fams["slab2"]) and any(c["arr"] == "cat" and not lanesel(c) for c in fams["slab2"])
    assert any(c["cb"] % c["plan"][1] for c in wg) and any(c["kn_valid"] for c in wg) and any(c["kc_valid"] for c in wg)
    assert {a for c in wg for a in c["A"]} == {"p", "ar", "ark", "arm", "sl"} and {c["db"] for c in wg} == {True, False}
    assert any((c["nsplit"] or 0) >= 64 for c in wg)        # wgrad_reduce_kernel<8>; every other case takes <64>


def test_deal_tiles_is_a_partition():
    for ntiles in (1, 9, 16, 18, 40, 80):
        for nsplit in range(1, ntiles + 1):
            d = kc.deal_tiles(ntiles, nsplit)
            assert len(d) == nsplit and sorted(t for s in d for t in s) == list(range(ntiles)), (ntiles, nsplit)


# ---- the emulated kernels --------------------------------------------------------------------------------------------------------------------------------------------
EMU_FWD = [(n, dt) for n, dt in kc.FWD_IDS if n not in kc.BIG]


@pytest.fixture(scope="module")
def fwd_ref():
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            c = kc.BY_NAME[name]
            inp = kc.fwd_inputs(c, dt)
            cache[(name, dt)] = (c, inp, kc.fwd_reference(c, dt, inp))
        return cache[(name, dt)]
    return get


@pytest.mark.parametrize("name,dt", EMU_FWD)
def test_clean_forward_emulation_passes(name, dt, fwd_ref):
    c, inp, r = fwd_ref(name, dt)
    flats, stats = kc.fwd_emulate(c, dt, inp)
    assert max(kc.fwd_check(c, dt, r, flats, stats)) <= 1.0


FWD_FAULT_CASES = [("edge_replicated", "g2_16_16_n1m1", " out:"), ("edge_replicated", "g3_16_16_n1", " out:"), ("edge_replicated", "wp_16_16", " out:"),
                   ("taps_swapped", "g2_32_32_n2m2", " out:"), ("taps_swapped", "b3_32_32_n2", " out:"), ("taps_swapped", "kp2_64_32", " out:"),
                   ("depth_row_taps_swapped", "g3_32_48_n2", " out:"), ("depth_row_taps_swapped", "b3_32_16_n1", " out:"), ("depth_row_taps_swapped", "kp3_64_64", " out:"),
                   ("stats_ragged_edge", "g2_16_16_n1m2", " stats "), ("stats_ragged_edge", "wp_32_32", " stats "), ("stats_ragged_edge", "g3_16_16_n1", " stats "),
                   ("stats_ragged_edge", "kp2_64_32", " stats "),
                   ("last_row_dropped", "g2_16_4_planar", " out:"), ("last_row_dropped", "g2_16_64_n4m4", " out:"), ("last_row_dropped", "b3_32_16_n1", " out:"),
                   ("tile_tail_stored", "g2_16_48_n2m2", "outside the output slot"), ("tile_tail_stored", "g2_16_100_n4m2", "outside the output slot"),
                   ("tile_tail_stored", "g3_32_48_n2", "outside the output slot"), ("tile_tail_stored", "kp3_cat_32_32_48", "outside the output slot"),
                   ("add_mask_on_second", "g2_add_16_16", " out:"), ("add_mask_on_second", "g2_add_32_32_n2m4", " out:"), ("add_mask_on_second", "g3_add_16_16_n1", " out:"),
                   ("straddle_from_first", "g2_cat_48_16_32_n2m2", " out:"), ("straddle_from_first", "g2_cat_16_16_16_n1m2", " out:"),
                   ("straddle_from_first", "wp_cat_16_16_16", " out:")]


@pytest.mark.parametrize("fault,name,where", FWD_FAULT_CASES)
def test_planted_forward_fault_fails_its_check(fault, name, where, fwd_ref):
    assert fault in kc.FWD_FAULTS
    for dt in kc.BY_NAME[name]["dts"]:
        c, inp, r = fwd_ref(name, dt)
        flats, stats = kc.fwd_emulate(c, dt, inp, fault=fault)
        with pytest.raises(AssertionError) as e:
            kc.fwd_check(c, dt, r, flats, stats)
        assert where in str(e.value), str(e.value)
        if fault == "stats_ragged_edge":                     # ... and only there: the output of that emulation is clean
            assert max(kc.fwd_check(dict(c, stats=False), dt, r, flats, None)) <= 1.0


def test_every_forward_fault_is_planted():
    assert {f for f, _, _ in FWD_FAULT_CASES} == set(kc.FWD_FAULTS)


@pytest.fixture(scope="module")
def wg_ref():
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            c = kc.BY_NAME[name]
            inp = kc.wgrad_inputs(c, dt)
            cache[(name, dt)] = (c, inp, kc.wgrad_reference(c, dt, inp))
        return cache[(name, dt)]
    return get


@pytest.mark.parametrize("name,dt", kc.WGRAD_IDS)
def test_clean_weight_gradient_emulation_passes(name, dt, wg_ref, plans):
    c, inp, rw = wg_ref(name, dt)
    ns = plans[(name, dt)]["nsplit"]
    dw, db = kc.wgrad_emulate(c, dt, inp, nsplit=ns if c["nsplit"] is not None and ns <= 18 else None)
    assert max(kc.wgrad_check(c, dt, rw, inp, dw, db)) <= 1.0
    assert tuple(dw.shape) == (c["kn_valid"] or c["cb"], c["kc_valid"] or kc.k_channels(c), 3 ** c["dims"])


WGRAD_FAULT_CASES = [("tile_twice", "w2_split5", " dW:"), ("tile_twice", "wb_split12", " dW:"), ("tile_twice", "w3_split9_of_9", " dW:"),
                     ("split_left_out", "w2_split12", " dW:"), ("split_left_out", "wp2_split5", " dW:"), ("split_left_out", "wb_split5", " dW:"),
                     ("empty_split_nan", "w2_split9_of_9", " dW:"), ("empty_split_nan", "w3_split9_of_9", " dW:"), ("empty_split_nan", "wb_split9_of_9", " dW:"),
                     ("empty_split_nan", "wp2_split9_of_9", " dW:"),
                     ("edge_replicated", "w2_16_16", " dW:"), ("edge_replicated", "wb_32_16", " dW:"), ("taps_swapped", "w2_32_32", " dW:"), ("taps_swapped", "w3_32_32", " dW:"),
                     ("add_mask_on_second", "w2_add_32_32", " dW:"), ("add_mask_on_second", "wb_add_32_32", " dW:"),
                     ("straddle_from_first", "w2_cat_48_16_32", " dW:"), ("straddle_from_first", "w2_cat_16_16_16", " dW:")]


@pytest.mark.parametrize("fault,name,where", WGRAD_FAULT_CASES)
def test_planted_weight_gradient_fault_fails_its_check(fault, name, where, wg_ref, plans):
    assert fault in kc.WGRAD_FAULTS
    for dt in kc.BY_NAME[name]["dts"]:
        c, inp, rw = wg_ref(name, dt)
        ns = plans[(name, dt)]["nsplit"] if fault in ("tile_twice", "split_left_out", "empty_split_nan") else None
        dw, db = kc.wgrad_emulate(c, dt, inp, fault=fault, nsplit=ns)
        with pytest.raises(AssertionError) as e:
            kc.wgrad_check(c, dt, rw, inp, dw, db)
        assert where in str(e.value), str(e.value)


def test_every_weight_gradient_fault_is_planted():
    assert {f for f, _, _ in WGRAD_FAULT_CASES} == set(kc.WGRAD_FAULTS)


def test_canaries_see_one_changed_element():
    """every output arrangement: an element outside the slot (or in the guard) that no longer holds its NaN bits is reported"""
    for name in ("g2_16_16_n1m1", "g2_out2_32_64_n4m2", "g2_16_4_planar", "g3_16_16_n1"):
        c = kc.BY_NAME[name]
        for i, (lc, lo, n) in enumerate(kc.out_parts(c)):
            flat, view = kc.new_outs(c, "bf16")[i]
            assert sc.split_out(lc, flat)[1]
            flat[-1] = 0.0
            assert not sc.split_out(lc, flat)[1]
            if c["out"] != "planar":
                flat, view = kc.new_outs(c, "bf16")[i]
                view[0, 0, 0, 0, sc.SLOT_COFF + n] = 1.0
                assert not sc.split_out(lc, flat)[1]
