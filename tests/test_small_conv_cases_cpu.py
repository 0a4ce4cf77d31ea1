"""The case table of tests/small_conv_cases.py without a GPU.

First half: the planner probe (tests/plan_probe.py) over the table -- every case plans the instance it names, the table reaches every k1 / k2 s2
instance of the bench-shaped steps (tests/golden/launch_plan_parent.csv), has a tile tail, ragged grids, and resident and staged weights per geometry;
the resident-weights arithmetic of conv_dispatch.inc, restated in the case module, is pinned against the WLDS template argument of every generic conv
row of the golden file.

Second half, in the style of tests/test_kernel_ref_cpu.py: an fp32 torch emulation of each op passes the very checks the GPU test makes
(small_conv_cases.fwd_check / wgrad_check), and an emulation with one planted fault fails the check the fault is aimed at."""
import csv
import math
import re

import pytest
import torch

from tests import small_conv_cases as sc
from tests.plan_probe import probe                         # noqa: F401 (fixture)
from tests.test_launch_plan_cpu import GOLDEN, _conv_request, _instance

DTS = ("f32", "bf16")
GEOMS = {"k1": 3, "d2s": 3, "head": 3}                     # conv_plan.h geom: 3 = 1x1, 4 / 5 = 2D / 3D k2 s2


def _geom(c):
    return GEOMS.get(c["op"], 4 if c["dims"] == 2 else 5)


@pytest.fixture(scope="module")
def plans(probe):
    """{(case name, dtype name): plan dict}"""
    out = {}
    for dt in DTS:
        cases = sc.ALL_FWD + sc.WGRAD_CASES
        reqs = [sc.fwd_request(c, dt) for c in sc.ALL_FWD] + [sc.wgrad_request(c, dt) for c in sc.WGRAD_CASES]
        out.update({(c["name"], dt): p for c, p in zip(cases, probe(reqs))})
    return out


# ---- (a) every case plans exactly what it names ------------------------------------------------------------------------------------------------------------
def test_every_case_plans_the_instance_it_names(plans):
    for dt in DTS:
        for c in sc.ALL_FWD:
            p = plans[(c["name"], dt)]
            assert p["rc"] == 0, (c["name"], dt, p)
            assert (p["route"], p["geom"], p["KC"], p["NT"], p["MR"]) == (c["route"][dt], _geom(c)) + c["plan"], (c["name"], dt, p)
            assert p["cpar"] == 0 and p["ntiles"] == -(-sc.launch_cout(c) // 16)
            if c["chunks"] is not None:
                assert p["nchunks"] == c["chunks"], (c["name"], dt, p)
        for c in sc.WGRAD_CASES:
            p = plans[(c["name"], dt)]
            assert p["rc"] == 0, (c["name"], dt, p)
            assert (p["brick"], p["KC"], p["bn"]) == (0,) + c["plan"][dt] and p["mr"] == 0 and p["nsplit"] > 1, (c["name"], dt, p)
            assert p["taps"] == c["ks"] ** c["dims"]


# ---- (b) the table reaches every k1 / k2 s2 instance the bench-shaped steps launch ---------------------------------------------------------------------------------
def _bench_instances():
    conv, wg = {}, {}
    for r in csv.DictReader(open(GOLDEN)):
        dt = "f32" if r["config"].endswith("fp32") else "bf16"
        i = _instance(r["launch"], "conv_fwd_kernel")      # <T, KS, ST, D3, KC, NT, MR, ADD2, WLDS, ZW, ONE>
        if i and i[0][1] in (1, 2):
            conv.setdefault((dt, i[0][1], bool(i[0][3]), i[0][4], i[0][5], i[0][6]), []).append(r["shape"])
        i = _instance(r["launch"], "wgrad_kernel")         # <T, KS, ST, D3, KC, MR, ADD2, BN, PD, ZW>
        if i and i[0][1] in (1, 2):
            wg.setdefault((dt, i[0][1], bool(i[0][3]), i[0][4], i[0][7]), []).append(r["shape"])
    return conv, wg


def test_table_reaches_every_k1_k2_instance_of_the_bench(plans):
    conv, wg = _bench_instances()
    assert len(conv) >= 20 and len(wg) >= 10
    reach_c, reach_w = {}, {}
    for dt in DTS:
        for c in sc.ALL_FWD:
            if c["route"][dt] == "generic":
                reach_c.setdefault(sc.fwd_instance(c, dt), []).append(c["name"])
        for c in sc.WGRAD_CASES:
            reach_w.setdefault(sc.wgrad_instance(c, dt), []).append(c["name"])
    fmt = lambda k: "%s k%d %s KC%d %s" % (k[0], k[1], "3D" if k[2] else "2D", k[3], "NT%d MR%d" % k[4:] if len(k) == 6 else "bn%d" % k[4])
    print("conv_fwd_kernel instance <- cases (bench layers)")
    for k in sorted(set(conv) | set(reach_c)):
        print("  %-28s %-60s %s" % (fmt(k), ", ".join(reach_c.get(k, ["-- none --"])), "bench x%d" % len(conv[k]) if k in conv else "not in the bench"))
    print("wgrad_kernel instance <- cases (bench layers)")
    for k in sorted(set(wg) | set(reach_w)):
        print("  %-28s %-60s %s" % (fmt(k), ", ".join(reach_w.get(k, ["-- none --"])), "bench x%d" % len(wg[k]) if k in wg else "not in the bench"))
    assert not [k for k in conv if k not in reach_c], [fmt(k) for k in conv if k not in reach_c]
    assert not [k for k in wg if k not in reach_w], [fmt(k) for k in wg if k not in reach_w]
    # the head kernel itself: one bf16 case per class count, both dims
    heads = [c for c in sc.HEAD_CASES]
    assert {c["cout"] for c in heads} >= {1, 2, 3, 5, 8} and {c["dims"] for c in heads} == {2, 3}


# ---- (c) a tile tail per geometry, (d) ragged grids ---------------------------------------------------------------------------------------------------------------
def test_tile_tails_and_ragged_grids():
    tails = {}
    for c in sc.FWD_CASES:
        NT = c["plan"][1]
        if -(-sc.launch_cout(c) // 16) % NT:
            tails.setdefault(_geom(c), []).append(c["name"])
    assert set(tails) == {3, 4, 5}, tails
    for c in sc.ALL_FWD:
        th, tw = sc.conv_tile(c)
        assert c["grid"][-1] % tw and c["grid"][-2] % th, (c["name"], c["grid"], (th, tw))
    for c in sc.WGRAD_CASES:
        th, tw = sc.wgrad_tile(c)
        assert c["grid"][-1] % tw and c["grid"][-2] % th, (c["name"], c["grid"], (th, tw))
    # all but the one second-trip head case stay below 60 000 pixels of the launch's grid
    for c in sc.ALL_FWD + sc.WGRAD_CASES:
        px = c["N"] * math.prod(c["grid"])
        assert (px > 4096 * 256) if c["name"] == sc.SECOND_TRIP else (px < 60000), (c["name"], px)


def test_sources_flags_and_kinds_are_spread_over_the_table():
    fam = lambda c: (_geom(c), c["plan"][0])
    seen = {}
    for c in sc.FWD_CASES:
        for s in c["src"]:
            seen.setdefault(fam(c), set()).add("masked" if s in ("ark", "arm") else s)
    assert set(seen) == {(g, kc) for g in (3, 4, 5) for kc in (16, 32)}
    assert all(v == {"p", "ar", "masked", "sl"} for v in seen.values()), seen
    # per-sample multipliers differ per sample only with N >= 2
    assert all(c["N"] >= 2 for c in sc.ALL_FWD + sc.WGRAD_CASES if "arm" in c.get("src", ()) and c["name"] != "k1_3d_16_16")
    # statistics with a shift per geometry and NT (the depth-to-space launches among the 1x1 ones), bias on and off per geometry
    st = {(_geom(c), c["plan"][1]) for c in sc.FWD_CASES if c["stats"]}
    assert st >= {(g, nt) for g in (3, 4, 5) for nt in (1, 2, 4)}
    assert {c["plan"][1] for c in sc.FWD_CASES if c["stats"] and c["op"] == "d2s"} == {2, 4}
    assert {(_geom(c), c["bias"]) for c in sc.FWD_CASES} == {(g, b) for g in (3, 4, 5) for b in (True, False)}
    kinds = {(c["op"], c["kind"]) for c in sc.FWD_CASES}
    assert kinds >= {("k1", sc.CF), ("k1", sc.CD), ("k2", sc.CF), ("k2", sc.DD), ("d2s", sc.DF), ("d2s", sc.WD)}
    d2s = [c for c in sc.FWD_CASES if c["op"] == "d2s"]
    assert {(c["dims"], c["plan"][1], c["plan"][2]) for c in d2s} >= {(2, 4, 1), (2, 4, 2), (3, 4, 1), (3, 4, 2), (3, 2, 1)} and any(c["cout"] == 48 for c in d2s)
    assert sc.SLOT_COFF > 0 and sc.SLOT_EXTRA > sc.SLOT_COFF
    # weight gradients: lazy A on k1 (multipliers in 3D), lazy B on the transposed conv, bias gradients, the padded head gradient, D > 1 under k1
    wg = sc.WGRAD_CASES
    assert any(c["ks"] == 1 and c["A"] == "ar" for c in wg) and any(c["ks"] == 1 and c["dims"] == 3 and c["A"] == "arm" and c["grid"][0] > 1 for c in wg)
    assert any(c["ks"] == 2 and c["role"] == "deconv" and c["B"] in ("ar", "arm") and c["dims"] == d for c in wg for d in (2, 3))
    assert any(c["kn_valid"] == 2 and c["cb"] == 16 and c["dims"] == 3 and c["ks"] == 1 for c in wg) and sum(c["db"] for c in wg) >= 6
    assert any(c["cb"] % c["plan"]["bf16"][1] for c in wg)                      # Cb not a multiple of the B tile


# ---- (e) resident and staged weights --------------------------------------------------------------------------------------------------------------------------------
def test_resident_weights_restatement_reproduces_the_golden_instances():
    """conv_lds (small_conv_cases.py) against EVERY generic conv row of the golden file, all kernel sizes: the WLDS template argument.  The file's
    `lds=` column cannot be compared: the trace it was read off recorded 0 bytes for every kernel (the kernels' LDS is dynamic; the trace's column is the
    static size), which the last assertion states -- a regenerated golden file with real sizes fails here and is then compared against conv_lds's bytes."""
    rows = 0
    lds_recorded = set()
    for r in csv.DictReader(open(GOLDEN)):
        i = _instance(r["launch"], "conv_fwd_kernel")
        if not i:
            continue
        T, KS, ST, D3, KC, NT, MR, ADD2, WLDS, ZW, ONE = i[0]
        _, ck, _ = _conv_request(r["shape"], T)
        wlds, nbytes = sc.conv_lds(2 if T == sc.BF16 else 4, KS, ST, bool(D3), KC, NT, MR, bool(ZW), ck // KC)
        assert wlds == bool(WLDS), (r["config"], r["shape"], r["launch"], wlds, nbytes)
        assert nbytes <= 160 * 1024
        lds_recorded.add(int(re.search(r"conv_fwd_kernel<[^>]*>: grid=\S+ lds=(\d+)", r["launch"]).group(1)))
        rows += 1
    assert rows >= 100
    assert lds_recorded == {0}


def test_table_holds_resident_and_staged_weights_per_geometry():
    got = {}
    for c in sc.FWD_CASES:
        for dt in DTS:
            wlds, nbytes = sc.case_lds(c, dt)
            if c["wlds"] is not None:
                assert c["wlds"][dt] == wlds, (c["name"], dt, wlds, nbytes)
            got.setdefault((_geom(c), dt), set()).add(wlds)
    assert all(got[(g, dt)] == {True, False} for g in (3, 4, 5) for dt in DTS), got


# ---- the emulated kernels --------------------------------------------------------------------------------------------------------------------------------------------
EMU_FWD = [c["name"] for c in sc.ALL_FWD if c["name"] != sc.SECOND_TRIP]            # (the one large case: the GPU file's alone)


@pytest.fixture(scope="module")
def fwd_ref():
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            c = sc.BY_NAME[name]
            inp = sc.fwd_inputs(c, dt)
            cache[(name, dt)] = (c, inp, sc.fwd_reference(c, dt, inp))
        return cache[(name, dt)]
    return get


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", EMU_FWD)
def test_clean_forward_emulation_passes(name, dt, fwd_ref):
    c, inp, r = fwd_ref(name, dt)
    flat, stats = sc.fwd_emulate(c, dt, inp)
    worst = sc.fwd_check(c, dt, r, flat, stats)
    assert max(worst) <= 1.0


# fault -> (case, the check it must fail at)
FWD_FAULT_CASES = [("d2s_xy_swapped", "d2s_128_64_mr1", " out:"), ("d2s_xy_swapped", "d2s_3d_256_128", " out:"),
                   ("bias_not_folded", "d2s_128_64_mr1", " out:"), ("bias_not_folded", "d2s_3d_256_128", " out:"),
                   ("tile_tail_stored", "k2_64_96", "outside the output slot"), ("tile_tail_stored", "k2_3d_16_48", "outside the output slot"),
                   ("tile_tail_stored", "k1_16_48", "outside the output slot"),
                   ("stats_ragged_columns", "k2_16_32", " stats "), ("stats_ragged_columns", "d2s_3d_256_128", " stats "), ("stats_ragged_columns", "k2_3d_16_16", " stats "),
                   ("last_column_dropped", "k1_64_16", " out:"), ("last_column_dropped", "k2_3d_32_32", " out:"), ("last_column_dropped", "d2s_128_64_mr1", " out:"),
                   ("k2_taps_transposed", "k2_32_32", " out:"), ("k2_taps_transposed", "k2_3d_16_32", " out:"),
                   ("chan_mul_of_sample0", "k2_3d_32_32", " out:"), ("chan_mul_of_sample0", "d2s_3d_256_128", " out:"), ("chan_mul_of_sample0", "head_c3_straddle", " out:")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fault,name,where", FWD_FAULT_CASES)
def test_planted_forward_fault_fails_its_check(fault, name, where, dt, fwd_ref):
    assert fault in sc.FWD_FAULTS
    c, inp, r = fwd_ref(name, dt)
    flat, stats = sc.fwd_emulate(c, dt, inp, fault=fault)
    with pytest.raises(AssertionError) as e:
        sc.fwd_check(c, dt, r, flat, stats)
    assert where in str(e.value), str(e.value)
    if fault == "stats_ragged_columns":                    # ... and only there: the output of that emulation is clean
        c2 = dict(c, stats=False)
        assert max(sc.fwd_check(c2, dt, r, flat, None)) <= 1.0


@pytest.fixture(scope="module")
def wg_ref():
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            c = sc.BY_NAME[name]
            inp = sc.wgrad_inputs(c, dt)
            cache[(name, dt)] = (c, inp, sc.wgrad_reference(c, dt, inp))
        return cache[(name, dt)]
    return get


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [c["name"] for c in sc.WGRAD_CASES])
def test_clean_weight_gradient_emulation_passes(name, dt, wg_ref):
    c, inp, rw = wg_ref(name, dt)
    dw, db = sc.wgrad_emulate(c, dt, inp)
    assert max(sc.wgrad_check(c, dt, rw, inp, dw, db)) <= 1.0
    if c["kn_valid"]:
        assert tuple(dw.shape) == (c["kn_valid"], c["ca"], 1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fault,name,where", [("lazy_b_raw", "wg_k2_16_32", " dW:"), ("lazy_b_raw", "wg_k2_3d_32_16", " dW:"),
                                              ("db_one_split", "wg_k2_32_16", " db:"), ("db_one_split", "wg_k1_3d_16_16", " db:"),
                                              ("db_of_rounded_b", "wg_k2_16_32", " db:"), ("db_of_rounded_b", "wg_k2_3d_32_16", " db:"),
                                              ("chan_mul_of_sample0", "wg_k1_3d_16_16_n2", " dW:"), ("chan_mul_of_sample0", "wg_k2_3d_32_16", " dW:")])
def test_planted_weight_gradient_fault_fails_its_check(fault, name, where, dt, wg_ref):
    assert fault in sc.WGRAD_FAULTS
    c, inp, rw = wg_ref(name, dt)
    dw, db = sc.wgrad_emulate(c, dt, inp, fault=fault)
    if fault == "db_of_rounded_b" and dt == "f32":         # an fp32 operand IS the fp32 value: nothing to tell apart
        assert max(sc.wgrad_check(c, dt, rw, inp, dw, db)) <= 1.0
        return
    with pytest.raises(AssertionError) as e:
        sc.wgrad_check(c, dt, rw, inp, dw, db)
    assert where in str(e.value), str(e.value)


def test_canaries_see_one_changed_element():
    """split_out: any element outside the slot that no longer holds its NaN bits -- another NaN payload included -- is reported"""
    for name in ("k1_64_16", "head_c2"):
        c = sc.BY_NAME[name]
        flat, view = sc.new_out(c, torch.bfloat16)
        assert sc.split_out(c, flat)[1]
        flat[-1] = 0.0
        assert not sc.split_out(c, flat)[1]
        flat, view = sc.new_out(c, torch.bfloat16)
        if name != "head_c2":
            view[0, 0, 0, 0, 0] = 1.0
            assert not sc.split_out(c, flat)[1]
