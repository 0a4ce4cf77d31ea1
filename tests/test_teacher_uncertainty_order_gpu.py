"""Launch order with the uncertainty-aware teacher consistency on: one eager and one captured 2D step with teacher, guard, monitor and T = 2
noisy teacher passes, recorded with the rich recorder of tests/issue_trace.py and run through the order checker of tests/launch_order.py.
The access modes and byte rules of chap_teacher_uncertainty and chap_teacher_consistency_masked are supplied at run time, as
tests/test_teacher_consistency_order_gpu.py supplies its entry's: tests/launch_access.py's tables are extended inside a fixture that restores
them.  Expectation: no finding; both teacher passes, their noise launches and the two new launches are on pass B's stream."""
import ctypes

import pytest
import torch

from chap_amd import _lib as L
from tests import issue_trace, launch_access, launch_order

UNC, MASKED = "chap_teacher_uncertainty", "chap_teacher_consistency_masked"
MODES = {UNC: dict(teacher="R", mask="W", entropy="W", count="W", ws="RW", threshold_dev="R"),
         MASKED: dict(logits="R", teacher="R", mask="R", count="R", dlogits="RW", loss="W", ws="RW", gscale_dev="R")}
ARGS = dict(teacher_consistency=0.7, teacher_noise=0.1, teacher_uncertainty=2)
TU_CASES = {"2d_all_tu_eager": dict(net="2d", mode="eager", teacher=True, guard=True, monitor=True, args=ARGS),
            "2d_all_tu_captured": dict(net="2d", mode="captured", teacher=True, guard=True, monitor=True, args=ARGS)}


def rule_unc(p):
    """Upper bounds from include/chap_hip_uncertainty.h: the first T passes' tensors N C P floats, mask N P bytes, entropy N P floats, ws
    [1 + CHAP_LOSS_SLOTS] int64, count 8 bytes, the device threshold 4."""
    out = {"mask": launch_access.span(p.mask, p.N * p.P), "entropy": launch_access.span(p.entropy or 0, p.N * p.P * 4), "count": launch_access.span(p.count, 8),
           "ws": launch_access.span(p.ws, (1 + L.LOSS_SLOTS) * 8), "threshold_dev": launch_access.span(p.threshold_dev or 0, 4)}
    for k in range(L.UNCERTAINTY_MAX_T):
        for h in range(2):
            out["teacher[%d][%d]" % (k, h)] = launch_access.span((p.teacher[k][h] or 0) if k < p.T else 0, p.N * p.C * p.P * 4)
    return out


def rule_masked(p):
    tensor = p.N * p.C * p.P * 4
    out = {"loss": launch_access.span(p.loss, 4), "gscale_dev": launch_access.span(p.gscale_dev or 0, 4), "ws": launch_access.span(p.ws, (1 + L.LOSS_SLOTS) * 2 * 4),
           "mask": launch_access.span(p.mask, p.N * p.P), "count": launch_access.span(p.count, 8)}
    for h in range(2):
        for k in ("logits", "teacher", "dlogits"):
            out["%s[%d]" % (k, h)] = launch_access.span(getattr(p, k)[h] or 0, tensor)
    return out


@pytest.fixture
def uncertainty_access():
    saved_modes, saved_rules, saved_struct_of, saved_cases = dict(launch_access.MODES), dict(launch_access.RULES), launch_access.struct_of, dict(issue_trace.OPT_CASES)
    launch_access.MODES.update(MODES)
    launch_access.RULES.update({UNC: rule_unc, MASKED: rule_masked})
    launch_access.struct_of = lambda name: L._UNCERTAINTY_SIGS[name] if name in L._UNCERTAINTY_SIGS else saved_struct_of(name)
    issue_trace.OPT_CASES.update(TU_CASES)
    try:
        yield
    finally:
        launch_access.struct_of = saved_struct_of
        for table, saved in ((launch_access.MODES, saved_modes), (launch_access.RULES, saved_rules), (issue_trace.OPT_CASES, saved_cases)):
            table.clear()
            table.update(saved)


def test_modes_cover_the_structs_and_the_byte_rules_by_hand(uncertainty_access):
    """Every pointer field of both structs has a mode and every mode names a field, and one hand-worked case of each rule: N = 4, C = 3, P = 323
    -> tensors of 15 504 bytes, mask 1 292, entropy 5 168, the int64 workspace 513 * 8 = 4 104, the fp32 one 513 * 2 * 4 = 4 104."""
    for name in (UNC, MASKED):
        assert sorted(launch_access.pointer_paths(launch_access.struct_of(name))) == sorted(MODES[name])
    p = L.TeacherUncertaintyParams()
    for k in range(2):                                                  # the passes behind T stay NULL, as ops.teacher_uncertainty leaves them: no access
        p.teacher[k][0], p.teacher[k][1] = 0x100000 * (2 * k + 1), 0x100000 * (2 * k + 2)
    p.mask, p.count, p.ws, p.threshold_dev, p.T, p.N, p.C, p.P = 0x10000, 0x20000, 0x30000, 0x40000, 2, 4, 3, 323
    acc = {path: (mode, addr, ext) for path, mode, addr, ext in launch_access.accesses(UNC, p)}
    assert sorted(acc) == ["count", "mask", "teacher[0][0]", "teacher[0][1]", "teacher[1][0]", "teacher[1][1]", "threshold_dev", "ws"]       # the NULL entropy is no access
    assert acc["teacher[1][1]"] == ("R", 0x400000, (0x400000, 0, 15504, 1)) and acc["mask"] == ("W", 0x10000, (0x10000, 0, 1292, 1))
    assert acc["ws"] == ("RW", 0x30000, (0x30000, 0, 4104, 1)) and acc["count"] == ("W", 0x20000, (0x20000, 0, 8, 1))
    p.entropy = 0x50000
    assert dict((a[0], a[3]) for a in launch_access.accesses(UNC, p))["entropy"] == (0x50000, 0, 5168, 1)
    q = L.TeacherConsistencyMaskedParams()
    q.logits[0], q.logits[1], q.teacher[0], q.teacher[1], q.dlogits[0], q.dlogits[1] = 0x10000, 0x20000, 0x30000, 0x40000, 0, 0x60000
    q.loss, q.ws, q.gscale_dev, q.mask, q.count, q.N, q.C, q.P = 0x70000, 0x80000, 0x90000, 0xa0000, 0xb0000, 4, 3, 323
    acc = {path: (mode, addr, ext) for path, mode, addr, ext in launch_access.accesses(MASKED, q)}
    assert sorted(acc) == ["count", "dlogits[1]", "gscale_dev", "logits[0]", "logits[1]", "loss", "mask", "teacher[0]", "teacher[1]", "ws"]
    assert acc["dlogits[1]"] == ("RW", 0x60000, (0x60000, 0, 15504, 1)) and acc["mask"] == ("R", 0xa0000, (0xa0000, 0, 1292, 1))
    assert acc["count"] == ("R", 0xb0000, (0xb0000, 0, 8, 1)) and acc["ws"] == ("RW", 0x80000, (0x80000, 0, 4104, 1))
    assert ctypes.sizeof(L.TeacherUncertaintyParams) == 128 + 5 * 8 + 5 * 4 + 4 and ctypes.sizeof(L.TeacherConsistencyMaskedParams) == 112


def test_the_fixture_restores_the_tables():
    for name in (UNC, MASKED):
        assert name not in launch_access.MODES and name not in launch_access.RULES
        with pytest.raises(KeyError):
            launch_access.struct_of(name)
    assert not set(TU_CASES) & set(issue_trace.OPT_CASES)


def record(name):
    """issue_trace.record_case(rich=True) with the teacher's pack table known to the recorder as well."""
    case = issue_trace.OPT_CASES[name]
    step, inp, inj = issue_trace._case_step(name)
    only = case["mode"] == "captured"
    rec = issue_trace.RichRecorder(only, issue_trace._Allocations(False), pack_entries=issue_trace._pack_entries_of(step.model, step.teacher))
    with rec.recording():
        if only:
            step.capture(inp["vol"], inp["lab"], warmup=1, inject=inj)
        else:
            step.step(inp["vol"], inp["lab"], box_yx=inp["box"], inject=inj)
    torch.cuda.synchronize()
    return rec.text(), rec.rich_text()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TU_CASES))
def test_every_conflicting_pair_is_ordered_with_the_mask_on(uncertainty_access, case):
    plain, rich = record(case)
    an = launch_order.Analysis(rich)
    found, c = an.findings(), an.counts()
    print("%s: %d launches, %d torch ops, %d streams, %d conflicting pairs all ordered but %d" % (case, c["launches"], c["torch_ops"], c["streams"], c["ordered_conflicts"], len(found)))
    launches = [ln for ln in rich.splitlines() if ln.startswith("L ")]
    bare = [ln for ln in launches if not ln.partition(" | ")[2].strip()]
    assert bare == [], "launches without any access would pass as conflict free: %s" % bare[:5]
    lines = plain.splitlines()
    L_ = [(i, ln.split()) for i, ln in enumerate(lines) if ln.startswith("L ")]
    unc, msk = [(i, w) for i, w in L_ if w[1] == UNC], [(i, w) for i, w in L_ if w[1] == MASKED]
    assert len(unc) == 1 and len(msk) == 1 and c["launches"] == len(L_) and not [w for i, w in L_ if w[1] == "chap_teacher_consistency"]
    # pass B's stream: the one its batched loss backward runs on; uncertainty, then the masked term, behind that backward launch on the same stream
    bwd = [(i, w) for i, w in L_ if w[1] == "chap_mix_loss_multi_bwd"]
    assert len(bwd) == 1 and bwd[0][0] < unc[0][0] < msk[0][0] and bwd[0][1][2] == unc[0][1][2] == msk[0][1][2]
    side = msk[0][1][2]
    # two teacher passes between pass B's forward and the losses: two noise draws and two perturb launches on pass B's stream
    fwd = [(i, w) for i, w in L_ if w[1] == "chap_mix_loss_multi_fwd"]
    rand = [(i, w) for i, w in L_ if w[1] == "chap_rand_uniform" and w[2] == side and i < fwd[0][0]]
    assert len(fwd) == 1 and len(rand) == 2
    for i, w in rand:
        nxt = [v for j, v in L_ if j > i][0]
        assert nxt[1] == "chap_perturb" and nxt[2] == side
    if case.endswith("captured"):
        assert {w[2] for i, w in L_ if rand[0][0] <= i < fwd[0][0]} == {side}            # captured: decoders grouped, nothing leaves pass B's stream
    assert found == [], "%d unordered conflicts, the first:\n%s" % (len(found), "\n".join(f["text"] for f in found[:10]))
