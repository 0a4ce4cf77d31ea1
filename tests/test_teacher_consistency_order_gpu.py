"""Launch order with the mean teacher's consistency term on: one eager and one captured 2D step with teacher, guard, monitor and the term
attached, recorded with the rich recorder of tests/issue_trace.py and run through the order checker of tests/launch_order.py.  The access
modes and the byte rule of chap_teacher_consistency are supplied at run time -- tests/launch_access.py's tables are extended inside a
fixture that restores them; the file itself is not edited -- and the recorder is given the teacher's pack table next to the student's, so
that the teacher's pack launch declares what it writes.  Expectation: no finding; the teacher's pass, its noise launches and the new launch
are on pass B's stream, and both models are packed before the first stream fork."""
import ctypes

import pytest
import torch

from chap_amd import _lib as L
from tests import issue_trace, launch_access, launch_order

NAME = "chap_teacher_consistency"
MODES = dict(logits="R", teacher="R", dlogits="RW", loss="W", ws="RW", gscale_dev="R")          # ws: per-block rows written, read by the finalize kernel, row 0 written
ARGS = dict(teacher_consistency=0.7, teacher_noise=0.1)
TC_CASES = {"2d_all_tc_eager": dict(net="2d", mode="eager", teacher=True, guard=True, monitor=True, args=ARGS),
            "2d_all_tc_captured": dict(net="2d", mode="captured", teacher=True, guard=True, monitor=True, args=ARGS)}


def rule(p):
    """Upper bounds from include/chap_hip_teacher.h: every tensor N C P floats, ws [1 + CHAP_LOSS_SLOTS][2] floats, loss and the device scalar one."""
    tensor = p.N * p.C * p.P * 4
    out = {"loss": launch_access.span(p.loss, 4), "gscale_dev": launch_access.span(p.gscale_dev, 4), "ws": launch_access.span(p.ws, (1 + L.LOSS_SLOTS) * 2 * 4)}
    for h in range(2):
        for k in ("logits", "teacher", "dlogits"):
            out["%s[%d]" % (k, h)] = launch_access.span(getattr(p, k)[h] or 0, tensor)
    return out


@pytest.fixture
def teacher_access():
    saved_modes, saved_rules, saved_struct_of, saved_cases = dict(launch_access.MODES), dict(launch_access.RULES), launch_access.struct_of, dict(issue_trace.OPT_CASES)
    launch_access.MODES[NAME], launch_access.RULES[NAME] = MODES, rule
    launch_access.struct_of = lambda name: L._TEACHER_SIGS[name] if name in L._TEACHER_SIGS else saved_struct_of(name)
    issue_trace.OPT_CASES.update(TC_CASES)
    try:
        yield
    finally:
        launch_access.struct_of = saved_struct_of
        for table, saved in ((launch_access.MODES, saved_modes), (launch_access.RULES, saved_rules), (issue_trace.OPT_CASES, saved_cases)):
            table.clear()
            table.update(saved)


def test_modes_cover_the_struct_and_the_byte_rule_by_hand(teacher_access):
    """Every pointer field of the struct has a mode and every mode names a field (what tests/test_launch_access_cpu.py asks of the tables it
    walks), and one hand-worked case of the rule: N = 4, C = 3, P = 323 -> tensors of 4 * 3 * 323 * 4 = 15 504 bytes, ws 513 * 2 * 4 = 4 104."""
    st = launch_access.struct_of(NAME)
    assert st is L.TeacherConsistencyParams and sorted(launch_access.pointer_paths(st)) == sorted(MODES)
    p = st()
    p.logits[0], p.logits[1], p.teacher[0], p.teacher[1], p.dlogits[0], p.dlogits[1] = 0x10000, 0x20000, 0x30000, 0x40000, 0, 0x60000
    p.loss, p.ws, p.gscale_dev, p.N, p.C, p.P = 0x70000, 0x80000, 0x90000, 4, 3, 323
    acc = {path: (mode, addr, ext) for path, mode, addr, ext in launch_access.accesses(NAME, p)}
    assert sorted(acc) == ["dlogits[1]", "gscale_dev", "logits[0]", "logits[1]", "loss", "teacher[0]", "teacher[1]", "ws"]          # the NULL dlogits[0] is no access
    assert acc["logits[1]"] == ("R", 0x20000, (0x20000, 0, 15504, 1)) and acc["teacher[0]"] == ("R", 0x30000, (0x30000, 0, 15504, 1))
    assert acc["dlogits[1]"] == ("RW", 0x60000, (0x60000, 0, 15504, 1))
    assert acc["ws"] == ("RW", 0x80000, (0x80000, 0, 4104, 1)) and acc["loss"] == ("W", 0x70000, (0x70000, 0, 4, 1)) and acc["gscale_dev"][2] == (0x90000, 0, 4, 1)
    assert ctypes.sizeof(st) == 96


def test_the_fixture_restores_the_tables():
    assert NAME not in launch_access.MODES and NAME not in launch_access.RULES and not set(TC_CASES) & set(issue_trace.OPT_CASES)
    with pytest.raises(KeyError):
        launch_access.struct_of(NAME)


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
@pytest.mark.parametrize("case", list(TC_CASES))
def test_every_conflicting_pair_is_ordered_with_the_term_on(teacher_access, case):
    plain, rich = record(case)
    an = launch_order.Analysis(rich)
    found, c = an.findings(), an.counts()
    print("%s: %d launches, %d torch ops, %d streams, %d conflicting pairs all ordered but %d" % (case, c["launches"], c["torch_ops"], c["streams"], c["ordered_conflicts"], len(found)))
    launches = [ln for ln in rich.splitlines() if ln.startswith("L ")]
    bare = [ln for ln in launches if not ln.partition(" | ")[2].strip()]
    assert bare == [], "launches without any access would pass as conflict free: %s" % bare[:5]
    lines = plain.splitlines()
    L_ = [(i, ln.split()) for i, ln in enumerate(lines) if ln.startswith("L ")]
    tc = [(i, w) for i, w in L_ if w[1] == NAME]
    assert len(tc) == 1 and c["launches"] == len(L_)
    # pass B's stream: the one its batched loss backward runs on; the term's launch is behind that backward launch, on the same stream
    bwd = [(i, w) for i, w in L_ if w[1] == "chap_mix_loss_multi_bwd"]
    assert len(bwd) == 1 and bwd[0][0] < tc[0][0] and bwd[0][1][2] == tc[0][1][2]
    side = tc[0][1][2]
    # the teacher's pass between pass B's forward and the term: the noise launches and the network's launches of that stretch, all on pass B's
    # stream or -- eager only: the executor's own fork of its second decoder -- on a stream that stretch forks from it and joins back
    fwd = [(i, w) for i, w in L_ if w[1] == "chap_mix_loss_multi_fwd"]
    rand = [(i, w) for i, w in L_ if w[1] == "chap_rand_uniform" and w[2] == side]
    assert len(fwd) == 1 and len(rand) == 1 and rand[0][0] < fwd[0][0]
    stretch = [w for i, w in L_ if rand[0][0] <= i < fwd[0][0]]
    assert stretch[1][1] == "chap_perturb" and stretch[1][2] == side and len(stretch) > 20
    others = {w[2] for w in stretch} - {side}
    if case.endswith("captured"):
        assert others == set()                                          # captured: decoders grouped, nothing leaves pass B's stream
    else:
        forked = {ln.split()[1] for ln in lines[rand[0][0]:fwd[0][0]] if ln.startswith("WS ") and ln.split()[2] == side}
        joined = {ln.split()[2] for ln in lines[rand[0][0]:fwd[0][0]] if ln.startswith("WS ") and ln.split()[1] == side}
        assert others <= forked and others <= joined
    # both models' packed weights are rewritten back to back on the iteration's own stream, in front of every pass: no wait between the two
    # pack launches, no other launch before them (the streams of the passes fork behind them)
    packs = [(i, w) for i, w in L_ if w[1] == "chap_pack_multi"]
    assert len(packs) == 2 and packs[0][1][2] == packs[1][1][2] != side
    assert not [ln for ln in lines[packs[0][0]:packs[1][0]] if ln.startswith(("WS ", "WE "))]
    assert [i for i, w in L_ if i < packs[1][0]] == [packs[0][0]]
    assert found == [], "%d unordered conflicts, the first:\n%s" % (len(found), "\n".join(f["text"] for f in found[:10]))
