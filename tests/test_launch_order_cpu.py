"""The happens-before check of tests/launch_order.py on small hand-written records, one per rule, and on the committed rich record of the
captured 2D step (tests/golden/launch_order_2d_captured.txt.gz, this project's own output: `python -m tests.issue_trace --rich DIR
2d_captured`): every stream wait of that record is taken out in turn -- on the record, never on the device -- and the check has to notice
the joins the iteration depends on.  The same on the records with the opt-in features (launch_order_2d_all_captured.txt.gz: teacher, guard
and monitor attached; launch_order_2d_all_interval.txt.gz: three replays with a validation interval and both readers between them,
`python -m tests.issue_trace --rich DIR 2d_all_captured 2d_all_interval`): the joins the opt-in launches hang on, and the readers' two waits."""
import gzip
import os

import pytest

from chap_amd import _lib as L
from tests import launch_access, launch_order
from tests.launch_order import analyze


def record(*lines):
    return "\n".join(lines) + "\n"


def races(text):
    return [f for f in analyze(text) if f["kind"] == "race"]


WRITE_A = "L chap_perturb s0 | out:W:A0+0:1024"
READ_A = "L chap_l2_normalize s1 | in_:R:A0+512:64 out:W:A1+0:64"


# ---------------------------------------------------------------------------------------------------------------- one rule each
def test_program_order_on_one_stream():
    assert analyze(record(WRITE_A, "L chap_l2_normalize s0 | in_:R:A0+512:64 out:W:A0+0:64")) == []


def test_a_missing_join_is_flagged_and_the_join_clears_it():
    found = races(record(WRITE_A, READ_A))
    assert len(found) == 1 and found[0]["lines"] == (1, 2)
    assert "chap_perturb on s0" in found[0]["text"] and "chap_l2_normalize on s1" in found[0]["text"]
    assert found[0]["fields"] == [("out:W", "in_:R")]
    assert analyze(record(WRITE_A, "WS s1 s0", READ_A)) == []
    assert len(races(record(WRITE_A, "WS s0 s1", READ_A))) == 1           # the wait the wrong way round orders nothing
    assert len(races(record("WS s1 s0", WRITE_A, READ_A))) == 1           # a wait covers what was issued BEFORE it only


def test_joins_are_transitive():
    assert analyze(record(WRITE_A, "WS s2 s0", "L chap_perturb s2 | out:W:A5+0:4", "WS s1 s2", READ_A)) == []


def test_event_edges_go_through_the_latest_record():
    assert analyze(record(WRITE_A, "ER e0 s0", "WE s1 e0", READ_A)) == []
    assert len(races(record("ER e0 s0", WRITE_A, "WE s1 e0", READ_A))) == 1            # recorded before the write: does not cover it
    assert analyze(record("ER e0 s0", WRITE_A, "ER e0 s0", "WE s1 e0", READ_A)) == []  # ... the second record does
    assert len(races(record(WRITE_A, "WE s1 e0", READ_A))) == 1                        # an event never recorded orders nothing


def test_host_waits_order_everything_the_host_issues_afterwards():
    assert analyze(record(WRITE_A, "HS", READ_A)) == []
    assert analyze(record(WRITE_A, "SS s0", READ_A)) == []
    assert len(races(record(WRITE_A, "SS s1", READ_A))) == 1                           # the host waited for the wrong stream
    assert analyze(record(WRITE_A, "ER e0 s0", "ES e0", READ_A)) == []
    assert len(races(record("ER e0 s0", WRITE_A, "ES e0", READ_A))) == 1


def test_the_default_stream_gives_no_implicit_edge():
    assert len(races(record("L chap_perturb s0 | out:W:A0+0:64", "T copy_ s1 | a1:R:A0+0:64 a0:W:A1+0:64"))) == 1


def test_torch_ops_and_replays_are_launches_like_any_other():
    staged = ["T copy_ s1 | a0:W:A3+0:4096", "ER e0 s1", "WE s0 e0", "T copy_ s0 | a1:R:A3+0:4096 a0:W:A0+0:4096", "ER e1 s0",
              "GR s0 | r0:R:A0+0:4096 w1:W:A9+0:64"]
    assert analyze(record(*staged, "WE s1 e1", "T copy_ s1 | a0:W:A3+0:4096")) == []
    found = races(record(*staged, "T copy_ s1 | a0:W:A3+0:4096"))                     # the next batch overwrites the staged one while it is being taken
    assert [f["lines"] for f in found] == [(4, 7)]
    found = races(record(*staged, "T copy_ s1 | a0:W:A0+0:4096"))                     # ... or lands in the static buffer under the running replay
    assert sorted(f["lines"] for f in found) == [(4, 7), (6, 7)]


def test_two_lanes_writing_one_buffer_are_flagged():
    region = ["GB s0 g0", "L chap_conv_fwd s0 g0 l0 | out:W:A0+0:256", "L chap_bn_finalize s0 g0 l0 | scale:W:A1+0:64", "GN g0 l1",
              "L chap_conv_fwd s0 g0 l1 | out:W:A0+128:256", "GE g0"]
    found = races(record(*region))
    assert [f["lines"] for f in found] == [(2, 5)] and "g0 l0" in found[0]["text"] and "g0 l1" in found[0]["text"]
    ok = [ln.replace("A0+128", "A0+256") for ln in region]
    assert analyze(record(*ok)) == []
    # within a lane the order is kept; the region as a whole sits in its stream's order: before what follows it, after what precedes it
    assert analyze(record("L chap_perturb s0 | out:W:A0+0:64", *ok, "L chap_perturb s0 | x:R:A0+0:512 out:W:A1+0:64")) == []
    assert analyze(record("GB s0 g0", "L chap_conv_fwd s0 g0 l0 | out:W:A0+0:256", "L chap_bn_finalize s0 g0 l0 | stats:R:A0+0:256 scale:W:A1+0:64", "GE g0")) == []


def test_a_region_issues_nothing_before_its_end():
    # the wait sits inside the region: s1 then waits for what s0 was handed BEFORE the region only, the region's launches come at GE
    text = record("GB s0 g0", "L chap_conv_fwd s0 g0 l0 | out:W:A0+0:1024", "WS s1 s0", "GE g0", READ_A)
    assert [f["lines"] for f in races(text)] == [(2, 5)]
    assert analyze(record("GB s0 g0", "L chap_conv_fwd s0 g0 l0 | out:W:A0+0:1024", "GE g0", "WS s1 s0", READ_A)) == []


def test_a_free_followed_by_reuse_on_another_stream_with_no_join_is_flagged():
    # s1 reads a temporary that was allocated on s0; Python drops it, the allocator hands the same bytes out again on s0 (same label and
    # offset in the record), and s0 overwrites them while nothing says that s1's reader has run
    reuse = ["L chap_perturb s0 | out:W:A2+4096:512", "WS s1 s0", "L chap_l2_normalize s1 | in_:R:A2+4096:512 out:W:A3+0:512",
             "L chap_rand_uniform s0 | out:W:A2+4096:256"]
    found = races(record(*reuse))
    assert [f["lines"] for f in found] == [(3, 4)] and found[0]["fields"] == [("in_:R", "out:W")]
    assert analyze(record(*reuse[:3], "WS s0 s1", reuse[3])) == []


def test_disjoint_channel_slices_are_clean_and_overlapping_ones_flagged():
    lo = "L chap_upsample2x s0 | out:W:A0+0:64x100/128"           # channels [0, 16) of fp32 pixels of 32
    hi = "L chap_conv_fwd s1 | out:W:A0+64:64x100/128"            # channels [16, 32): inside the other's first-to-last range, yet disjoint
    assert analyze(record(lo, hi)) == []
    found = races(record(lo, hi.replace("A0+64:", "A0+60:")))     # one channel too early
    assert len(found) == 1
    assert len(races(record(lo, "L chap_conv_fwd s1 | out:W:A0+12736:64x100/128"))) == 0          # behind the last row
    assert len(races(record(lo, "L chap_conv_fwd s1 | out:W:A0+12672:4"))) == 1                   # the last row's first channel


def test_read_read_is_clean_and_accumulations_are_writes():
    assert analyze(record("L chap_conv_fwd s0 | wpacked:R:A0+0:64", "L chap_conv_fwd s1 | wpacked:R:A0+0:64")) == []
    found = races(record("L chap_wgrad s0 | dw:RW:A0+0:64", "L chap_wgrad s1 | dw:RW:A0+0:64"))   # no float atomics: an unordered += is order dependent
    assert len(found) == 1 and found[0]["fields"] == [("dw:RW", "dw:RW")]


def test_the_recorders_own_findings_come_through():
    found = analyze(record("X chap_perturb x: pointer in no live allocation", WRITE_A))
    assert [f["kind"] for f in found] == ["recorder"] and found[0]["line"] == 1


# ---------------------------------------------------------------------------------------------------------------- through the access table
def _launch(name, params, where):
    """The L line of one launch as the recorder writes it, with every pointer taken as an offset into one allocation A0."""
    acc = []
    for path, mode, addr, ext in launch_access.accesses(name, params):
        assert ext is not None, path
        acc.append("%s:%s:%s" % (path, mode, launch_order.format_extent("A0", ext[0], ext)))
    return "L %s %s | %s" % (name, where, " ".join(acc))


def _wgrad(a, b, dw, ws):
    p = L.WgradParams()
    p.na, p.dtype, p.dims, p.ksize, p.stride = 1, L.F32, 2, 3, 1
    p.N, p.D, p.H, p.W, p.ID, p.IH, p.IW = 1, 1, 4, 4, 1, 4, 4
    for s, ptr in ((p.a[0], a), (p.b, b)):
        s.ptr, s.C, s.ld = ptr, 16, 16
    p.dw, p.ws, p.ws_bytes, p.s_kn, p.s_kc, p.s_tap = dw, ws, 1024, 144, 9, 1
    return p


def test_two_lanes_accumulating_into_one_dw_are_flagged():
    """The weight gradients of two passes of one layer, in two lanes of one region, into the SAME gradient bucket.  This is the case that fails
    when the table says R for chap_wgrad's dw: the two launches then only read common memory."""
    assert launch_access.MODES["chap_wgrad"]["dw"] == "RW"
    lanes = lambda dw1: record("GB s0 g0", _launch("chap_wgrad", _wgrad(0x1000, 0x2000, 0x10000, 0x20000), "s0 g0 l0"), "GN g0 l1",
                               _launch("chap_wgrad", _wgrad(0x3000, 0x4000, dw1, 0x30000), "s0 g0 l1"), "GE g0")
    found = races(lanes(0x10000))
    assert len(found) == 1 and found[0]["fields"] == [("dw:RW", "dw:RW")]
    assert analyze(lanes(0x10000 + 16 * 16 * 9 * 4)) == []           # the next layer's slice of the flat gradient buffer


def _grad_norm(grad, ws, state, ring=4):
    p = L.GradNormParams()
    p.grad, p.n, p.ring, p.ws, p.state = grad, 256, ring, ws, state
    return p


def test_the_guards_state_block_is_written_by_the_norm_launch(monkeypatch):
    """chap_grad_norm on one stream, StepGuard's copy of the state block on another, no join: a finding -- and only because the table says
    that the launch WRITES the block.  With `state` declared R the same record is clean: the mode carries the finding, not the analyser."""
    assert launch_access.MODES["chap_grad_norm"]["state"] == "RW"
    state, nbytes = 0x9000, 32 + 4 * 16
    copy = "T copy_ s1 | a1:R:A0+%d:%d" % (state, nbytes)
    text = lambda: record(_launch("chap_grad_norm", _grad_norm(0x1000, 0x4000, state), "s0"), copy)
    found = races(text())
    assert len(found) == 1 and found[0]["fields"] == [("state:RW", "a1:R")] and "chap_grad_norm on s0" in found[0]["text"]
    assert analyze(record(text().splitlines()[0], "ER e0 s0", "WE s1 e0", copy)) == []           # the reader's wait for its `ready` event
    assert len(races(record(text().splitlines()[0], copy.replace("A0+%d:" % state, "A0+%d:" % (state + nbytes))))) == 0      # behind the last row
    assert len(races(record(text().splitlines()[0], copy.replace(":%d" % nbytes, ":4").replace("+%d" % state, "+%d" % (state + nbytes - 4))))) == 1
    monkeypatch.setitem(launch_access.MODES["chap_grad_norm"], "state", "R")
    assert "state:R:" in text() and analyze(text()) == []


# ---------------------------------------------------------------------------------------------------------------- the committed records
def _golden(golden_dir, name):
    return launch_order.read_record(os.path.join(golden_dir, name))


@pytest.fixture(scope="module")
def all_captured(golden_dir):
    """The captured 2D step with teacher, guard and monitor attached (issue_trace.OPT_CASES['2d_all_captured'])."""
    return _golden(golden_dir, "launch_order_2d_all_captured.txt.gz")


@pytest.fixture(scope="module")
def interval(golden_dir):
    """issue_trace.record_interval(): three replays of that capture with a validation interval between the second and the third."""
    return _golden(golden_dir, "launch_order_2d_all_interval.txt.gz")


OPT_IN = ("chap_grad_norm", "chap_sgd_guard_step", "chap_monitor_accumulate", "chap_monitor_accumulate_labels", "chap_monitor_finalize")
# Entry points of the record that no join protects, each with the reason: named here so that none is dropped silently.
ALL_ON_ITS_OWN_STREAM = {
    "chap_monitor_accumulate": "issued behind chap_pseudo_block on the capture's origin stream: both heads' pass-A logits are complete there (the forked "
                               "decoder has been joined), the labels are the static batch, and its region of the workspace is read by the finalize "
                               "launch on the same stream -- program order settles every conflict it has",
}


def _names(finding):
    """the two launches of a finding, as (kind, name) pairs"""
    return [tuple(w.split(": ")[1].split()[:2]) for w in (finding["a"], finding["b"])]


def test_committed_opt_in_records_are_clean(all_captured, interval):
    an = launch_order.Analysis(all_captured)
    assert an.findings() == []
    c = an.counts()
    print(c)
    assert c["launches"] > 500 and c["streams"] >= 4 and c["ordered_conflicts"] > 1000
    names = [e.name for e in an.events if e.kind == "L"]
    assert [names.count(n) for n in OPT_IN] == [1] * 5 and "chap_sgd_step" not in names and "chap_sgd_ema_step" not in names
    opt = next(e for e in an.events if e.name == "chap_sgd_guard_step")
    assert {f for f, m, _, _ in opt.acc} >= {"se.ema", "se.coef", "state"}                       # the teacher's average rides in the guarded launch
    an = launch_order.Analysis(interval)
    assert an.findings() == []
    c = an.counts()
    print(c)
    assert c["replays"] == 3 and c["launches"] > 50 and c["torch_ops"] > 20 and c["streams"] >= 4


def test_each_opt_in_launch_hangs_on_a_join_of_the_captured_step(all_captured):
    """launch_order.join_table on the record with all three features: for the norm launch (it reads the buckets that the weight-gradient launches
    of pass B's stream fill), the label-map accumulate (pass B's stream) and the finalize launch (the origin stream) at least one join is
    necessary and the record without it has a finding that names the entry point.  profiles/launch_order_joins_opt.txt is this table."""
    an = launch_order.Analysis(all_captured)
    lines = an.lines
    joins = launch_order.join_table(all_captured)
    named = {n: [] for n in OPT_IN}
    for n, ln, kind, extra in joins:
        unit = (n - 1, n, n + 1) if ln.startswith("WS ") and lines[n].startswith("ER ") and lines[n + 1].startswith("WE ") else (n - 1,)
        found = an.findings(skip=unit)
        assert (len(found) > 0) == (kind == "necessary") and len(found) == extra
        for name in OPT_IN:
            k = sum(("L", name) in _names(f) for f in found)
            if k:
                named[name].append((n, ln, k))
    for name, hits in named.items():
        print("%-32s %s" % (name, hits))
    for name in ("chap_grad_norm", "chap_monitor_accumulate_labels", "chap_monitor_finalize", "chap_sgd_guard_step"):
        assert named[name], "no join of the record protects %s" % name
    # ... and every other opt-in launch is listed with its reason, and the record bears the reason out
    assert {n for n, hits in named.items() if not hits} == set(ALL_ON_ITS_OWN_STREAM)
    for name in ALL_ON_ITS_OWN_STREAM:
        mine = [i for i, e in enumerate(an.events) if e.name == name]
        assert len(mine) == 1 and not any(mine[0] in key for key in an.pairs)                     # no conflict across streams at all
        assert an.events[mine[0]].stream == lines[0].split()[2]                                   # the origin stream (line 1: the seed increment)
    # the join behind pass B -- main.wait_stream(side) in ChapStep._iteration -- is one that all three hang on
    origin = lines[0].split()[2]
    side = next(e.stream for e in an.events if e.name == "chap_monitor_accumulate_labels")
    assert side != origin
    for name in ("chap_grad_norm", "chap_monitor_accumulate_labels", "chap_monitor_finalize"):
        assert "WS %s %s" % (origin, side) in [ln for _, ln, _ in named[name]], name


def _readers(text):
    """[(line of the reader's wait for its `ready` event, line of its copy, line of the host's wait for its `copied` event)] of the device-to-host
    copies between the second and the third replay that run on a stream of their own: StepMonitor.read(), then StepGuard.read()."""
    lines = text.splitlines()
    gr = [n for n, ln in enumerate(lines) if ln.startswith("GR ")]
    main = lines[gr[0]].split()[1]
    out = []
    for n in range(gr[1], gr[2]):
        f = lines[n].split(" | ")[0].split()
        if f[:2] == ["T", "copy_"] and f[2] != main and ":W:" not in lines[n]:
            assert lines[n - 2].split()[0] == "ER" and lines[n - 2].split()[2] == main             # ready.record(current stream)
            assert lines[n - 1] == "WE %s %s" % (f[2], lines[n - 2].split()[1])
            assert lines[n + 1] == "ER %s %s" % (lines[n + 1].split()[1], f[2]) and lines[n + 2] == "ES %s" % lines[n + 1].split()[1]
            out.append((n - 1, n, n + 2))
    return lines, gr, out


def test_the_interval_record_has_both_readers_on_streams_of_their_own(interval):
    lines, gr, readers = _readers(interval)
    assert len(gr) == 3 and len(readers) == 2
    (_, mon, _), (_, guard, _) = readers
    assert lines[mon].split()[2] != lines[guard].split()[2]
    size = lambda n: launch_order.parse_extent(lines[n].partition(" | ")[2].split(":", 2)[2])[1][2]
    # the monitor's ring of 8 rows of 1 + 2 * (8 + 5 * 4) + 2 * 16 + 16 = 105 words; the guard's header and its 256 rows
    assert size(mon) == 8 * 105 * 8 and size(guard) == 32 + 256 * 16


@pytest.mark.parametrize("reader", ["monitor", "guard"])
def test_a_reader_without_its_waits_meets_the_replays(interval, reader):
    """The reader's `WE <own stream> <ready event>` taken out: its copy is no longer behind the replay that wrote what it copies.  The host's
    wait for the copy (ES) taken out: the next replay may overwrite what is still being copied.

    Each reader is checked in a record that holds it alone.  In the full record the guard's stream wait is IMPLIED: monitor.read() runs
    first and ends with the host waiting for a copy that itself waited for the replay, so everything the host issues afterwards -- the guard's
    copy included -- is behind that replay whatever the guard's own stream waits for (asserted below).  StepGuard.read() must not lean on
    a monitor being attached, so the monitor's five lines are taken out before the guard's wait is."""
    lines, gr, readers = _readers(interval)
    mon, guard = readers
    if reader == "guard":
        an = launch_order.Analysis(interval)
        assert an.findings(skip=guard[0]) == [], "the guard's stream wait used to be implied by the monitor reader's host wait"
        assert (gr[1] + 1, guard[1] + 1) in [f["lines"] for f in an.findings(skip=(guard[0], mon[2]))]       # ... and by nothing else
    other = guard if reader == "monitor" else mon
    keep = [ln for n, ln in enumerate(lines) if not other[0] - 1 <= n <= other[2]]                # ER ready, WE, copy_, ER copied, ES
    assert len(keep) == len(lines) - 5
    text = "\n".join(keep) + "\n"
    lines, gr, readers = _readers(text)
    assert len(readers) == 1
    wait, copy, host_wait = readers[0]
    an = launch_order.Analysis(text)
    assert an.findings() == []
    found = an.findings(skip=wait)
    print("%s reader without %r: %s" % (reader, lines[wait], [f["lines"] for f in found]))
    assert (gr[1] + 1, copy + 1) in [f["lines"] for f in found]                                   # the replay just before the interval
    assert all(copy + 1 in f["lines"] and _names(f)[0] == ("GR", "graph_replay") for f in found)
    found = an.findings(skip=host_wait)
    print("%s reader without %r: %s" % (reader, lines[host_wait], [f["lines"] for f in found]))
    assert [f["lines"] for f in found] == [(copy + 1, gr[2] + 1)]                                 # the replay behind the interval
    assert len(an.findings(skip=(wait, host_wait))) == 3                                          # all three replays write what the copy reads


@pytest.fixture(scope="module")
def captured_2d(golden_dir):
    with gzip.open(os.path.join(golden_dir, "launch_order_2d_captured.txt.gz"), "rt") as f:
        return f.read()


@pytest.fixture(scope="module")
def joins(captured_2d):
    return launch_order.join_table(captured_2d)


def test_committed_record_is_clean(captured_2d):
    an = launch_order.Analysis(captured_2d)
    assert an.findings() == []
    c = an.counts()
    print(c)
    assert c["launches"] > 500 and c["streams"] >= 4 and c["ordered_conflicts"] > 1000


def test_taking_a_join_out_of_the_record_is_noticed(captured_2d, joins):
    """Each join of the record deleted in turn (launch_order.join_table: a WS line goes with the event pair torch's wait_stream makes of it):
    the record then has a finding -- the join is necessary -- or other edges still order everything -- implied.
    profiles/launch_order_joins.txt is this table (`python -m tests.launch_order tests/golden/launch_order_2d_captured.txt.gz`).

    Streams of the record: the capture's origin stream is the one of the first line (the seed increment); _decoder_fork opens with the
    first wait, `WS <d2> <origin>`; the side stream of pass B is the last stream the origin waits for other than d2.

    The wait that ends _decoder_fork (`origin.wait_stream(self._d2)`) is the LAST line of the record that joins d2.  Alone it is implied:
    the executor closes every forked pass with the same wait (`cur_stream.wait_stream(side)`, engine.py), the last forked pass is the last
    thing _decoder_fork contains, and nothing is issued on d2 between the two waits.  So the edge is deleted as what it is, one edge issued
    twice: both waits together are necessary, each alone is implied by the other."""
    lines = captured_2d.splitlines()
    waits = [(n, ln) for n, ln in enumerate(lines) if ln.startswith(("WS ", "WE "))]
    triples = sum(1 for n, ln, _, _ in joins if ln.startswith("WS ") and lines[n].startswith("ER ") and lines[n + 1].startswith("WE "))
    assert len(joins) + triples == len(waits)                       # every WS / WE line is in exactly one join
    necessary = [j for j in joins if j[2] == "necessary"]
    print("%d of %d joins necessary" % (len(necessary), len(joins)))
    assert len(necessary) > 0
    table = {n: kind for n, _, kind, _ in joins}

    origin = lines[0].split()[2]
    assert lines[0].startswith("T add_")                            # ChapStep.capture: seed_dev.add_(1) opens the captured iteration
    d2 = next(ln for ln in lines if ln.startswith("WS ")).split()[1]
    assert next(ln for ln in lines if ln.startswith("WS ")) == "WS %s %s" % (d2, origin)
    to_origin = [(n, ln) for n, ln, _, _ in joins if ln.startswith("WS %s " % origin)]
    # main.wait_stream(self._side) after pass B
    after_b = max(n for n, ln in to_origin if ln != "WS %s %s" % (origin, d2))
    assert table[after_b] == "necessary", "deleting main.wait_stream(side) after pass B (line %d) went unnoticed" % after_b
    # the join that ends _decoder_fork: of the origin's waits for d2, the last is ChapStep._decoder_fork's `origin.wait_stream(self._d2)`
    # (train.py, the `finally` of _decoder_fork) and the one before it the executor's `cur_stream.wait_stream(side)` that closes the last
    # forked pass (engine.py, the end of the forked backward).  A re-recorded fixture in which another wait for d2 follows the last forked
    # pass, or work is issued on d2 between the two, fails the shape assertions below before it can be misread.
    end_fork, closing = [n for n, ln in to_origin if ln == "WS %s %s" % (origin, d2)][::-1][:2]
    assert end_fork == max(n for n, _ in to_origin) and not any(ln.split()[2:3] == [d2] for ln in lines[closing:end_fork - 1] if ln[:2] in ("L ", "T "))
    an = launch_order.Analysis(captured_2d)
    both = [m - 1 + k for m in (end_fork, closing) for k in range(3)]
    assert all(lines[m].split()[0] in ("WS", "ER", "WE") for m in both)
    found = an.findings(skip=tuple(both))
    print("without the edge that ends _decoder_fork (lines %d and %d): %d findings, e.g. %s" % (closing, end_fork, len(found), found[0]["text"] if found else None))
    assert len(found) > 0, "deleting the join that ends _decoder_fork went unnoticed"
    assert table[end_fork] == table[closing] == "implied"          # (each of the two waits alone: the other one still carries the edge)
