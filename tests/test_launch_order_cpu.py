"""The happens-before check of tests/launch_order.py on small hand-written records, one per rule, and on the committed rich record of the
captured 2D step (tests/golden/launch_order_2d_captured.txt.gz, this project's own output: `python -m tests.issue_trace --rich DIR
2d_captured`): every stream wait of that record is taken out in turn -- on the record, never on the device -- and the check has to notice
the joins the iteration depends on."""
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


# ---------------------------------------------------------------------------------------------------------------- the committed record
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
