"""No two launches of one iteration touch the same memory without an order between them.

Every case of tests/issue_trace.py (the small steps whose issue order tests/test_issue_order_gpu.py pins: 2D 8 x 64 x 64, 3D 4 x 16 x 32 x 16)
is recorded once with the rich recorder -- every launch with the bytes it reads and writes (tests/launch_access.py), torch's own copies and
fills, stream waits, events, host waits, the lanes of grouped regions -- and tests/launch_order.py looks for a pair of launches that meet
in memory, one of them writing, with no happens-before path between them.  The pinned issue order says that the schedule has not moved;
this says that it is race free as far as the access table declares what the kernels touch (a pointer in no live allocation and an extent
that leaves its allocation are findings too).  Nothing here changes what runs: the recorder only observes, and what the check would
say about a lost join is shown on records, never on the device (tests/test_launch_order_cpu.py).

The extra case is two consecutive replay() calls that take their batch from stage(): the copy stream with its two events must keep the
next batch out of the staging and the static buffers while the previous hand-over and the previous replay still read them.

The opt-in launches are checked the same way: issue_trace.OPT_CASES attach a mean teacher, a gradient guard and a training monitor to the
same steps; one record holds what train() does at a validation interval between two replays (the student's and the teacher's evaluation,
StepMonitor.read() and StepGuard.read() on streams of their own); two hold stage_from(loader), where the loader's augmentation kernel fills
the staging buffers beside the running replay."""
import pytest

pytestmark = pytest.mark.gpu

from tests import issue_trace, launch_order


def _report(name, rich):
    an = launch_order.Analysis(rich)
    found = an.findings()
    c = an.counts()
    print("%s: %d launches, %d torch ops, %d replays, %d streams, %d conflicting pairs all ordered but %d"
          % (name, c["launches"], c["torch_ops"], c["replays"], c["streams"], c["ordered_conflicts"], len(found)))
    return c, found


def _fail_text(found):
    return "%d unordered conflicts, the first:\n%s" % (len(found), "\n".join(f["text"] for f in found[:10]))


# Recorded with the allocator's snapshot read after every allocation AND free, so that a pointer into a block that has been freed and not
# yet handed out again is a finding at the launch that carries it.  The other cases read it lazily (a freed block counts as live until it
# is handed out again, from when on the record names the same bytes and the order check sees them): three to five times faster.
EXACT = ("2d_eager", "2d_captured", "3d_eager", "3d_captured")


@pytest.mark.parametrize("case", list(issue_trace.CASES))
def test_every_conflicting_pair_of_launches_is_ordered(case):
    plain, rich = issue_trace.record_case(case, rich=True, exact=case in EXACT)
    c, found = _report(case, rich)
    assert c["launches"] == issue_trace.counts(plain)["launches"] > 0          # every launch of the first record is in the rich one
    assert [ln.split(" | ")[0] for ln in rich.splitlines() if ln[:2] in ("L ", "GB", "GN", "GE", "WS", "WE", "ER")] == plain.splitlines()
    assert c["torch_ops"] > 0 and c["ordered_conflicts"] > 0
    bare = [ln for ln in rich.splitlines() if ln.startswith("L ") and not ln.partition(" | ")[2].strip()]
    assert bare == [], "launches without any access would pass as conflict free: %s" % bare[:5]
    assert found == [], _fail_text(found)


OPT_EXACT = ("2d_all_captured", "3d_all_captured")


@pytest.mark.parametrize("case", list(issue_trace.OPT_CASES))
def test_every_conflicting_pair_is_ordered_with_the_opt_in_features_attached(case):
    """The same check with a mean teacher, a gradient guard and a training monitor attached (issue_trace.OPT_CASES): their launches are in
    the record, each with its accesses -- the optimizer entry that the features put in place of chap_sgd_step, the norm launch in front of
    it, the monitor's launches -- and they are ordered against everything they meet in memory."""
    plain, rich = issue_trace.record_case(case, rich=True, exact=case in OPT_EXACT)
    c, found = _report(case, rich)
    assert c["launches"] == issue_trace.counts(plain)["launches"] > 0
    assert [ln.split(" | ")[0] for ln in rich.splitlines() if ln[:2] in ("L ", "GB", "GN", "GE", "WS", "WE", "ER")] == plain.splitlines()
    assert c["torch_ops"] > 0 and c["ordered_conflicts"] > 0
    launches = [ln for ln in rich.splitlines() if ln.startswith("L ")]
    bare = [ln for ln in launches if not ln.partition(" | ")[2].strip()]
    assert bare == [], "launches without any access would pass as conflict free: %s" % bare[:5]
    want, absent = issue_trace.opt_entry_points(issue_trace.OPT_CASES[case])
    names = [ln.split()[1] for ln in launches]
    assert want and {n: names.count(n) for n in want} == want
    assert {n: names.count(n) for n in absent} == {n: 0 for n in absent}
    assert found == [], _fail_text(found)


@pytest.mark.parametrize("case", ["2d_all_eager", "3d_all_eager", "2d_ablation_all_eager"])
def test_the_recorded_guarded_step_clips(case):
    """issue_trace.GUARD_MAX_NORM is far below the gradient norm of the recorded steps: the guarded optimizer launch of every guarded case takes
    its scaled path (0 < coef < 1), not the one that equals the plain launch."""
    step, inp, inj = issue_trace._case_step(case)
    step.step(inp["vol"], inp["lab"], box_yx=inp["box"], inject=inj)
    rows = step.guard.read()
    print("%s: gradient norm %.6g, max_norm %g, coef %.6g" % (case, rows["norm"][0], issue_trace.GUARD_MAX_NORM, rows["coef"][0]))
    assert rows["steps"] == 1 and rows["skip"].tolist() == [0] and rows["clipped_total"] == 1
    assert 0 < float(rows["coef"][0]) < 0.1 and float(rows["norm"][0]) > 10 * issue_trace.GUARD_MAX_NORM


def _between(name):
    captured, rich = (issue_trace.record_interval() if name == issue_trace.INTERVAL else issue_trace.record_loader_replays(name))
    assert launch_order.analyze(captured) == []
    an = launch_order.Analysis(rich)
    found, c = an.findings(), an.counts()           # (leaves the clocks of the full record in `an`: _before below reads them)
    print("%s: %d launches, %d torch ops, %d replays, %d streams, %d conflicting pairs all ordered but %d"
          % (name, c["launches"], c["torch_ops"], c["replays"], c["streams"], c["ordered_conflicts"], len(found)))
    return rich.splitlines(), an, c, found


def test_the_readers_of_a_validation_interval_never_meet_a_replay():
    """issue_trace.record_interval: between the second and the third replay the student and the teacher are evaluated and the monitor's
    ring and the guard's state block are copied out, each on its reader's own stream."""
    lines, an, c, found = _between(issue_trace.INTERVAL)
    assert found == [], _fail_text(found)
    assert c["replays"] == 3 and sum(ln.startswith("GR ") for ln in lines) == 3
    replay_stream = {ln.split()[1] for ln in lines if ln.startswith("GR ")}
    assert len(replay_stream) == 1
    main = replay_stream.pop()
    gr = [n for n, ln in enumerate(lines) if ln.startswith("GR ")]
    copies = [n for n, ln in enumerate(lines) if ln.startswith("T copy_ ") and ln.split()[2] != main and gr[1] < n < gr[2]
              and ":W:" not in ln.partition(" | ")[2]]               # device to host: nothing written on the device
    assert len(copies) == 2 and lines[copies[0]].split()[2] != lines[copies[1]].split()[2]       # monitor.read(), then guard.read(): two streams
    ev = {e.line: i for i, e in enumerate(an.events)}
    for n in copies:
        for g in (gr[1], gr[2]):        # the replay before wrote what the copy reads, the replay after writes it again: a conflict, and ordered
            key = tuple(sorted((ev[n], ev[g])))
            assert key in an.pairs, (lines[n], g)
        a, before, after = an.events[ev[n]], an.events[ev[gr[1]]], an.events[ev[gr[2]]]
        assert an._before(before, a) and an._before(a, after) and not an._before(a, before)


@pytest.mark.parametrize("name", list(issue_trace.LOADER_REPLAYS))
def test_device_built_batches_never_land_under_a_running_replay(name):
    """issue_trace.record_loader_replays: the loader's augmentation kernel fills the staging buffers on the copy stream."""
    lines, an, c, found = _between(name)
    assert found == [], _fail_text(found)
    assert c["replays"] == 2
    aug = [n for n, ln in enumerate(lines) if ln.startswith("L chap_augment")]
    assert len(aug) == 2 and all(lines[n].split()[1] == ("chap_augment2d" if name.startswith("2d") else "chap_augment3d_padded") for n in aug)
    for n in aug:
        acc = {item.split(":")[0]: item.split(":")[1] for item in lines[n].partition(" | ")[2].split()}
        assert acc == dict(images="R", labels="R", records="R", image_out="W", label_out="W"), lines[n]
    main = next(ln for ln in lines if ln.startswith("GR ")).split()[1]
    copy_stream = lines[aug[0]].split()[2]
    assert copy_stream != main and lines[aug[1]].split()[2] == copy_stream
    # the second stage_from overwrites the staging buffers, which the first replay()'s copies into the static buffers read: ordered, through
    # the hand-over event alone -- the record without that wait has exactly these pairs unordered
    first_gr = next(n for n, ln in enumerate(lines) if ln.startswith("GR "))
    taken = [n for n, ln in enumerate(lines) if ln.startswith("T copy_ %s " % main) and aug[0] < n < first_gr]
    ev = {e.line: i for i, e in enumerate(an.events)}
    met = [n for n in taken if (ev[n], ev[aug[1]]) in an.pairs]
    assert len(met) == 2                                            # image and label
    assert all(an._before(an.events[ev[n]], an.events[ev[aug[1]]]) for n in met)
    wait = [n for n, ln in enumerate(lines) if ln.startswith("WE %s " % copy_stream) and first_gr < n < aug[1]]
    assert len(wait) == 1
    lost = an.findings(skip=wait[0])
    assert sorted(f["lines"] for f in lost) == sorted((n + 1, aug[1] + 1) for n in met), lost[:4]


def test_staged_batches_never_land_under_a_running_replay():
    captured, rich = issue_trace.record_staged_replays()
    c, found = _report(issue_trace.STAGED_REPLAY, rich)
    assert launch_order.analyze(captured) == []
    lines = rich.splitlines()
    assert c["replays"] == 2 and c["streams"] == 2
    assert sum(ln.startswith("WE ") for ln in lines) == 3          # replay waits for the staged batch (twice), the second stage() for the hand-over
    assert sum(ln.startswith("T copy_") for ln in lines) >= 8      # two batches: image and label into the staging buffers, then into the static ones
    replay = next(ln for ln in lines if ln.startswith("GR "))
    assert ":R:" in replay and ":W:" in replay
    assert found == [], _fail_text(found)
