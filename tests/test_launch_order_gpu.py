"""No two launches of one iteration touch the same memory without an order between them.

Every case of tests/issue_trace.py (the small steps whose issue order tests/test_issue_order_gpu.py pins: 2D 8 x 64 x 64, 3D 4 x 16 x 32 x 16)
is recorded once with the rich recorder -- every launch with the bytes it reads and writes (tests/launch_access.py), torch's own copies and
fills, stream waits, events, host waits, the lanes of grouped regions -- and tests/launch_order.py looks for a pair of launches that meet
in memory, one of them writing, with no happens-before path between them.  The pinned issue order says that the schedule has not moved;
this says that it is race free as far as the access table declares what the kernels touch (a pointer in no live allocation and an extent
that leaves its allocation are findings too).  Nothing here changes what runs: the recorder only observes, and what the check would
say about a lost join is shown on records, never on the device (tests/test_launch_order_cpu.py).

The extra case is two consecutive replay() calls that take their batch from stage(): the copy stream with its two events must keep the
next batch out of the staging and the static buffers while the previous hand-over and the previous replay still read them."""
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
