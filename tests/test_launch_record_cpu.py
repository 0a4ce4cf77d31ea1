"""The host-only parts of the rich recorder (tests/issue_trace.py): the lazily read map of the allocator's live blocks on synthetic snapshots,
what the dispatch mode makes of torch's own ops (on CPU tensors standing in for device tensors), the labels of streams the first record
never met, and the union of a capture's accesses that stands for a graph replay."""
import pytest
import torch

from chap_amd import _lib as L
from tests import issue_trace, launch_access, launch_order


# ---------------------------------------------------------------------------------------------------------------- the allocation map
class FakeAllocator:
    """One segment at 1000 of 10000 bytes; blocks as (size, live) in address order; counters as the caching allocator keeps them."""

    def __init__(self, monkeypatch, blocks):
        self.blocks, self.allocated, self.freed, self.segments = blocks, len(blocks), 0, 1
        monkeypatch.setattr(torch.cuda, "memory_stats_as_nested_dict", lambda: {
            "allocation": {"all": {"allocated": self.allocated, "freed": self.freed}}, "segment": {"all": {"allocated": self.segments, "freed": 0}}})
        monkeypatch.setattr(torch.cuda, "memory_snapshot", lambda: [{
            "address": 1000, "total_size": 10000, "blocks": [{"size": n, "state": "active_allocated" if live else "inactive"} for n, live in self.blocks]}])


def test_blocks_come_from_the_snapshot_and_it_is_read_once(monkeypatch):
    FakeAllocator(monkeypatch, [(512, True), (512, False), (1024, True)])
    a = issue_trace._Allocations()
    a.sync()
    assert a.block(1000) == (1000, 512, 1000) and a.block(1511) == (1000, 512, 1000)
    assert a.block(1512) is None and a.block(999) is None                 # an inactive block, an address in front of the segment
    assert a.block(2024) == (2024, 1024, 1000) and a.block(3048) is None
    a.sync()
    assert a.snapshots == 1 and a.label(1000) == "A0" and a.label(50000) == "A1" and a.label(1000) == "A0"


def test_an_allocation_the_mode_reported_needs_no_reading(monkeypatch):
    f = FakeAllocator(monkeypatch, [(512, True), (9488, False)])
    a = issue_trace._Allocations()
    a.sync()
    f.allocated += 1
    a.note(1512, 700)                                                     # the bytes of the storage, not the allocator's rounded block
    a.sync()
    assert a.snapshots == 1
    assert a.block(1512) == (1512, 700, 1000) and a.block(2211) == (1512, 700, 1000) and a.block(1000) == (1000, 512, 1000)
    f.blocks = [(512, True), (1024, True), (8464, False)]
    assert a.block(3000) is None and a.snapshots == 2                     # a miss is looked up in a fresh snapshot before it is a finding
    assert a.block(3000) is None and a.snapshots == 2 and a.block(2300) == (1512, 1024, 1000)          # ... once per launch, and the reading is the truth from then on


def test_an_allocation_the_mode_did_not_see_forces_a_reading(monkeypatch):
    f = FakeAllocator(monkeypatch, [(512, True), (9488, False)])
    a = issue_trace._Allocations()
    a.sync()
    f.allocated += 2                                                      # two allocations, one reported
    a.note(1512, 512)
    f.blocks = [(512, True), (512, True), (2048, True), (6928, False)]
    a.sync()
    assert a.snapshots == 2 and a.block(3000) == (2024, 2048, 1000)
    f.segments += 1                                                       # a segment came: labels and blocks may have moved
    a.sync()
    assert a.snapshots == 3


def test_a_snapshot_block_that_has_been_allocated_over_is_stale(monkeypatch):
    f = FakeAllocator(monkeypatch, [(2048, True), (7952, False)])
    a = issue_trace._Allocations()
    a.sync()
    assert a.block(2500) == (1000, 2048, 1000)
    # the 2048-byte block is freed and its first half handed out again: seen by the mode, so no reading at sync() ...
    f.freed, f.allocated = f.freed + 1, f.allocated + 1
    a.note(1000, 1024)
    a.sync()
    assert a.snapshots == 1 and a.block(1500) == (1000, 1024, 1000)
    # ... but an address in the old block's second half must not resolve to the old block (its extent would be the old 2048 bytes)
    f.blocks = [(1024, True), (1024, False), (7952, False)]
    assert a.block(2500) is None and a.snapshots == 2


def test_noted_allocations_replace_what_they_overlap(monkeypatch):
    FakeAllocator(monkeypatch, [(10000, False)])
    a = issue_trace._Allocations()
    a.sync()
    for ptr, n in ((5000, 100), (5200, 100), (5400, 100), (5050, 300)):   # the last one covers the tail of the first and all of the second
        a.note(ptr, n)
    assert [o[:2] for o in a._over] == [(5050, 300), (5400, 100)] and a._over_starts == [5050, 5400]
    assert a.block(5020) is None and a.block(5349) == (5050, 300, 1000) and a.block(5400) == (5400, 100, 1000)


def test_a_freed_block_counts_as_live_until_read_again_unless_exact(monkeypatch):
    f = FakeAllocator(monkeypatch, [(512, True), (9488, False)])
    lazy, exact = issue_trace._Allocations(), issue_trace._Allocations(exact=True)
    lazy.sync(), exact.sync()
    f.freed, f.blocks = 1, [(512, False), (9488, False)]
    lazy.sync(), exact.sync()
    assert lazy.block(1100) == (1000, 512, 1000) and lazy.snapshots == 1  # the documented limit of the lazy map
    assert exact.block(1100) is None and exact.snapshots == 2             # a dangling pointer is a finding at issue time


# ---------------------------------------------------------------------------------------------------------------- the recorder on the host
class OneSegment:
    """Every address in one live allocation: label A0, offset = the address."""

    def sync(self):
        pass

    def note(self, ptr, nbytes):
        pass

    def block(self, ptr):
        return (0, 1 << 62, 0)

    def label(self, segment):
        return "A0"


class HostRecorder(issue_trace.RichRecorder):
    """A RichRecorder that takes CPU tensors for device tensors and stream handle `stream` for the current stream."""
    stream = 7

    def _on(self):
        return True

    @staticmethod
    def _is_dev(t):
        return True

    def _cur(self):
        return self._rs(self.stream)


def _ops(rec, fn):
    before = len(rec.rich)
    fn()
    return [ln.replace(" | ", " ").split() for ln in rec.rich[before:]]


def test_torch_ops_reads_writes_views_and_host_copies(monkeypatch):
    monkeypatch.setattr(L, "call", lambda name, params, stream: None)
    rec = HostRecorder(allocations=OneSegment())
    with rec.recording():
        a, b = torch.zeros(4, 4), torch.ones(4, 4)
        pa, pb = a.data_ptr(), b.data_ptr()
        assert _ops(rec, lambda: a.copy_(b)) == [["T", "copy_", "@s7@", "a1:R:A0+%d:64" % pb, "a0:W:A0+%d:64" % pa]]
        assert _ops(rec, lambda: a[1:3].zero_()) == [["T", "zero_", "@s7@", "a0:W:A0+%d:32" % (pa + 16)]]        # a view: no line; its fill: its own span
        assert _ops(rec, lambda: a[:, 1].fill_(2.0)) == [["T", "fill_.Scalar", "@s7@", "a0:W:A0+%d:%d" % (pa + 4, 13 * 4)]]     # strided: first to last element
        assert _ops(rec, lambda: (torch.empty(3), a.view(16), a.t(), a.detach())) == []                          # allocations and views are no device work
        got = _ops(rec, lambda: a.sum().item())
        assert [g[1] for g in got[:2]] == ["sum", "_local_scalar_dense"] and got[2] == ["SS", "@s7@"]                # .item(): the host waits for the stream
        assert got[0][3] == "a0:R:A0+%d:64" % pa and got[0][4].startswith("out0:W:") and got[1][3].startswith("a0:R:")
        p = L.AxpyParams()
        p.x, p.out, p.n = 4096, 8192, 16
        L.call("chap_perturb", p, 7)
    assert rec.lines == ["L chap_perturb s0"] and rec.text() == "L chap_perturb s0\n"                            # the first record sees none of it
    assert rec.rich[-1] == "L chap_perturb s0 | x:R:A0+4096:64 out:W:A0+8192:64"
    text = rec.rich_text()
    assert "@" not in text and "T copy_ s0 |" in text                     # stream 7 got its label from the first record's launch
    assert launch_order.analyze(text) == []


def test_streams_and_events_only_the_rich_record_meets_get_later_labels(monkeypatch):
    monkeypatch.setattr(L, "call", lambda name, params, stream: None)
    rec = HostRecorder(allocations=OneSegment())
    with rec.recording():
        rec.stream = 9
        torch.zeros(2).add_(1)                                            # a torch op on a stream that never launches
        rec.rich.append("SS %s" % rec._rs(9))
        rec.rich.append("ES %s" % rec._re(object()))
        L.call("chap_perturb", L.AxpyParams(), 5)
    assert rec._streams == {5: "s0"} and rec.text() == "L chap_perturb s0\n"          # labels of the first record go by ITS first appearances
    lines = rec.rich_text().splitlines()
    assert lines[0].startswith("T zeros s1 |") and lines[1].startswith("T add_.Tensor s1 |") and lines[2:] == ["SS s1", "ES e0", "L chap_perturb s0 | "]


def test_a_pointer_in_no_allocation_and_an_extent_past_its_allocation_are_findings():
    class Small(OneSegment):
        def block(self, ptr):
            return (4096, 100, 4096) if 4096 <= ptr < 4196 else None
    rec = HostRecorder(allocations=Small())
    p = L.AxpyParams()
    p.x, p.out, p.n = 4096, 9000, 30                                      # x: 120 bytes in an allocation of 100; out: nowhere
    text = rec._access_text("chap_perturb", launch_access.accesses("chap_perturb", p))
    assert text == " | x:R:A0+0:120"
    assert rec.rich == ["X chap_perturb x: extent [0, 120) leaves its allocation of 100 bytes (pointer at +0)",
                        "X chap_perturb out: pointer in no live allocation"]
    assert [f["kind"] for f in launch_order.analyze("\n".join(rec.rich) + "\n")] == ["recorder", "recorder"]


def test_union_of_a_captures_accesses():
    rich = "\n".join(["T add_.Tensor s1 | a0:W:A0+64:8", "WS s0 s1",
                      "L chap_conv_fwd s1 | src[0].ptr:R:A1+0:64x4/128 out:W:A2+0:256 stats:W:A0+0:32",
                      "L chap_wgrad s0 g0 l1 | a[0].ptr:R:A1+448:64 dw:RW:A0+32:16 b.ptr:R:A2+128:64", "X ignored", "GE g0"]) + "\n"
    # rows count from their first to their last byte (A1+0 .. 448), ranges that touch merge (A0+0:32 with +32:16), RW is a write
    assert issue_trace.union_accesses(rich).split() == ["w0:W:A0+0:48", "w1:W:A0+64:8", "r2:R:A1+0:512", "r3:R:A2+128:64", "w4:W:A2+0:256"]
    replay = "GR s1 | %s\n" % issue_trace.union_accesses(rich)
    assert len(launch_order.analyze(replay + "T copy_ s0 | a0:W:A2+200:8\n")) == 1
    assert launch_order.analyze(replay + "T copy_ s0 | a0:W:A1+600:8\n") == []
