"""Issue-order recorder: what ONE training iteration hands to the runtime, in the order in which it is handed over.

Under capture the issue order is the creation order of the graph's nodes, by which the ROCm 7.2 graph executor places the chains on
its hardware queues ("Issue order": it alone moves a 2D step between 6.5 and 8.05 ms), and a lost join is a race
that the bit-identity tests may pass by luck.  So the record holds, one line each and in issue order:

    L <entry point> <stream> [g<region> l<lane>]     every _lib.call(name, params, stream) and _lib.pack_multi(...) (`chap_pack_multi`)
    GB <stream> g<region> / GN g<region> l<lane> / GE g<region>      begin, next_lane and end of an enabled _lib.group region
    WS <stream> <stream>   Stream.wait_stream        WE <stream> <event>   Stream.wait_event        ER <event> <stream>   Event.record

Streams and events are labelled by order of first appearance (s0, s1, ..., e0, ...), so a record does not depend on handles.  Torch's
own copies and fills (copy_, zero_, add_ on the seed word, the schedule-block upload) are not recorded, and neither are a launch's
parameters (CHAP_SPLIT_CONCAT=0 issues the same entry points as the default: its record equals 2d_eager's).  The recorder only observes:
every patched function calls through, and what was patched is restored in a `finally`.

An eager step() is recorded directly; a capture is recorded during capture(warmup=1) with the recording switched on for the captured
pass only (the warm-up is eager).  The four-graph data-parallel capture (ChapStep._capture_dp) needs RCCL and is left to the
bit-identity tests of tests/test_parallel_gpu.py.

`python -m tests.issue_trace DIR [case ...]` writes every case's full record to DIR/<case>.txt and the fixture lines (case name,
SHA-256 of the record, counts) to DIR/summary.txt; tests/golden/issue_order_parent.txt is such a summary, made on the commit BEFORE the
executor's and the training step's schedules were rewritten (tests/test_issue_order_gpu.py).

RichRecorder keeps a second record beside that one, which `text()` and its hashes do not see: every launch with the memory it reads and
writes, torch's own device work, the host's waits (`python -m tests.issue_trace --rich DIR [case ...]` writes DIR/<case>.rich.txt).
tests/launch_order.py checks on it that every two launches which meet in memory are ordered (tests/test_launch_order_gpu.py).

OPT_CASES are the same steps with the opt-in features attached (mean teacher, gradient guard, monitor), rich records only; record_interval()
and record_loader_replays() record what runs between and beside replays (a validation interval with both readers; stage_from(loader)).
"""
import bisect
import contextlib
import hashlib
import os
import re
import sys

import torch

DEV = "cuda"


class Recorder:
    def __init__(self, only_capturing=False):
        self.lines, self.only_capturing = [], only_capturing
        self._streams, self._events, self._keep = {}, {}, []
        self._region, self._lane, self._nregions = None, 0, 0

    def _line(self, line):
        """One line of the record (RichRecorder keeps a second record beside it)."""
        self.lines.append(line)

    def _on(self):
        return not self.only_capturing or torch.cuda.is_current_stream_capturing()

    def _s(self, handle):
        handle = int(handle or 0)
        return self._streams.setdefault(handle, "s%d" % len(self._streams))

    def _e(self, event):
        if id(event) not in self._events:
            self._keep.append(event)            # (kept alive: the id of a freed event would be handed out again)
            self._events[id(event)] = "e%d" % len(self._events)
        return self._events[id(event)]

    def launch(self, name, stream):
        if self._on():
            where = "" if self._region is None else " g%d l%d" % (self._region, self._lane)
            self._line("L %s %s%s" % (name, self._s(stream), where))

    @contextlib.contextmanager
    def recording(self):
        from chap_amd import _lib as L
        rec = self
        saved = (L.call, L.pack_multi, L.group.__enter__, L.group.next_lane, L.group.__exit__,
                 torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record)
        call, pack_multi, g_enter, g_next, g_exit, wait_stream, wait_event, ev_record = saved

        def r_call(name, params, stream):
            rec.launch(name, stream)
            return call(name, params, stream)

        def r_pack_multi(entries, n, max_total, stream):
            rec.launch("chap_pack_multi", stream)
            return pack_multi(entries, n, max_total, stream)

        def r_enter(self):
            if self.enabled and rec._on():
                rec._region, rec._lane, rec._nregions = rec._nregions, 0, rec._nregions + 1
                rec._line("GB %s g%d" % (rec._s(self.stream), rec._region))
            return g_enter(self)

        def r_next(self):
            if self.enabled and rec._region is not None:
                rec._lane += 1
                rec._line("GN g%d l%d" % (rec._region, rec._lane))
            return g_next(self)

        def r_exit(self, et, ev, tb):
            if self.enabled and rec._region is not None:
                rec._line("GE g%d" % rec._region)
                rec._region = None
            return g_exit(self, et, ev, tb)

        def r_wait_stream(self, stream):
            if rec._on():
                rec._line("WS %s %s" % (rec._s(self.cuda_stream), rec._s(stream.cuda_stream)))
            return wait_stream(self, stream)

        def r_wait_event(self, event):
            if rec._on():
                rec._line("WE %s %s" % (rec._s(self.cuda_stream), rec._e(event)))
            return wait_event(self, event)

        def r_record(self, stream=None):
            if rec._on():
                st = torch.cuda.current_stream() if stream is None else stream
                rec._line("ER %s %s" % (rec._e(self), rec._s(st.cuda_stream)))
            return ev_record(self, stream)

        try:
            L.call, L.pack_multi = r_call, r_pack_multi
            L.group.__enter__, L.group.next_lane, L.group.__exit__ = r_enter, r_next, r_exit
            torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = r_wait_stream, r_wait_event, r_record
            yield self
        finally:
            (L.call, L.pack_multi, L.group.__enter__, L.group.next_lane, L.group.__exit__,
             torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record) = saved

    def text(self):
        return "\n".join(self.lines) + "\n"


# ---------------------------------------------------------------------------------------------------------------- the rich record
class _Allocations:
    """The caching allocator's live blocks.  The base is torch.cuda.memory_snapshot(); reading it costs more than recording a launch and a
    step allocates in front of almost every launch, so it is read lazily: the dispatch mode reports every allocation it sees (note(): the
    storage of a fresh result, address and bytes) into an overlay on top of the last snapshot, and the snapshot is read again only when
    that cannot be the whole truth -- the allocator's counters (torch.cuda.memory_stats) show more allocations than were reported, a
    segment came or went, a pointer lies in no known block, or it lies in a snapshot block that a reported allocation has since
    overlapped.  A block freed and not handed out again stays "live" until the next reading; once it is handed out again the record
    names the same bytes, which is what the order check works on.  `exact` reads the snapshot whenever any counter has moved, frees
    included: a pointer into a freed block is then a finding at the launch that carries it (three to five times the recording time;
    tests/test_launch_order_gpu.py records the four default steps this way).  Segments are labelled A0, A1, ... in order of first appearance; an
    address is written as label + offset inside its segment, so a reused address keeps its name."""

    def __init__(self, exact=False):
        self.labels, self.snapshots, self.exact = {}, 0, exact
        self._starts, self._blocks, self._segments, self._seg_starts, self._counter, self._fresh = [], [], [], [], None, False
        self._over_starts, self._over, self._seen = [], [], 0

    @staticmethod
    def _moved():
        st = torch.cuda.memory_stats_as_nested_dict()          # (not memory_stats(): flattening it costs more than the launch being recorded)
        return tuple(st[k]["all"][d] for k in ("allocation", "segment") for d in ("allocated", "freed"))

    def _read(self):
        blocks, segments = [], []
        for seg in torch.cuda.memory_snapshot():
            at = seg["address"]
            segments.append((seg["address"], seg["total_size"]))
            for b in seg["blocks"]:
                at = b.get("address", at)
                if b["state"] == "active_allocated":
                    blocks.append((at, b["size"], seg["address"]))
                at += b["size"]
        blocks.sort()
        segments.sort()
        self._blocks, self._starts, self._segments, self._seg_starts = blocks, [b[0] for b in blocks], segments, [g[0] for g in segments]
        self._over_starts, self._over = [], []
        self.snapshots += 1
        self._fresh = True

    @staticmethod
    def _in(starts, items, ptr):
        i = bisect.bisect_right(starts, ptr) - 1
        if i >= 0 and ptr < items[i][0] + items[i][1]:
            return items[i]
        return None

    def note(self, ptr, nbytes):
        """An allocation the dispatch mode has seen: [ptr, ptr + nbytes) is live now, whatever was noted there before is gone."""
        self._seen += 1
        lo = bisect.bisect_right(self._over_starts, ptr) - 1
        if lo < 0 or self._over[lo][0] + self._over[lo][1] <= ptr:
            lo += 1
        hi = bisect.bisect_left(self._over_starts, ptr + nbytes)
        seg = self._in(self._seg_starts, self._segments, ptr)
        self._over[lo:hi] = [(ptr, nbytes, seg[0] if seg else None)]
        self._over_starts[lo:hi] = [ptr]

    def sync(self):
        """Once per recorded launch, in front of its pointers: has the allocator done anything the overlay does not know of?"""
        now = self._moved()
        self._fresh = False
        if now != self._counter:
            if self.exact or self._counter is None or now[2:] != self._counter[2:] or now[0] - self._counter[0] != self._seen:
                self._read()
            self._counter = now
        self._seen = 0

    def block(self, ptr):
        """(address, bytes, segment address) of the live allocation around ptr, or None."""
        for attempt in range(2):
            blk = self._in(self._over_starts, self._over, ptr)
            if blk is None:
                blk = self._in(self._starts, self._blocks, ptr)
                if blk is not None:          # stale if something has been allocated on top of it since the snapshot
                    i = bisect.bisect_left(self._over_starts, blk[0] + blk[1])
                    if i > 0 and self._over[i - 1][0] + self._over[i - 1][1] > blk[0]:
                        blk = None
            if blk is not None and blk[2] is not None:
                return blk
            if self._fresh:
                return None
            self._read()
        return None

    def label(self, segment):
        return self.labels.setdefault(segment, "A%d" % len(self.labels))


_NO_DEVICE_WORK = ("aten::empty", "aten::new_empty", "aten::_efficientzerotensor")      # allocations: a result, nothing written


class RichRecorder(Recorder):
    """Recorder with a second record beside the first (`rich_text()`; `text()` is unchanged, byte for byte): every L line carries the
    launch's accesses (tests/launch_access.py: field, mode, extent relative to the live allocation's segment), torch's own device work is
    there (T lines, through a TorchDispatchMode: reads are the device tensors among the arguments, writes those the op's schema marks
    as written plus the results that are no views; the extent is the span of the tensor's elements; the stream is the current one), and
    so are the host's waits (HS torch.cuda.synchronize, SS Stream.synchronize and the device-to-host copies that wait for their stream,
    ES Event.synchronize) and graph replays (GR, with the accesses in `replay_accesses`: the union of what the capture recorded).  A
    non-null pointer in no live allocation and an extent that leaves its allocation are findings (X lines).  tests/launch_order.py
    reads the format.  `pack_entries(device pointer)` returns the host-side PackEntry array behind a chap_pack_multi table."""

    def __init__(self, only_capturing=False, allocations=None, pack_entries=None, replay_accesses=""):
        super().__init__(only_capturing)
        self.rich, self._pending = [], ""
        self.allocs = allocations or _Allocations()
        self.pack_entries, self.replay_accesses = pack_entries, replay_accesses

    def _line(self, line):
        self.lines.append(line)
        self.rich.append(line + self._pending)
        self._pending = ""

    def _rs(self, handle):
        """The label of a stream in lines that only the rich record has.  A stream (or event) that the first record has not met yet must not
        get its label here -- labels go by first appearance in THAT record -- so it is written as a placeholder that rich_text() resolves."""
        handle = int(handle or 0)
        return self._streams[handle] if handle in self._streams else "@s%d@" % handle

    def _re(self, event):
        if id(event) in self._events:
            return self._events[id(event)]
        self._keep.append(event)
        return "@e%d@" % id(event)

    def rich_text(self):
        text = "\n".join(self.rich) + "\n"
        streams = dict(("@s%d@" % h, label) for h, label in self._streams.items())
        events = dict(("@e%d@" % i, label) for i, label in self._events.items())
        for token in dict.fromkeys(re.findall(r"@[se]\d+@", text)):        # what the first record never met: further labels, by first appearance here
            table = streams if token[1] == "s" else events
            if token not in table:
                table[token] = "%s%d" % (token[1], len(table))
            text = text.replace(token, table[token])
        return text

    # ------------------------------------------------------------------------------------------------------------ accesses
    def _extent(self, what, addr, ext):
        """The extent text of one access (whole live allocation when the field has no rule), or None: nothing to touch, or an X line written."""
        from tests.launch_order import format_extent
        blk = self.allocs.block(addr)
        if blk is None:
            self.rich.append("X %s: pointer in no live allocation" % what)
            return None
        start, size, segment = blk
        if ext is None:
            ext = (start, 0, size, 1)
        else:
            lo, hi = ext[0], ext[0] + (ext[3] - 1) * ext[1] + ext[2]
            if hi <= lo:
                return None
            if lo < start or hi > start + size:
                self.rich.append("X %s: extent [%d, %d) leaves its allocation of %d bytes (pointer at +%d)" % (what, lo - start, hi - start, size, addr - start))
        return format_extent(self.allocs.label(segment), ext[0] - segment, ext)

    def _access_text(self, name, acc):
        self.allocs.sync()
        out = []
        for path, mode, addr, ext in acc:
            e = self._extent("%s %s" % (name, path), addr, ext)
            if e is not None:
                out.append("%s:%s:%s" % (path, mode, e))
        return " | " + " ".join(out)

    @staticmethod
    def _span(t):
        """The bytes between a tensor's first and last element (an upper bound of a strided view, exact for a contiguous one)."""
        if t.numel() == 0:
            return None
        last = sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride()))
        return (t.data_ptr(), 0, (last + 1) * t.element_size(), 1)

    @staticmethod
    def _is_dev(t):
        return t.is_cuda

    def _cur(self):
        return self._rs(torch.cuda.current_stream().cuda_stream)

    def note_results(self, args, kwargs, result):
        """Tell the allocation map about every fresh device storage among an op's results (recording or not: the map has to stay true)."""
        def tensors(value):
            if isinstance(value, torch.Tensor):
                if self._is_dev(value):
                    yield value
            elif isinstance(value, (list, tuple)):
                for v in value:
                    yield from tensors(v)
        fresh = [t for t in tensors(result)]
        if not fresh:
            return
        known = {t.untyped_storage().data_ptr() for t in tensors(args)} | {t.untyped_storage().data_ptr() for t in tensors(tuple(kwargs.values()))}
        for t in fresh:
            st = t.untyped_storage()
            if st.data_ptr() and st.data_ptr() not in known and st.nbytes():
                known.add(st.data_ptr())
                self.allocs.note(st.data_ptr(), st.nbytes())

    def torch_op(self, func, args, kwargs, result):
        if not self._on():
            return
        schema = func._schema
        if schema.name.startswith(_NO_DEVICE_WORK):
            return
        reads, writes, storages, host_side = [], [], set(), False

        def visit(value, written, tag):
            nonlocal host_side
            if isinstance(value, torch.Tensor):
                if self._is_dev(value):
                    storages.add(value.untyped_storage().data_ptr())
                    (writes if written else reads).append((tag, value))
                elif written:
                    host_side = True
            elif isinstance(value, (list, tuple)):
                for v in value:
                    visit(v, written, tag)

        formal = schema.arguments
        for i, value in enumerate(args):
            visit(value, bool(formal[i].alias_info and formal[i].alias_info.is_write), "a%d" % i)
        for i, a in enumerate(formal):
            if a.name in kwargs:
                visit(kwargs[a.name], bool(a.alias_info and a.alias_info.is_write), "a%d" % i)
        seen = set(storages)
        results = result if isinstance(result, (list, tuple)) else (result,)
        for i, value in enumerate(results):
            if isinstance(value, torch.Tensor):
                if not self._is_dev(value):
                    host_side = True            # a device-to-host copy (_to_copy, _local_scalar_dense gives a number: below)
                elif value.untyped_storage().data_ptr() not in seen and not any(value is w for _, w in writes):
                    writes.append(("out%d" % i, value))         # a fresh result; a view of an argument is no device work
        if schema.name == "aten::_local_scalar_dense":
            host_side = True
        if not writes and not (host_side and reads):
            return
        acc = [(tag, "R", t.data_ptr(), self._span(t)) for tag, t in reads] + [(tag, "W", t.data_ptr(), self._span(t)) for tag, t in writes]
        name = schema.name.split("::")[-1] + ("." + schema.overload_name if schema.overload_name else "")
        stream = self._cur()
        self.rich.append("T %s %s%s" % (name, stream, self._access_text(name, [a for a in acc if a[3] is not None])))
        if host_side and reads and not kwargs.get("non_blocking", False) and not (len(args) > 2 and args[2] is True and schema.name == "aten::copy_"):
            self.rich.append("SS %s" % stream)          # the host waits for the copy, i.e. for everything its stream was handed before

    # ------------------------------------------------------------------------------------------------------------ patches
    @contextlib.contextmanager
    def recording(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        from chap_amd import _lib as L
        from tests import launch_access
        rec = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                kwargs = kwargs or {}
                out = func(*args, **kwargs)
                rec.note_results(args, kwargs, out)
                rec.torch_op(func, args, kwargs, out)
                return out

        with super().recording():
            saved = (L.call, L.pack_multi, torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize,
                     torch.cuda.CUDAGraph.replay)
            call, pack_multi, dev_sync, stream_sync, event_sync, replay = saved

            def r_call(name, params, stream):
                if rec._on():
                    rec._pending = rec._access_text(name, launch_access.accesses(name, params))
                return call(name, params, stream)

            def r_pack_multi(entries, n, max_total, stream):
                if rec._on():
                    host = rec.pack_entries(entries) if rec.pack_entries is not None else None
                    acc = [("entries", "R", int(entries), None)] + (launch_access.pack_multi_accesses(host[:n]) if host is not None else [])
                    if host is None:
                        rec.rich.append("X chap_pack_multi: no host-side entry list for the table at its pointer")
                    rec._pending = rec._access_text("chap_pack_multi", acc)
                return pack_multi(entries, n, max_total, stream)

            def r_dev_sync(device=None):
                out = dev_sync(device)
                if rec._on():
                    rec.rich.append("HS")
                return out

            def r_stream_sync(self):
                out = stream_sync(self)
                if rec._on():
                    rec.rich.append("SS %s" % rec._rs(self.cuda_stream))
                return out

            def r_event_sync(self):
                out = event_sync(self)
                if rec._on():
                    rec.rich.append("ES %s" % rec._re(self))
                return out

            def r_replay(self):
                if rec._on():
                    rec.rich.append("GR %s | %s" % (rec._cur(), rec.replay_accesses))
                return replay(self)

            try:
                L.call, L.pack_multi = r_call, r_pack_multi
                torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize = r_dev_sync, r_stream_sync, r_event_sync
                torch.cuda.CUDAGraph.replay = r_replay
                with Mode():
                    yield self
            finally:
                (L.call, L.pack_multi, torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize,
                 torch.cuda.CUDAGraph.replay) = saved


def union_accesses(rich_text):
    """The accesses of all L and T lines of a rich record as one access list for a GR line: per allocation label the merged ranges read
    and the merged ranges written (a row set counts with the range from its first to its last byte: an upper bound)."""
    from tests.launch_order import parse_extent
    spans = {}
    for ln in rich_text.splitlines():
        head, _, acc = ln.partition(" | ")
        if head.startswith(("L ", "T ")):
            for item in acc.split():
                _, mode, ext = item.split(":", 2)
                label, (base, pitch, row_bytes, nrows) = parse_extent(ext)
                spans.setdefault((label, "R" if mode == "R" else "W"), []).append((base, base + (nrows - 1) * pitch + row_bytes))
    out = []
    for (label, mode), ranges in sorted(spans.items()):
        ranges.sort()
        merged = [list(ranges[0])]
        for lo, hi in ranges[1:]:
            if lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], hi)
            else:
                merged.append([lo, hi])
        out += ["%s%d:%s:%s+%d:%d" % (mode.lower(), len(out) + i, mode, label, lo, hi - lo) for i, (lo, hi) in enumerate(merged)]
    return " ".join(out)


def counts(text):
    """The counts of a record: launches, grouped regions, launches per stream label, waits, event records."""
    lines = text.splitlines()
    per = {}
    for ln in lines:
        if ln.startswith("L "):
            s = ln.split()[2]
            per[s] = per.get(s, 0) + 1
    return dict(launches=sum(per.values()), regions=sum(ln.startswith("GB ") for ln in lines),
                streams=",".join("%s:%d" % (s, per[s]) for s in sorted(per, key=lambda s: int(s[1:]))),
                waits=sum(ln.startswith(("WS ", "WE ")) for ln in lines), records=sum(ln.startswith("ER ") for ln in lines))


def summary_line(name, text):
    c = counts(text)
    return "%s %s launches=%d regions=%d streams=%s waits=%d records=%d" % (
        name, hashlib.sha256(text.encode()).hexdigest(), c["launches"], c["regions"], c["streams"], c["waits"], c["records"])


def parse_summary_line(line):
    """one fixture line -> (sha256, {count name: text})"""
    _, sha, *kv = line.split()
    return sha, dict(x.split("=", 1) for x in kv)


def parse_summary(path):
    """fixture file -> {case: parse_summary_line(its line)}"""
    with open(path) as f:
        return {ln.split()[0]: parse_summary_line(ln) for ln in f if ln.strip()}


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> dict(net='2d' | '3d' | '3d_res', mode='eager' | 'captured', args=..., env=..., step='chap' | 'ablation', bf16=...)
CASES = {
    "2d_eager": dict(net="2d", mode="eager"),
    "2d_captured": dict(net="2d", mode="captured"),
    "3d_eager": dict(net="3d", mode="eager"),
    "3d_captured": dict(net="3d", mode="captured"),
    "2d_captured_single_stream": dict(net="2d", mode="captured", args=dict(concurrent=False)),
    "2d_captured_no_adv_noise": dict(net="2d", mode="captured", args=dict(adv_noise=False)),
    "2d_dropout_eager": dict(net="2d", mode="eager", args=dict(dropout=True)),
    "2d_dropout_captured": dict(net="2d", mode="captured", args=dict(dropout=True), fp_inject=True),
    "3d_residual_eager": dict(net="3d_res", mode="eager"),
    "3d_residual_captured": dict(net="3d_res", mode="captured"),
    "2d_ablation_eager": dict(net="2d", mode="eager", step="ablation"),
    "2d_captured_group0": dict(net="2d", mode="captured", env={"CHAP_GROUP": "0"}),
    "2d_captured_fork_mask15": dict(net="2d", mode="captured", env={"CHAP_FORK_MASK": "15"}),
    "2d_captured_fork_mask0": dict(net="2d", mode="captured", env={"CHAP_FORK_MASK": "0"}),
    "2d_eager_defer_wgrad0": dict(net="2d", mode="eager", env={"CHAP_DEFER_WGRAD": "0"}),
    "2d_eager_side_decoder2": dict(net="2d", mode="eager", env={"CHAP_SIDE_DECODER": "2"}),
    "2d_eager_split_concat0": dict(net="2d", mode="eager", env={"CHAP_SPLIT_CONCAT": "0"}),
    "2d_eager_bf16_c1_direct0": dict(net="2d", mode="eager", env={"CHAP_C1_DIRECT": "0"}, bf16=True),
}

# The same steps with the opt-in features attached: a mean teacher (chap_sgd_ema_step in place of chap_sgd_step), a gradient guard
# (chap_grad_norm, then chap_sgd_guard_step in its place) and a training monitor (its three launches; AblationStep: two).  NOT part of CASES:
# these have no record of the first kind in tests/golden/issue_order_parent.txt -- the features did not exist on that commit -- and are
# checked for order alone (tests/test_launch_order_gpu.py).  Further keys: teacher, guard, monitor (bool), classes (2D: the model's class
# count; three issues pass B's single-term loss launches, tests/test_class_counts_step_gpu.py).
_ALL = dict(teacher=True, guard=True, monitor=True)
OPT_CASES = {
    "2d_teacher_eager": dict(net="2d", mode="eager", teacher=True),
    "2d_teacher_captured": dict(net="2d", mode="captured", teacher=True),
    "2d_guard_eager": dict(net="2d", mode="eager", guard=True),
    "2d_guard_captured": dict(net="2d", mode="captured", guard=True),
    "2d_guard_teacher_eager": dict(net="2d", mode="eager", guard=True, teacher=True),
    "2d_guard_teacher_captured": dict(net="2d", mode="captured", guard=True, teacher=True),
    "2d_all_eager": dict(net="2d", mode="eager", **_ALL),
    "2d_all_captured": dict(net="2d", mode="captured", **_ALL),
    "2d_all_bf16_captured": dict(net="2d", mode="captured", bf16=True, **_ALL),
    "3d_all_eager": dict(net="3d", mode="eager", **_ALL),
    "3d_all_captured": dict(net="3d", mode="captured", **_ALL),
    "3d_residual_all_captured": dict(net="3d_res", mode="captured", **_ALL),
    "2d_ablation_all_eager": dict(net="2d", mode="eager", step="ablation", **_ALL),
    "2d_all_c3_captured": dict(net="2d", mode="captured", classes=3, **_ALL),
}
# The recorded step must clip, so that the guarded optimizer takes its scaled path (coef < 1): the global gradient norm of these steps is
# 6 to 150 (2D 12.2, 3D 150.5, ablation 6.5), thousands of times this; tests/test_launch_order_gpu.py asserts 0 < coef < 0.1.
GUARD_MAX_NORM = 1e-3
MONITOR_RING = 8


def opt_entry_points(case):
    """{entry point: launches} that the opt-in features of a case add to one iteration, and `absent`: the optimizer entries they replace."""
    want = {}
    if case.get("guard"):
        want.update(chap_grad_norm=1, chap_sgd_guard_step=1)
    elif case.get("teacher"):
        want["chap_sgd_ema_step"] = 1
    if case.get("monitor"):
        want.update(chap_monitor_accumulate=1, chap_monitor_finalize=1)
        if case.get("step") != "ablation":          # AblationStep has no largest-component filter: no label-map launch
            want["chap_monitor_accumulate_labels"] = 1
    absent = [n for n in ("chap_sgd_step", "chap_sgd_ema_step", "chap_sgd_guard_step", "chap_grad_norm", "chap_monitor_accumulate",
                          "chap_monitor_accumulate_labels", "chap_monitor_finalize") if n not in want]
    return want, absent


_inputs = {}


def _net_inputs(net, classes=None):
    """State, batch, injected randomness and box of tests/test_train_step_gpu.py::test_grouped_decoder_launches_equal_separate_launches
    (made once per process; nothing here changes them).  `classes`: a 2D model of another class count than the default four."""
    key = ("2d" if net == "2d" else "3d") + ("_c%d" % classes if classes else "")
    if key not in _inputs:
        from oracle import init as oinit
        from oracle import train_step as ots
        from tests.iteration_parity import inject_2d, inject_3d, to_dev
        if key.startswith("2d"):
            B, lbs, sp = 8, 4, (64, 64)
            state = oinit.dual_decoder_2d_state(301, n_class=classes) if classes else oinit.dual_decoder_2d_state(301)
            vol, lab = ots.synthetic_batch(1337, lbs, B - lbs, *sp, classes) if classes else ots.synthetic_batch(1337, lbs, B - lbs, *sp)
            inj = to_dev(inject_2d(B - lbs, lbs // 2 + (B - lbs) // 2, sp[0], sp[1], 2), 2)
            inj["drop_F"] = to_dev({"drop_F": oinit.drop_masks_2d(11, B, sp[0], sp[1])}, 2)["drop_F"]      # AblationStep's full-batch pass
            box, extra = (7, 11), ({"num_classes": classes} if classes else {})
        else:
            B, lbs, sp = 4, 2, (16, 32, 16)
            state = oinit.dual_decoder_3d_state(401)
            vol, lab = ots.synthetic_batch_3d(1337, lbs, B - lbs, *sp)
            inj = to_dev(inject_3d(B - lbs, lbs // 2 + (B - lbs) // 2, sp, 2), 3)
            box, extra = (2, 5, 3), {"num_classes": 2}
        _inputs[key] = dict(state=state, vol=vol.to(DEV), lab=lab.to(DEV), inj=inj, box=box, args=dict(dict(labeled_bs=lbs, batch_size=B, vat_iters=2), **extra))
    return _inputs[key]


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pack_entries_of(*models):
    """device pointer of a chap_pack_multi table -> the host-side PackEntry array the executor (of one of `models`) built it from"""
    def find(ptr):
        for model in models:
            for tab in model._exec._packed.values():
                if tab["table"].data_ptr() == int(ptr):
                    return tab["entries"]
        return None
    return find


def _case_step(name):
    """(step, inputs, injected randomness, environment) of one case: the model with the case's state, its training step not yet run."""
    from chap_amd.networks import DualDecoder, DualDecoder3d
    from chap_amd.train import AblationStep, ChapStep
    case = _case(name)
    inp = _net_inputs(case["net"], case.get("classes"))
    classes = case.get("classes") or (4 if case["net"] == "2d" else 2)

    def make():
        if case["net"] == "2d":
            return DualDecoder(1, classes, {"decoder_type": "mcnet"})
        return DualDecoder3d(n_channels=1, n_classes=classes, normalization="batchnorm", has_dropout=True, has_residual=case["net"] == "3d_res")

    m = make().to(DEV).train()
    m.load_state_dict(inp["state"], strict=True)
    if case.get("bf16"):
        m.set_compute_dtype(torch.bfloat16)
    features, extra_args = {}, {}
    if case.get("teacher"):         # as tests/test_mean_teacher_step_gpu.py builds it: weights of its own, of which nothing survives the first step
        from chap_amd.train import build_teacher

        def make_teacher():
            torch.manual_seed(99)
            return make().to(DEV)
        features["teacher"], extra_args["ema_decay"] = build_teacher(make_teacher).eval(), 0.99
    if case.get("guard"):
        from chap_amd.guard import StepGuard
        features["guard"] = StepGuard(max_norm=GUARD_MAX_NORM, skip_nonfinite=True, device=DEV)
    if case.get("monitor"):
        from chap_amd.monitor import StepMonitor
        features["monitor"] = StepMonitor(classes, ring=MONITOR_RING, device=DEV)
    inj = dict(inp["inj"])
    if case.get("fp_inject"):       # no host copies under capture: the scripted draws of the perturbed pass on the device (tests/test_train_step_gpu.py:262-278)
        from oracle import filter_dropout as ofd
        _, scores, uniforms = ofd.fd_inputs(B=inp["vol"].shape[0] - inp["args"]["labeled_bs"])
        inj.update(fp_uniforms=[(a.to(DEV), b.to(DEV)) for a, b in uniforms], sim_score=[sc.to(DEV) for sc in scores])
    with _environ(case.get("env", {})):
        step = (AblationStep if case.get("step") == "ablation" else ChapStep)(m, dict(inp["args"], **extra_args, **case.get("args", {})), **features)
    step.iter_num = 4500
    return step, inp, inj


def _case(name):
    return CASES[name] if name in CASES else OPT_CASES[name]


def record_case(name, rich=False, exact=False):
    """Run one case (of CASES or OPT_CASES) on the GPU and return its full text record; with `rich`, (that record, the rich record) of a
    RichRecorder (`exact`: with the allocator's snapshot read after every allocation and free, _Allocations)."""
    case = _case(name)
    step, inp, inj = _case_step(name)
    with _environ(case.get("env", {})):
        only = case["mode"] == "captured"
        rec = RichRecorder(only, _Allocations(exact), pack_entries=_pack_entries_of(step.model)) if rich else Recorder(only)
        with rec.recording():
            if case["mode"] == "eager":
                step.step(inp["vol"], inp["lab"], box_yx=inp["box"], inject=inj)
            else:
                step.capture(inp["vol"], inp["lab"], warmup=1, inject=inj)
        torch.cuda.synchronize()
    return (rec.text(), rec.rich_text()) if rich else rec.text()


STAGED_REPLAY = "2d_staged_double_replay"       # not in CASES: it has no record of the first kind in tests/golden/issue_order_parent.txt


def record_staged_replays():
    """The rich record of two consecutive replay() calls of the captured 2D step that take their batch from stage() (ChapStep._stage: the
    copy stream and its two events).  A replay is one GR line on its stream whose accesses are the union of what the capture recorded;
    the copies into the staging and the static buffers come from the dispatch mode.  Returns (record of the capture, record of the replays)."""
    step, inp, inj = _case_step("2d_captured")
    cap = RichRecorder(True, pack_entries=_pack_entries_of(step.model))
    with cap.recording():
        step.capture(inp["vol"], inp["lab"], warmup=1, inject=inj)
    torch.cuda.synchronize()
    rec = RichRecorder(False, allocations=cap.allocs, pack_entries=cap.pack_entries, replay_accesses=union_accesses(cap.rich_text()))
    with rec.recording():
        for _ in range(2):
            step.stage(inp["vol"], inp["lab"])
            step.replay(box_yx=inp["box"])
    torch.cuda.synchronize()
    return cap.rich_text(), rec.rich_text()


def _capture_for_replays(name):
    """(step, inputs, recorder of the capture, recorder for what follows it) of a captured case: the second recorder shares the first one's
    allocation map and writes every replay as one GR line with the union of the capture's accesses."""
    step, inp, inj = _case_step(name)
    models = [m for m in (step.model, step.teacher) if m is not None]
    cap = RichRecorder(True, pack_entries=_pack_entries_of(*models))
    with cap.recording():
        step.capture(inp["vol"], inp["lab"], warmup=1, inject=inj)
    torch.cuda.synchronize()
    rec = RichRecorder(False, allocations=cap.allocs, pack_entries=cap.pack_entries, replay_accesses=union_accesses(cap.rich_text()))
    return step, inp, cap, rec


INTERVAL = "2d_all_interval"                    # not in CASES or OPT_CASES: records of what runs between and around replays


def record_interval():
    """The rich record of what train() does around a validation interval (train_ours_2D.py, the loop behind `it % val_interval == 0`) with
    teacher, guard and monitor attached: two replays fed by stage(); then the student evaluated on one 64 x 64 slice, sync_teacher_stats()
    and the teacher evaluated on it -- both read buffers that the captured optimizer launch writes --, StepMonitor.read() and
    StepGuard.read(), each a copy on a stream of its own between two events; then stage() and a third replay, which writes what the
    readers copied.  Returns (record of the capture, record of the replays and the interval)."""
    step, inp, cap, rec = _capture_for_replays("2d_all_captured")
    model, teacher = step.model, step.teacher
    x = inp["vol"][:1].contiguous()
    with rec.recording():
        for _ in range(2):
            step.stage(inp["vol"], inp["lab"])
            step.replay(box_yx=inp["box"])
        with torch.no_grad():
            model.eval()
            model(x)
            step.sync_teacher_stats()
            teacher(x)
            model.train()
        step.monitor.read()
        step.guard.read()
        step.stage(inp["vol"], inp["lab"])
        step.replay(box_yx=inp["box"])
    torch.cuda.synchronize()
    return cap.rich_text(), rec.rich_text()


LOADER_REPLAYS = {"2d_loader_double_replay": "2d_captured", "3d_padded_loader_double_replay": "3d_captured"}


def _synthetic_loader(net):
    """A DeviceLoader over a synthetic store of mixed shapes, as tests/test_augment_gpu.py and tests/test_la_kernels_gpu.py build them (2D:
    twenty slices, some smaller than the output; 3D: six volumes, three of them smaller than some crop, pad=True).  Labels stay inside
    the networks' class counts: these batches are trained on."""
    import numpy as np
    from chap_amd.data import DeviceLoader, SliceStore, VolumeStore
    rng = np.random.default_rng(5)
    if net == "2d":
        shapes = [((256, 216), (216, 256), (224, 154), (37, 29), (96, 88), (80, 72))[i % 6] for i in range(20)]
        store = SliceStore([rng.random(s, dtype=np.float32) + 0.5 for s in shapes], [rng.integers(0, 4, s).astype(np.uint8) for s in shapes], DEV)
        return DeviceLoader(store, range(8), range(8, 20), 8, 4, (64, 64), seed=5)
    shapes = [(20, 30, 12), (40, 40, 36), (24, 24, 24), (10, 50, 30), (44, 44, 44), (33, 35, 31)]
    store = VolumeStore([rng.random(s, dtype=np.float32) + 0.5 for s in shapes], [rng.integers(0, 2, s).astype(np.uint8) for s in shapes], DEV)
    return DeviceLoader(store, range(3), range(3, 6), 4, 2, (16, 32, 16), seed=1, pad=True)


def record_loader_replays(name):
    """The rich record of capture, stage_from(loader), replay, stage_from(loader), replay (ChapStep.stage_from: the loader's augmentation
    kernel fills the staging buffers on the copy stream, beside the running iteration).  Returns (record of the capture, record of the rest)."""
    step, inp, cap, rec = _capture_for_replays(LOADER_REPLAYS[name])
    loader = _synthetic_loader("2d" if name.startswith("2d") else "3d")
    torch.cuda.synchronize()                    # the store's upload is not part of the record
    with rec.recording():
        for _ in range(2):
            step.stage_from(loader)
            step.replay(box_yx=inp["box"])
    torch.cuda.synchronize()
    return cap.rich_text(), rec.rich_text()


BETWEEN_REPLAYS = [STAGED_REPLAY, INTERVAL] + list(LOADER_REPLAYS)


def record_between_replays(name):
    """The rich record of one of BETWEEN_REPLAYS (the part behind the capture)."""
    if name == STAGED_REPLAY:
        return record_staged_replays()[1]
    return record_interval()[1] if name == INTERVAL else record_loader_replays(name)[1]


def write_records(directory, names=None):
    """Every case's full record to `directory`/<case>.txt and the fixture lines to `directory`/summary.txt (returned)."""
    os.makedirs(directory, exist_ok=True)
    out = []
    for name in names or CASES:
        text = record_case(name)
        with open(os.path.join(directory, name + ".txt"), "w") as f:
            f.write(text)
        out.append(summary_line(name, text))
        print(out[-1], flush=True)
    with open(os.path.join(directory, "summary.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return out


def write_rich_records(directory, names=None):
    """Every case's rich record to `directory`/<case>.rich.txt, the staged double replay (STAGED_REPLAY) included when asked for by name
    or when no names are given; tests/golden/launch_order_2d_captured.txt.gz is such a file (2d_captured), gzipped.  `directory`/times.txt
    gets every case's wall time recorded the first way and the rich way, in that order, after one untimed step of each network
    (profiles/launch_order_times.txt)."""
    import time
    os.makedirs(directory, exist_ok=True)
    record_case("2d_eager"), record_case("3d_eager")
    times = []
    for name in names or list(CASES) + [STAGED_REPLAY]:         # (the opt-in cases and the other records between replays: by name)
        t0 = time.time()
        if name not in BETWEEN_REPLAYS:
            record_case(name)
        t1 = time.time()
        rich = record_between_replays(name) if name in BETWEEN_REPLAYS else record_case(name, rich=True)[1]
        t2 = time.time()
        with open(os.path.join(directory, name + ".rich.txt"), "w") as f:
            f.write(rich)
        times.append("%-28s first record %.2f s   rich record %.2f s   %d lines" % (name, t1 - t0, t2 - t1, len(rich.splitlines())))
        print(times[-1], flush=True)
    with open(os.path.join(directory, "times.txt"), "w") as f:
        f.write("\n".join(times) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "--rich":
        write_rich_records(sys.argv[2], sys.argv[3:] or None)
    else:
        write_records(sys.argv[1], sys.argv[2:] or None)
