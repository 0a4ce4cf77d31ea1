"""Happens-before check over one recorded iteration (the rich record of tests/issue_trace.py): which pairs of launches touch the same
bytes, at least one of them writing, with nothing that orders them.  Pure Python over text: no torch, no GPU.

The record, one line each in issue order (`|` separates a line's head from its access list):

    L <entry point> <stream> [g<region> l<lane>] | <field>:<R|W|RW>:<extent> ...      a launch of the library
    T <aten op> <stream> | <a<i>|out<i>>:<R|W>:<extent> ...                           device work torch does itself (copy_, zero_, add_, ...)
    GR <stream> | r<i>:R:<extent> ... w<i>:W:<extent> ...                             a graph replay: the union of what its capture recorded
    GB <stream> g<region> / GN g<region> l<lane> / GE g<region>                       a grouped launch region of the library
    WS <a> <b>      stream a waits for what stream b has been handed so far           ER <event> <stream> / WE <stream> <event>
    HS / SS <stream> / ES <event>      the HOST waits for the device / one stream / an event
    X <text>        a finding of the recorder itself (a pointer in no live allocation, an extent that leaves its allocation)

    extent:  <label>+<offset>:<bytes>                     one range
             <label>+<offset>:<row bytes>x<rows>/<pitch>  rows (a channel slice of a channel-last tensor)

Order.  Launches on one stream follow program order.  `WS a b` puts everything issued on b so far before everything issued on a
afterwards; ER / WE do the same through the event's latest record.  Torch's streams are non-blocking: the default stream gives no edges.
A host wait puts what it waited for before everything the host issues afterwards, on any stream.  Under capture the same lines are graph
edges, so the rules do not change.  A group region issues nothing before its end (chap_group_end): its launches take the stream's order of
the GE line; inside, a lane's launches are ordered and the lanes are mutually unordered (the library issues the j-th launches of all lanes
as one grid, which orders more than that; the check does not lean on it).  Vector clocks, one component per stream; a region's launches share
the clock in front of the region and are seen from outside through the region's last tick.

A finding is a pair of launches whose extents share a byte (exactly: rows against rows, not bounding boxes), one of them W or RW, neither
before the other.  RW against RW counts: there are no float atomics on the training path, an unordered += depends on the order.
"""
from tests.launch_access import bounds, intersects


# ---------------------------------------------------------------------------------------------------------------- the text format
def format_extent(label, offset, ext):
    _, pitch, row_bytes, nrows = ext
    if nrows == 1:
        return "%s+%d:%d" % (label, offset, row_bytes)
    return "%s+%d:%dx%d/%d" % (label, offset, row_bytes, nrows, pitch)


def parse_extent(text):
    """'A3+128:64x16/256' -> ('A3', (128, 256, 64, 16))"""
    where, size = text.split(":")
    label, offset = where.split("+")
    if "x" in size:
        row_bytes, rest = size.split("x")
        nrows, pitch = rest.split("/")
        return label, (int(offset), int(pitch), int(row_bytes), int(nrows))
    return label, (int(offset), 0, int(size), 1)


class Event:
    __slots__ = ("line", "kind", "name", "stream", "region", "lane", "idx", "acc", "clock", "vis")

    def where(self):
        return "line %d: %s %s on %s%s" % (self.line + 1, self.kind, self.name, self.stream,
                                           "" if self.region is None else " g%d l%d" % (self.region, self.lane))


def _parse_accesses(text):
    out = []
    for item in text.split():
        field, mode, ext = item.split(":", 2)
        label, e = parse_extent(ext)
        out.append((field, mode, label, e))
    return out


class Analysis:
    """A record parsed once: its launches and the pairs of them that conflict by memory.  findings(skip) then only walks the ordering lines,
    so the deletion table over a record (every WS / WE line taken out in turn) costs one clock pass per line."""

    def __init__(self, text):
        self.lines = text.splitlines()
        self.events, self.recorder_findings = [], []
        self._by_line = {}
        lane_count = {}
        for n, ln in enumerate(self.lines):
            head, _, acc = ln.partition(" | ")
            f = head.split()
            if not f:
                continue
            if f[0] in ("L", "T", "GR"):
                ev = Event()
                ev.line, ev.kind, ev.region, ev.lane, ev.idx = n, f[0], None, 0, 0
                if f[0] == "GR":
                    ev.name, ev.stream = "graph_replay", f[1]
                else:
                    ev.name, ev.stream = f[1], f[2]
                    if len(f) >= 5:
                        ev.region, ev.lane = int(f[3][1:]), int(f[4][1:])
                        ev.idx = lane_count[(ev.region, ev.lane)] = lane_count.get((ev.region, ev.lane), -1) + 1
                ev.acc = _parse_accesses(acc)
                self._by_line[n] = ev
                self.events.append(ev)
            elif f[0] == "X":
                self.recorder_findings.append(dict(kind="recorder", line=n + 1, text=ln[2:]))
        self.streams = sorted({ev.stream for ev in self.events} | {s for ln in self.lines for s in self._streams_of(ln)})
        self._sidx = {s: i for i, s in enumerate(self.streams)}
        self.pairs, self.same_stream_pairs = self._conflicts()

    @staticmethod
    def _streams_of(ln):
        f = ln.split(" | ")[0].split()
        if not f:
            return ()
        return {"WS": f[1:3], "WE": f[1:2], "ER": f[2:3], "GB": f[1:2], "SS": f[1:2]}.get(f[0], ())

    def _conflicts(self):
        """{(i, j): [(field of i, field of j)]} for events i < j on different streams, or in different lanes of one region, whose extents
        share a byte with a write among them; and the number of such pairs that one stream's program order settles."""
        per_label = {}
        for i, ev in enumerate(self.events):
            for field, mode, label, ext in ev.acc:
                lo, hi = bounds(ext)
                if hi > lo:
                    per_label.setdefault(label, []).append((lo, hi, i, field, mode, ext))
        pairs, same = {}, set()
        for items in per_label.values():
            items.sort(key=lambda t: t[0])
            active = []
            for it in items:
                lo, hi, i, field, mode, ext = it
                active = [a for a in active if a[1] > lo]
                for a in active:
                    if a[2] == i or (mode == "R" and a[4] == "R"):
                        continue
                    x, y = self.events[a[2]], self.events[i]
                    settled = x.stream == y.stream and (x.region is None or x.region != y.region or x.lane == y.lane)
                    key = (a[2], i) if a[2] < i else (i, a[2])
                    if settled and key in same:
                        continue
                    if not intersects(a[5], ext):
                        continue
                    if settled:
                        same.add(key)
                    else:
                        fields = (a[3] + ":" + a[4], field + ":" + mode) if a[2] < i else (field + ":" + mode, a[3] + ":" + a[4])
                        pairs.setdefault(key, []).append(fields)
                active.append(it)
        return pairs, len(same)

    # ------------------------------------------------------------------------------------------------------------ order
    def _clocks(self, skip=None):
        S = len(self.streams)
        clock = [[0] * S for _ in range(S)]
        host, events = [0] * S, {}
        join = lambda a, b: [x if x > y else y for x, y in zip(a, b)]

        def cur(s):
            clock[s] = join(clock[s], host)
            return clock[s]

        region = {}             # region number -> [its launches]
        skip = () if skip is None else (skip,) if isinstance(skip, int) else skip
        for n, ln in enumerate(self.lines):
            if n in skip:
                continue
            ev = self._by_line.get(n)
            if ev is not None:
                if ev.region is not None and ev.region in region:
                    region[ev.region].append(ev)
                    continue
                s = self._sidx[ev.stream]
                c = cur(s)
                c[s] += 1
                ev.clock, ev.vis = tuple(c), c[s]
                continue
            f = ln.split()
            if not f:
                continue
            k = f[0]
            if k == "WS":
                a, b = self._sidx[f[1]], self._sidx[f[2]]
                clock[a] = join(cur(a), cur(b))
            elif k == "ER":
                events[f[1]] = tuple(cur(self._sidx[f[2]]))
            elif k == "WE":
                if f[2] in events:
                    a = self._sidx[f[1]]
                    clock[a] = join(cur(a), events[f[2]])
            elif k == "GB":
                region[int(f[2][1:])] = []
            elif k == "GE":
                evs = region.pop(int(f[1][1:]), [])
                if evs:
                    s = self._sidx[evs[0].stream]
                    c = cur(s)
                    before = tuple(c)
                    c[s] += len(evs)
                    for e in evs:
                        e.clock, e.vis = before, c[s]
            elif k == "HS":
                for s in range(S):
                    host = join(host, clock[s])
            elif k == "SS":
                host = join(host, clock[self._sidx[f[1]]])
            elif k == "ES":
                if f[1] in events:
                    host = join(host, events[f[1]])

    def _before(self, a, b):
        if a.region is not None and a.region == b.region:
            return a.lane == b.lane and a.idx < b.idx
        return b.clock[self._sidx[a.stream]] >= a.vis

    def findings(self, skip=None):
        """The unordered conflicting pairs of the record (with the line or lines `skip`, 0-based, taken out), plus the recorder's own findings."""
        self._clocks(skip)
        out = list(self.recorder_findings)
        for (i, j), fields in self.pairs.items():
            a, b = self.events[i], self.events[j]
            if not self._before(a, b) and not self._before(b, a):
                out.append(dict(kind="race", a=a.where(), b=b.where(), lines=(a.line + 1, b.line + 1), fields=fields[:4],
                                text="%s  <->  %s  fields %s" % (a.where(), b.where(), fields[:4])))
        return out

    def counts(self):
        return dict(launches=sum(e.kind == "L" for e in self.events), torch_ops=sum(e.kind == "T" for e in self.events),
                    replays=sum(e.kind == "GR" for e in self.events), streams=len(self.streams),
                    ordered_conflicts=len(self.pairs) + self.same_stream_pairs)


def analyze(text):
    """record -> list of findings (dicts with `kind`, `text`, ...)."""
    return Analysis(text).findings()


def join_table(text):
    """[(line number (1-based), line, 'necessary' | 'implied', findings without it)] for every join of the record: a join is necessary when
    the record without it has a finding that the full record lacks, implied when other edges still order everything.  A join is a WS or a
    WE line.  torch's Stream.wait_stream records an event on the other stream and waits for it, so the recorder, which patches all three,
    writes `WS a b`, `ER e b`, `WE a e` for ONE wait: such a triple is taken out as a whole and listed under its WS line (its WE line
    alone would always be implied by the WS line, and the other way round)."""
    an = Analysis(text)
    base = len(an.findings())
    out, n, lines = [], 0, an.lines
    while n < len(lines):
        f = lines[n].split()
        unit = None
        if f and f[0] == "WS":
            unit = (n,)
            if n + 2 < len(lines):
                g, h = lines[n + 1].split(), lines[n + 2].split()
                if g[:1] == ["ER"] and h[:1] == ["WE"] and g[2] == f[2] and h[1] == f[1] and h[2] == g[1]:
                    unit = (n, n + 1, n + 2)
        elif f and f[0] == "WE":
            unit = (n,)
        if unit is not None:
            extra = len(an.findings(skip=unit)) - base
            out.append((n + 1, lines[n], "necessary" if extra > 0 else "implied", extra))
            n = unit[-1]
        n += 1
    return out


def read_record(path):
    import gzip
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return f.read()


if __name__ == "__main__":          # python -m tests.launch_order RECORD: the record's counts, findings and join table (profiles/launch_order_joins.txt)
    import sys
    text = read_record(sys.argv[1])
    an = Analysis(text)
    found = an.findings()
    print("# %s: %s, %d findings" % (sys.argv[1], " ".join("%s=%d" % kv for kv in an.counts().items()), len(found)))
    for f in found:
        print("# finding:", f["text"])
    print("# line  join         without it   findings without it")
    for n, ln, kind, extra in join_table(text):
        print("%6d  %-11s  %-10s  %d" % (n, ln, kind, extra))
