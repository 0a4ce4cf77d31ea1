"""The merging of recorded launches (chap_amd/csrc/launch.cpp: same_launch, the grp[] fill, the used[] walk, the error paths) against a plain model of
the contract written in include/chap_hip.h, on the host: tests/group_probe.py builds launch.cpp into a stand-alone program with the host sanitizers and a
fake `merged` callback; nothing here touches a device.

The contract (chap_hip.h, chap_group_end): issue is position-major (the j-th launch of every lane before any (j + 1)-th); within a position the first
lane not yet issued takes with it every later lane whose (kernel, LDS bytes, grid, block) are the same, up to CHAP_MAX_LANES = 4 lanes in one grid; what
is left follows the same way, in lane order."""
import random

import pytest

from tests.group_probe import ARG_BYTES, MAX_LANES, probe      # noqa: F401 (fixture)

STREAM = 7


def L(fn=1, g=(3, 2, 1), b=256, lds=0):
    return dict(fn=fn, g=tuple(g), b=b, lds=lds)


def key(it):
    return (it["fn"], it["lds"], it["g"], it["b"])


def model(lanes):
    """the contract, restated: lanes = [[launch, ...], ...] -> [[(lane, position), ...] per grid]"""
    grids = []
    for j in range(max((len(l) for l in lanes), default=0)):
        items = [(i, j) for i, l in enumerate(lanes) if j < len(l)]
        used = set()
        for a in items:
            if a in used:
                continue
            grp = [a]
            for b in items[items.index(a) + 1:]:
                if len(grp) < MAX_LANES and b not in used and key(lanes[b[0]][b[1]]) == key(lanes[a[0]][a[1]]):
                    grp.append(b)
            used.update(grp)
            grids.append(grp)
    return grids


def checksum(ident):
    h = 2166136261
    for i in range(ARG_BYTES):
        h = ((h ^ ((ident * 131 + i * 7 + (ident >> 3)) & 255)) * 16777619) & 0xFFFFFFFF
    return h


def ident(table, lane, pos):
    return 1000 * table + 10 * lane + pos + 1                 # <= 9 lanes, <= 6 positions


def rec_line(idt, it, stream=STREAM, op="rec"):
    return "%s %d %d %d %d %d %d %d %d" % (op, idt, it["fn"], it["g"][0], it["g"][1], it["g"][2], it["b"], it["lds"], stream)


def script(t, lanes):
    out = ["begin %d" % STREAM]
    for i, l in enumerate(lanes):
        if i:
            out.append("lane")
        out += [rec_line(ident(t, i, j), it) for j, it in enumerate(l)]
    return out + ["end"]


def parse_grid(line):
    assert line.startswith("grid "), line
    f = dict(tok.split("=") for tok in line.split()[1:])
    items = [tuple(map(int, x.split(":"))) for x in f["items"].split(",")]
    return dict(n=int(f["n"]), stream=int(f["stream"]), fn=int(f["fn"]), g=tuple(map(int, f["g"].split(","))), b=int(f["b"]), lds=int(f["lds"]), items=items)


def run_tables(probe, tables):
    """all tables through ONE process, region after region; returns [(grids, rc) per table]"""
    req = [line for t, lanes in enumerate(tables) for line in script(t, lanes)]
    out = iter(probe(req))
    res = []
    for t, lanes in enumerate(tables):
        assert next(out) == "rc 0"                            # begin
        for i, l in enumerate(lanes):
            for _ in range(len(l) + (1 if i else 0)):
                assert next(out) == "rc 0"                    # lane / rec: recorded, nothing issued
        grids = []
        for line in out:
            if line.startswith("rc "):
                res.append((grids, int(line.split()[1])))
                break
            grids.append(parse_grid(line))
    assert len(res) == len(tables) and next(out, None) is None
    return res


def check_table(t, lanes, grids, rc):
    want = model(lanes)
    assert rc == len(grids) == len(want), (t, rc, len(grids), len(want))                        # the return value is the number of grids
    got_ids = [i for g in grids for i, _ in g["items"]]
    all_ids = sorted(ident(t, i, j) for i, l in enumerate(lanes) for j in range(len(l)))
    assert sorted(got_ids) == all_ids, (t, "not every launch exactly once")
    order = {idt: k for k, g in enumerate(grids) for idt, _ in g["items"]}
    for i, l in enumerate(lanes):                                                             # order within a lane
        ks = [order[ident(t, i, j)] for j in range(len(l))]
        assert ks == sorted(ks) and len(set(ks)) == len(ks), (t, i, ks)
    for g, w in zip(grids, want):
        assert 1 <= g["n"] == len(g["items"]) <= MAX_LANES, (t, g)
        assert [i for i, _ in g["items"]] == [ident(t, i, j) for i, j in w], (t, g, w)          # the model's grid, items in lane order
        assert all(c == checksum(i) for i, c in g["items"]), (t, "argument bytes changed", g)
        first = lanes[w[0][0]][w[0][1]]
        assert (g["fn"], g["lds"], g["g"], g["b"], g["stream"]) == (first["fn"], first["lds"], first["g"], first["b"], STREAM), (t, g)
        assert all(key(lanes[i][j]) == key(first) for i, j in w)


A, B = L(1), L(2)
HAND = {
    "one_lane": [[A, B, A]],
    "four_matching": [[A, B]] * 4,
    "five_matching": [[A]] * 5,
    "nine_matching": [[A, B]] * 9,
    "aba": [[A], [B], [A]],
    "ababa": [[A, A], [B, B], [A, A], [B, B], [A, A]],
    "empty_middle_lane": [[A, B], [], [A, B]],
    "empty_first_lane": [[], [A], [A]],
    "unequal_lengths": [[A, B, A], [A], [A, B]],
    "differ_in_grid_z": [[L(g=(3, 2, 1))], [L(g=(3, 2, 2))], [L(g=(3, 2, 1))]],
    "differ_in_grid_x": [[L(g=(3, 2, 1))], [L(g=(4, 2, 1))]],
    "differ_in_grid_y": [[L(g=(3, 2, 1))], [L(g=(3, 1, 1))]],
    "differ_in_lds": [[L(lds=0)], [L(lds=1024)], [L(lds=0)]],
    "differ_in_block_x": [[L(b=256)], [L(b=64)], [L(b=256)]],
    "nothing_recorded": [[], []],
}
HAND_GRIDS = {"one_lane": 3, "four_matching": 2, "five_matching": 2, "nine_matching": 6, "aba": 2, "ababa": 4, "empty_middle_lane": 2, "empty_first_lane": 1,
              "unequal_lengths": 3, "differ_in_grid_z": 2, "differ_in_grid_x": 2, "differ_in_grid_y": 2, "differ_in_lds": 2, "differ_in_block_x": 2,
              "nothing_recorded": 0}


def test_model_on_the_hand_written_tables():
    """the model itself, against grid counts worked out by hand (and the shapes the header's wording is about)"""
    for name, lanes in HAND.items():
        assert len(model(lanes)) == HAND_GRIDS[name], name
    assert model(HAND["aba"]) == [[(0, 0), (2, 0)], [(1, 0)]]                      # the second A goes with the first, BEFORE B
    assert model(HAND["five_matching"]) == [[(0, 0), (1, 0), (2, 0), (3, 0)], [(4, 0)]]
    assert [len(g) for g in model(HAND["nine_matching"])] == [4, 4, 1] * 2
    assert model(HAND["ababa"])[:2] == [[(0, 0), (2, 0), (4, 0)], [(1, 0), (3, 0)]]


def test_hand_written_tables(probe):
    names = list(HAND)
    for (name, (grids, rc)), t in zip(zip(names, run_tables(probe, [HAND[n] for n in names])), range(len(names))):
        check_table(t, HAND[name], grids, rc)
        assert rc == HAND_GRIDS[name], name


def random_tables(n=400, seed=20251):
    rnd = random.Random(seed)
    kinds = [L(fn, g, b, lds) for fn in (1, 2, 3) for g in ((5, 1, 1), (5, 1, 3)) for lds in (0, 4096) for b in (256, 64)]
    tables = []
    for _ in range(n):
        few = rnd.sample(kinds, rnd.choice((1, 2, 3, len(kinds))))                  # mostly few distinct launches: merges happen
        tables.append([[rnd.choice(few) for _ in range(rnd.randint(0, 5))] for _ in range(rnd.randint(1, 9))])
    return tables


def test_random_tables(probe):
    tables = random_tables()
    res = run_tables(probe, tables)
    merged = 0
    for t, (lanes, (grids, rc)) in enumerate(zip(tables, res)):
        check_table(t, lanes, grids, rc)
        merged += sum(g["n"] > 1 for g in grids)
    assert merged > len(tables)                                                      # the tables do exercise merging
    assert any(len(l) > MAX_LANES for l in tables) and any(g["n"] == MAX_LANES for grids, _ in res for g in grids)


def test_record_on_another_stream_fails_the_region(probe):
    out = probe(["begin 7", rec_line(1, A), "lane", rec_line(2, A, stream=8), rec_line(3, A), "end", "recording",
                 "begin 7", rec_line(4, A), "end"])
    assert out[:5] == ["rc 0", "rc 0", "rc 0", "rc -1", "rc 0"]                      # CHAP_EINVAL = -1 from the record itself
    assert out[5].startswith("rc -1 ") and "another stream" in out[5]                # ... and from chap_group_end, which issued nothing
    assert out[6] == "recording 0"
    assert out[7:9] == ["rc 0", "rc 0"] and parse_grid(out[9])["items"] == [(4, checksum(4))] and out[10] == "rc 1"      # the next region is clean


def test_failing_callback_stops_the_issue(probe):
    lanes = [[A, B, A], [B, A, A]]                                                    # 5 grids: A | B | B | A | AA
    assert len(model(lanes)) == 5
    for k in range(5):
        out = probe(["failat %d -5" % k] + script(0, lanes) + ["recording", "begin 7", rec_line(9, A), "end"])
        body = out[1 + 1 + 6 + 1:]
        grids = [l for l in body if l.startswith("grid")]
        i_rc = next(i for i, l in enumerate(body) if l.startswith("rc "))
        assert i_rc == k + 1, (k, body)                                              # grid k was the last one handed over
        assert body[i_rc].split()[:2] == ["rc", "-5"]
        assert [parse_grid(g)["items"][0][0] for g in grids[:k + 1]] == [ident(0, *w[0]) for w in model(lanes)[:k + 1]]
        assert body[i_rc + 1] == "recording 0"                                       # the region is left
        assert body[i_rc + 2:i_rc + 4] == ["rc 0", "rc 0"] and body[-1] == "rc 1"    # and the next one starts empty: one grid, its own


def test_cancel_issues_nothing(probe):
    out = probe(["begin 7", rec_line(1, A), "lane", rec_line(2, A), "cancel", "recording", "end", "cancel", "lane", rec_line(3, B, stream=5)])
    assert out[:6] == ["rc 0", "rc 0", "rc 0", "rc 0", "rc 0", "recording 0"]
    assert out[6].startswith("rc -1") and out[7] == "rc -1" and out[8] == "rc -1"    # end / cancel / next_lane outside a region: CHAP_EINVAL
    assert parse_grid(out[9])["items"] == [(3, checksum(3))] and out[10] == "rc 0"   # not recording: a launch goes straight through
    assert not any(l.startswith("grid") for l in out[:9])


def test_regions_do_not_nest(probe):
    out = probe(["begin 7", rec_line(1, A), "begin 7", "end"])
    assert out[:3] == ["rc 0", "rc 0", "rc -1"]
    assert parse_grid(out[3])["items"] == [(1, checksum(1))] and out[4] == "rc 1"    # the failed begin left the open region as it was


def test_recording_is_per_thread(probe):
    out = probe(["begin 7", rec_line(1, A), rec_line(2, B, stream=9, op="trec"), "recording", "end"])
    assert out[:2] == ["rc 0", "rc 0"]
    assert out[2] == "thread recording=0"
    g = parse_grid(out[3])                                                            # the other thread's launch was issued at once, on its own stream
    assert g["items"] == [(2, checksum(2))] and g["stream"] == 9 and g["n"] == 1 and out[4] == "rc 0"
    assert out[5] == "recording 1"
    assert parse_grid(out[6])["items"] == [(1, checksum(1))] and out[7] == "rc 1"
