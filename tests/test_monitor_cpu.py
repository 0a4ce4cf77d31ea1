"""Host side of the training monitor (no GPU): the fp64 restatement of a row (tests/monitor_ref.py) against a plain numpy restatement of
acc_conf_analysis (train_ours_2D.py:152-193), StepMonitor.derive on hand-made rows, the ring bookkeeping of StepMonitor.read() on a host
tensor, the header include/chap_hip_monitor.h against the binding table _lib._SIGS_MONITOR, the struct sizes, and the argument checks of
the three entry points (which return before anything is launched)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from chap_amd import _lib, ops
from chap_amd.monitor import StepMonitor, csv_lines, row_fields, split_rows
from tests import monitor_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chap_hip.h")
EXT_HEADER = os.path.join(ROOT, "include", "chap_hip_ext.h")
MON_HEADER = os.path.join(ROOT, "include", "chap_hip_monitor.h")
ENTRIES = ["chap_monitor_accumulate", "chap_monitor_accumulate_labels", "chap_monitor_finalize"]


def _declared(path):
    """tests/test_abi_cpu.py::_declared_functions on another header."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const char\*)\s+(chap_[a-z0-9_]+)\s*\(", src)))


# ---------------------------------------------------------------------------------------------- the restatement
def test_restatement_matches_acc_conf_analysis():
    """A random 4-class batch, labeled_bs 2 of 4: the six numbers of acc_conf_analysis from derive(row_ref) within 1e-12 of the numpy
    restatement on the soft-max outputs.  Group 0 is the labelled half, group 1 the unlabelled one."""
    rng = np.random.default_rng(11)
    N, C, H, W, lbs = 4, 4, 12, 10, 2
    logits = mr.quantised_logits(rng, (N, C, H, W))
    label = rng.integers(0, C, (N, H, W))
    z = logits.astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    prob = e / e.sum(1, keepdims=True)
    want = mr.acc_conf_numpy(prob, label, lbs)
    d = StepMonitor.derive(mr.stack_rows([mr.row_ref(logits, logits, label, lbs)]))
    got = []
    for g in (0, 1):
        got += [d["avg_dice"][0, g, 0], d["corr_conf"][0, g, 0], d["err_conf"][0, g, 0]]
    assert len(want) == len(got) == 6
    for w, g_ in zip(want, got):
        assert abs(w - g_) <= 1e-12, (want, got)
    assert (d["disagree"] == 0).all()                      # the same head twice
    assert (d["avg_dice"][..., 0] == d["avg_dice"][..., 1]).all()


def test_restatement_out_of_range_labels_and_split():
    rng = np.random.default_rng(5)
    N, C, P = 3, 3, 40
    l1, l2 = mr.quantised_logits(rng, (N, C, P)), mr.quantised_logits(rng, (N, C, P))
    label = rng.integers(0, C, (N, P))
    label[0, :7], label[2, 5:9] = 255, C
    for n_first in (0, 1, N):
        r = mr.row_ref(l1, l2, label, n_first)
        assert r["n"].tolist() == [n_first * P, (N - n_first) * P]
        assert r["gt"].sum() == N * P - 11                 # the eleven labels outside [0, C) are in no gt[c] ...
        a1 = l1.argmax(1)
        assert r["n_correct"][:, 0].sum() == (a1 == label).sum()         # ... and never correct
        assert (r["pred"].sum(-1) == r["n"][:, None]).all()
        assert np.allclose(r["conf_correct"] + r["conf_err"], [[(1 / np.exp(l.astype(np.float64) - l.max(1, keepdims=True)).sum(1))[sl].sum()
                                                                for l in (l1, l2)] for sl in (slice(0, n_first), slice(n_first, N))], rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------- derive
def test_derive_on_hand_made_rows():
    C = 3
    r = {k: np.zeros(s) for k, s in (("n", (1, 2)), ("n_disagree", (1, 2)), ("gt", (1, 2, C)), ("n_correct", (1, 2, 2)), ("conf_correct", (1, 2, 2)),
                                     ("conf_err", (1, 2, 2)), ("inter", (1, 2, 2, C)), ("pred", (1, 2, 2, C)), ("inter_f", (1, 2, 2, C)), ("pred_f", (1, 2, 2, C)))}
    r["iteration"] = np.array([7])
    r["scalars"] = np.arange(16, dtype=np.float64)[None] * 0.5
    # group 1: 100 pixels, class 2 absent from the labels AND from head 0's prediction (an empty class: Dice 0), predicted by head 1 only
    r["n"][0, 1], r["n_disagree"][0, 1] = 100, 25
    r["gt"][0, 1] = [60, 40, 0]
    r["n_correct"][0, 1] = [80, 50]
    r["conf_correct"][0, 1], r["conf_err"][0, 1] = [72.0, 30.0], [10.0, 20.0]
    r["pred"][0, 1, 0], r["inter"][0, 1, 0] = [70, 30, 0], [55, 25, 0]
    r["pred"][0, 1, 1], r["inter"][0, 1, 1] = [50, 30, 20], [35, 15, 0]
    r["pred_f"][0, 1, 0], r["inter_f"][0, 1, 0] = [75, 25, 0], [58, 24, 0]
    d = StepMonitor.derive(r)
    assert d["iteration"].tolist() == [7]
    assert d["accuracy"][0, 1].tolist() == [0.8, 0.5] and d["accuracy"][0, 0].tolist() == [0.0, 0.0]      # the empty group: 0, not NaN
    assert d["corr_conf"][0, 1, 0] == 72.0 / (80 + 1e-6) and d["err_conf"][0, 1, 0] == 10.0 / (20 + 1e-6)
    assert d["corr_conf"][0, 0, 0] == 0.0 and d["err_conf"][0, 0, 1] == 0.0
    assert d["dice"][0, 1, 0].tolist() == [2 * 55 / 130, 2 * 25 / 70, 0.0]             # class 2: 0 / 0 -> 0 (medpy's dc)
    assert d["dice"][0, 1, 1].tolist() == [2 * 35 / 110, 2 * 15 / 70, 0.0]             # predicted, absent from the labels: 0 / 20
    assert d["avg_dice"][0, 1, 0] == (2 * 25 / 70 + 0.0) / 2                           # the mean over classes 1..C-1
    assert d["avg_dice_f"][0, 1, 0] == (2 * 24 / 65 + 0.0) / 2 and d["avg_dice_f"][0, 1, 1] == 0.0
    assert d["disagree"][0].tolist() == [0.0, 0.25]
    s = r["scalars"][0]
    assert d["loss_l"][0] == s[1] + s[4] + s[6] + s[9] and d["loss_u"][0] == s[0] + s[3] + s[7] + s[10] and d["vat_loss"][0] == s[12]
    r["scalar_layout"] = "ablation"
    d = StepMonitor.derive(r)
    assert d["loss_l"][0] == s[0] + s[1] and d["loss_u"][0] == s[2] + s[3] and d["vat_loss"][0] == s[4]
    line, = csv_lines(d)
    assert line.split(",")[0] == "7" and len(line.split(",")) == 15 and float(line.split(",")[4]) == 0.25


def test_row_layout_is_the_headers():
    for C in ops.LOSS_CLASSES:
        f = row_fields(C)
        assert ops.monitor_row_words(C) == 33 + 18 * C
        assert f["n"][0] == 1 and f["gt"][0] == 3 and f["conf_correct"][0] == 1 + 4 + C and f["pred"][0] == 1 + 8 + 3 * C
        assert f["inter_f"][0] == 1 + 2 * (8 + 5 * C) and f["scalars"][0] == ops.monitor_row_words(C) - 16
        mat = np.arange(2 * ops.monitor_row_words(C), dtype=np.float64).reshape(2, -1)
        rows = split_rows(mat, C)
        seen = np.concatenate([rows[k].reshape(2, -1) for k in f], 1)
        assert sorted(seen[0].tolist()) == mat[0].tolist()            # every word of a row is named exactly once
        assert rows["gt"][1, 1, 0] == mat[1, 1 + (8 + 5 * C) + 2]


# ---------------------------------------------------------------------------------------------- ring bookkeeping
def _write(mon, iteration):
    """What the finalize kernel does to the ring, on the host: row `slot % R` stamped with the iteration."""
    row = mon.ring[mon.next_slot() % mon.R]
    row.zero_()
    row[0] = iteration
    row[1] = 1000 + iteration                       # n of group 0: tells the rows apart
    mon.advance()


def test_ring_wrap_order_and_dropped():
    mon = StepMonitor(4, ring=4, device="cpu")
    assert mon.ws is None and mon.ring.shape == (4, ops.monitor_row_words(4))
    r = mon.read()
    assert len(r["iteration"]) == 0 and r["dropped"] == 0
    for it in (1, 2, 3):
        _write(mon, it)
    r = mon.read()
    assert r["iteration"].tolist() == [1, 2, 3] and r["n"][:, 0].tolist() == [1001, 1002, 1003] and r["dropped"] == 0
    assert len(mon.read()["iteration"]) == 0                   # nothing twice
    for it in (4, 5, 6):                                      # wraps: slots 3, 0, 1
        _write(mon, it)
    r = mon.read()
    assert r["iteration"].tolist() == [4, 5, 6] and r["dropped"] == 0 and r["n"][:, 0].tolist() == [1004, 1005, 1006]
    for it in range(7, 18):                                   # eleven rows into four slots, no read in between
        _write(mon, it)
    r = mon.read()
    assert r["iteration"].tolist() == [14, 15, 16, 17] and r["dropped"] == 7 and mon.dropped == 7
    assert mon.count == 17 and mon.last_iteration == 17
    snap = mon.snapshot()
    _write(mon, 18)
    mon.restore(snap)                                         # (capture()'s warm-up: the row and the slot are taken back)
    assert mon.count == 17 and len(mon.read()["iteration"]) == 0
    with pytest.raises(ValueError, match="2..8 built"):
        StepMonitor(9, device="cpu")


# ---------------------------------------------------------------------------------------------- header, binding, structs
def test_header_and_binding_table_are_in_step():
    src = open(MON_HEADER).read()
    assert _declared(MON_HEADER) == sorted(_lib._SIGS_MONITOR) == ENTRIES              # every declared entry is bound and vice versa
    others = set(_lib._SIGS) | set(_lib._SIGS_EXT) | set(_lib._SIZE_FNS)
    assert not set(_lib._SIGS_MONITOR) & others
    assert not set(ENTRIES) & (set(_declared(HEADER)) | set(_declared(EXT_HEADER)))
    assert "chap_hip_monitor.h" not in open(HEADER).read() and re.search(r'^#include "chap_hip\.h"$', src, flags=re.M)
    assert re.search(r"#define\s+CHAP_ABI_VERSION\s+9\b", open(HEADER).read())
    for cite in ("train_ours_2D.py:152-193", "train_ours_2D.py:404-405", "train_ablation_2D.py:180-190"):
        assert cite in src
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in ENTRIES) and lib.chap_abi_version() == _lib.ABI_VERSION == 9
    for n in ENTRIES:
        fn = _lib._fn(n)
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(_lib._SIGS_MONITOR[n])


def test_ctypes_struct_size_matches_header(tmp_path):
    pairs = {"chap_monitor_params": _lib.MonitorParams, "chap_monitor_labels_params": _lib.MonitorLabelsParams,
             "chap_monitor_finalize_params": _lib.MonitorFinalizeParams}
    c = tmp_path / "sz.c"
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in pairs)
    body += 'printf("n_first %zu\\nscalars %zu\\nhas_labels %zu\\n", offsetof(chap_monitor_params, n_first), offsetof(chap_monitor_finalize_params, scalars), offsetof(chap_monitor_finalize_params, has_labels));\n'
    body += "".join('printf("row%d %%d\\nws%d %%d\\nlab%d %%d\\n", CHAP_MONITOR_ROW_WORDS(%d), CHAP_MONITOR_WS_WORDS(%d), CHAP_MONITOR_LABEL_REGION(%d));\n' % (C, C, C, C, C, C)
                    for C in ops.LOSS_CLASSES)
    body += 'printf("slots %d\\nmaxs %d\\nhdr %d\\n", CHAP_MONITOR_SLOTS, CHAP_MONITOR_MAX_SCALARS, CHAP_MONITOR_HDR);\n'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip_monitor.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    v = {k: int(x) for k, x in (line.split() for line in out.strip().splitlines())}
    for name, st in pairs.items():
        assert v[name] == ctypes.sizeof(st), (name, v[name], ctypes.sizeof(st))
    assert v["n_first"] == _lib.MonitorParams.n_first.offset and v["scalars"] == _lib.MonitorFinalizeParams.scalars.offset
    assert v["has_labels"] == _lib.MonitorFinalizeParams.has_labels.offset
    assert (v["slots"], v["maxs"], v["hdr"]) == (_lib.MONITOR_SLOTS, _lib.MONITOR_MAX_SCALARS, _lib.MONITOR_HDR)
    for C in ops.LOSS_CLASSES:
        assert (v["row%d" % C], v["ws%d" % C], v["lab%d" % C]) == (ops.monitor_row_words(C), ops.monitor_ws_words(C), ops.monitor_label_region(C))


# ---------------------------------------------------------------------------------------------- argument checks
def _acc(**over):
    """Made-up, aligned, non-null addresses: every check below fails before a launch, nothing is dereferenced."""
    v = dict(l0=0x10000, l1=0x20000, labels=0x30000, ws=0x40000, N=4, C=4, P=64, n_first=2)
    v.update(over)
    q = _lib.MonitorParams()
    q.logits[0], q.logits[1], q.labels, q.ws = v["l0"], v["l1"], v["labels"], v["ws"]
    q.N, q.C, q.P, q.n_first = v["N"], v["C"], v["P"], v["n_first"]
    return q


def _lab(**over):
    v = dict(m0=0x10000, m1=0x20000, labels=0x30000, ws=0x40000, N=4, C=4, P=64, n_first=0)
    v.update(over)
    q = _lib.MonitorLabelsParams()
    q.maps[0], q.maps[1], q.labels, q.ws = v["m0"], v["m1"], v["labels"], v["ws"]
    q.N, q.C, q.P, q.n_first = v["N"], v["C"], v["P"], v["n_first"]
    return q


def _fin(**over):
    v = dict(ws=0x40000, ring=0x50000, slot_iter=0x60000, C=4, ring_rows=8, nscalars=2, has_labels=1, s0=0x70000, s1=0x70004)
    v.update(over)
    q = _lib.MonitorFinalizeParams()
    q.ws, q.ring, q.slot_iter = v["ws"], v["ring"], v["slot_iter"]
    q.scalars[0], q.scalars[1] = v["s0"], v["s1"]
    q.C, q.ring_rows, q.nscalars, q.has_labels = v["C"], v["ring_rows"], v["nscalars"], v["has_labels"]
    return q


@pytest.mark.parametrize("entry,params,match", [
    ("chap_monitor_accumulate", _acc(l1=0), "chap_monitor_accumulate: null argument"),
    ("chap_monitor_accumulate", _acc(ws=0), "chap_monitor_accumulate: null argument"),
    ("chap_monitor_accumulate", _acc(C=9), r"chap_monitor_accumulate: C=9 \(2..8 built\)"),
    ("chap_monitor_accumulate", _acc(C=1), r"chap_monitor_accumulate: C=1 \(2..8 built\)"),
    ("chap_monitor_accumulate", _acc(n_first=5), "chap_monitor_accumulate: bad shape"),
    ("chap_monitor_accumulate", _acc(N=65536, P=65536), "chap_monitor_accumulate: N\\*P=4294967296 exceeds the 32-bit pixel index"),
    ("chap_monitor_accumulate", _acc(labels=0x30004), "chap_monitor_accumulate: logits must be 4-byte, labels and ws 8-byte aligned"),
    ("chap_monitor_accumulate", _acc(l0=0x10002), "chap_monitor_accumulate: logits must be 4-byte"),
    ("chap_monitor_accumulate_labels", _lab(m0=0), "chap_monitor_accumulate_labels: null argument"),
    ("chap_monitor_accumulate_labels", _lab(C=0), r"chap_monitor_accumulate_labels: C=0 \(2..8 built\)"),
    ("chap_monitor_accumulate_labels", _lab(N=0), "chap_monitor_accumulate_labels: bad shape"),
    ("chap_monitor_accumulate_labels", _lab(N=32768, P=131072), "chap_monitor_accumulate_labels: N\\*P=4294967296 exceeds"),
    ("chap_monitor_accumulate_labels", _lab(m1=0x20004), "chap_monitor_accumulate_labels: maps, labels and ws must be 8-byte aligned"),
    ("chap_monitor_finalize", _fin(ring=0), "chap_monitor_finalize: null argument"),
    ("chap_monitor_finalize", _fin(slot_iter=0), "chap_monitor_finalize: null argument"),
    ("chap_monitor_finalize", _fin(C=16), r"chap_monitor_finalize: C=16 \(2..8 built\)"),
    ("chap_monitor_finalize", _fin(ring_rows=0), "chap_monitor_finalize: bad argument"),
    ("chap_monitor_finalize", _fin(nscalars=17), "chap_monitor_finalize: bad argument"),
    ("chap_monitor_finalize", _fin(s1=0), "chap_monitor_finalize: null scalar 1"),
    ("chap_monitor_finalize", _fin(ring=0x50004), "chap_monitor_finalize: ws and ring must be 8-byte"),
    ("chap_monitor_finalize", _fin(s0=0x70002), "chap_monitor_finalize: ws and ring must be 8-byte, slot_iter and scalars 4-byte aligned"),
])
def test_argument_checks_refuse_by_name(entry, params, match):
    with pytest.raises(_lib.ChapError, match=match):
        _lib.call(entry, params, 0)


# ---------------------------------------------------------------------------------------------- off by default
def test_train_entries_default_to_no_monitor():
    from chap_amd import train, train_ours_2D, train_ours_3D
    assert train_ours_2D.FLAG_DEFAULTS["monitor"] is False and train_ours_3D.FLAG_DEFAULTS["monitor"] is False
    import inspect
    assert inspect.signature(train.ChapStep.__init__).parameters["monitor"].default is None
