"""The training monitor's kernels against the fp64 restatement of a row (tests/monitor_ref.py): chap_monitor_accumulate on the scalar path
(4 x C x 17 x 19), the 16-byte path (4 x C x 16 x 20) and volumes (2 x C x 5 x 9 x 13) for C in 2, 3, 4, 8, and once where a thread takes a
second grid-stride trip (3 x 4 x 420 x 420), each with the split n_first in {0, 2, N}; chap_monitor_accumulate_labels on ops.largest_cc's
outputs; chap_monitor_finalize into a framed ring.  Labels equal to C and to 255, exact logit ties between class 0 and C - 1, NaN canaries
behind the workspace rows in use and around the ring, nonzero neighbouring ring slots that must come back untouched.  Counts are exact, also
against ops.pseudo_block's own arg-max maps; confidence sums within monitor_ref's bound; two calls give bitwise-equal rows.  One JSON line
per case (worst |err| / bound; `-s` shows them): profiles/monitor_kernels.jsonl is a copy of those lines."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chap_amd import _lib, ops
from chap_amd.monitor import split_rows
from tests import monitor_ref as mr

DEV = torch.device("cuda", 0)
NAN_WORD = torch.tensor([float("nan")], dtype=torch.float64).view(torch.int64).item()
R = 4                                   # ring rows handed to the kernel; one framing row in front and one behind

SHAPES = [(4, 17, 19), (4, 16, 20), (2, 5, 9, 13)]
CASES = [(s, C) for s in SHAPES for C in (2, 3, 4, 8)] + [((3, 420, 420), 4)]


def make_inputs(shape, C, seed):
    rng = np.random.default_rng(seed)
    N, sp = shape[0], shape[1:]
    l1, l2 = mr.quantised_logits(rng, (N, C) + sp), mr.quantised_logits(rng, (N, C) + sp)
    # exact ties between class 0 and C - 1 at the top of the pixel: the first maximum (class 0) must win
    for l in (l1, l2):
        tie = rng.random((N,) + sp) < 0.05
        top = l.max(1) + 0.5
        l[:, 0][tie] = top[tie]
        l[:, C - 1][tie] = top[tie]
    # labels that follow head 1 on about half of the pixels (so that both confidence sums are populated), C and 255 sprinkled in
    lab = rng.integers(0, C, (N,) + sp)
    follow = rng.random((N,) + sp) < 0.5
    lab[follow] = l1.argmax(1)[follow]
    lab[rng.random((N,) + sp) < 0.02] = C
    lab[rng.random((N,) + sp) < 0.02] = 255
    return l1, l2, lab.astype(np.int64)


def rows_in_use(group_px, P, per_thread):
    units = group_px // per_thread if P % per_thread == 0 else group_px
    return min((units + 255) // 256, _lib.MONITOR_SLOTS)


def expected_ws_mask(C, N, n_first, P):
    """True for every workspace word the two accumulate launches may write: the headers and the rows of the blocks in use."""
    ga, gl, S = ops.monitor_group_words(C), ops.monitor_label_words(C), _lib.MONITOR_SLOTS
    m = np.zeros(ops.monitor_ws_words(C), bool)
    lr = ops.monitor_label_region(C)
    m[0:2] = m[lr:lr + 2] = True
    want_hdr = []
    for g, px in enumerate((n_first * P, (N - n_first) * P)):
        ra, rl = rows_in_use(px, P, 4), rows_in_use(px, P, 2)
        m[2 + g * S * ga: 2 + (g * S + ra) * ga] = True
        m[lr + 2 + g * S * gl: lr + 2 + (g * S + rl) * gl] = True
        want_hdr.append((ra, rl))
    return m, want_hdr


@pytest.mark.parametrize("shape,C", CASES, ids=["%s-C%d" % ("x".join(map(str, s)), c) for s, c in CASES])
def test_rows_against_the_restatement(shape, C):
    N, sp = shape[0], shape[1:]
    P = int(np.prod(sp))
    l1, l2, lab = make_inputs(shape, C, 900 + 7 * C + P % 1000)
    d1, d2, dlab = (torch.from_numpy(x).to(DEV) for x in (l1, l2, lab))
    _, _, p1, p2, _ = ops.pseudo_block(d1, d2, want_soft=False)
    assert torch.equal(p1.cpu(), torch.from_numpy(l1.argmax(1))) and torch.equal(p2.cpu(), torch.from_numpy(l2.argmax(1)))      # the inputs decide every arg-max
    f1, f2 = ops.largest_cc(p1, C), ops.largest_cc(p2, C)
    fm = (f1.cpu().numpy(), f2.cpu().numpy())
    W = ops.monitor_row_words(C)
    scal = torch.tensor([0.1, -2.5, 3.0e-8, 7.0, 11.25], dtype=torch.float32, device=DEV)
    worst = 0.0
    for k, n_first in enumerate((0, 2, N)):
        ws = torch.full((ops.monitor_ws_words(C),), NAN_WORD, dtype=torch.int64, device=DEV)
        frame = torch.full((R + 2, W), float("nan"), dtype=torch.float64, device=DEV)
        ring = frame[1:1 + R]
        ring.copy_(torch.arange(R * W, dtype=torch.float64).reshape(R, W) + 0.5)          # nonzero content in every slot
        before = ring.cpu().clone()
        slot, it = 5 + k, 40 + k                                                           # row (5 + k) % 4
        slot_iter = torch.tensor([slot, it], dtype=torch.int32, device=DEV)
        got = []
        for rep in range(2):
            ops.monitor_accumulate(d1, d2, dlab, ws, n_first)
            ops.monitor_accumulate_labels(f1, f2, dlab, ws, n_first, C)
            ops.monitor_finalize(ws, ring, slot_iter, C, [scal[i:i + 1] for i in range(5)])
            torch.cuda.synchronize()
            got.append(ring[slot % R].cpu().clone())
            if rep == 0:
                ring[slot % R].fill_(-1.0)                                                 # the second call must write every word again
        assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), "two calls differ (n_first=%d)" % n_first
        # the frame and the neighbouring slots
        fr = frame.cpu()
        assert torch.isnan(fr[0]).all() and torch.isnan(fr[R + 1]).all()
        for r in range(R):
            if r != slot % R:
                assert torch.equal(fr[1 + r], before[r]), "ring slot %d was touched" % r
        # the workspace: headers, rows in use, canaries everywhere else
        mask, want_hdr = expected_ws_mask(C, N, n_first, P)
        w = ws.cpu().numpy()
        assert (w[~mask] == NAN_WORD).all(), "a workspace word outside the rows in use was written"
        assert (w[mask] != NAN_WORD).all(), "a workspace word of a row in use was left unwritten"
        lr = ops.monitor_label_region(C)
        assert [(int(w[g]), int(w[lr + g])) for g in (0, 1)] == want_hdr
        # the row
        row = split_rows(got[0].numpy()[None], C)
        ref = mr.row_ref(l1, l2, lab, n_first, maps=fm)
        assert row["iteration"].tolist() == [it]
        for name in mr.COUNT_FIELDS + ("inter_f", "pred_f"):
            assert np.array_equal(row[name][0], ref[name]), (name, n_first, row[name][0], ref[name])
        a1, a2 = p1.cpu().numpy().reshape(N, -1), p2.cpu().numpy().reshape(N, -1)
        for g, sl in enumerate((slice(0, n_first), slice(n_first, N))):
            assert row["n_disagree"][0, g] == (a1[sl] != a2[sl]).sum()
            for h, a in enumerate((a1, a2)):
                assert row["pred"][0, g, h].tolist() == np.bincount(a[sl].ravel(), minlength=C).tolist()
                assert row["pred_f"][0, g, h].tolist() == np.bincount(fm[h].reshape(N, -1)[sl].ravel(), minlength=C).tolist()
        for name in ("conf_correct", "conf_err"):
            err, bnd = np.abs(row[name][0] - ref[name]), ref[name + "_b"]
            ratio = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
            print("%s n_first=%d |err| %s bound %s" % (name, n_first, err.ravel().tolist(), bnd.ravel().tolist()))
            assert (err[bnd == 0] == 0).all() and (ratio <= 1.0).all(), (name, n_first, err, bnd)
            worst = max(worst, float(ratio.max()))
        assert (ref["conf_correct"].sum() > 0) and (ref["conf_err"].sum() > 0)
        sc = row["scalars"][0]
        assert sc[:5].tolist() == [float(x) for x in scal.cpu().double()] and (sc[5:] == 0).all()         # widened exactly; the unused words are 0
    print(json.dumps({"kernel": "chap_monitor_accumulate+labels+finalize", "shape": [N, C] + list(sp), "n_first": [0, 2, N],
                      "conf_worst_err_over_bound": round(worst, 6)}))


def test_finalize_without_a_label_launch_writes_zeros():
    C, N, sp = 4, 4, (16, 20)
    l1, l2, lab = make_inputs((N,) + sp, C, 77)
    d1, d2, dlab = (torch.from_numpy(x).to(DEV) for x in (l1, l2, lab))
    ws = torch.full((ops.monitor_ws_words(C),), NAN_WORD, dtype=torch.int64, device=DEV)
    ring = torch.full((2, ops.monitor_row_words(C)), float("nan"), dtype=torch.float64, device=DEV)
    slot_iter = torch.tensor([3, 9], dtype=torch.int32, device=DEV)
    ops.monitor_accumulate(d1, d2, dlab, ws, 2)
    ops.monitor_finalize(ws, ring, slot_iter, C, [], has_labels=False)
    torch.cuda.synchronize()
    assert torch.isnan(ring[0]).all()
    row = split_rows(ring[1].cpu().numpy()[None], C)
    ref = mr.row_ref(l1, l2, lab, 2)
    assert (row["inter_f"] == 0).all() and (row["pred_f"] == 0).all() and (row["scalars"] == 0).all() and row["iteration"].tolist() == [9]
    for name in mr.COUNT_FIELDS:
        assert np.array_equal(row[name][0], ref[name]), name


def test_misaligned_and_unbuilt_arguments_are_refused_on_device_pointers():
    C = 4
    l = torch.zeros(2, C, 8, 8, device=DEV)
    lab = torch.zeros(2, 8, 8, dtype=torch.int64, device=DEV)
    ws = torch.zeros(ops.monitor_ws_words(C), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.ChapError, match="bad shape"):
        ops.monitor_accumulate(l, l, lab, ws, 3)
    with pytest.raises(_lib.ChapError, match=r"C=9 \(2..8 built\)"):
        ops.monitor_accumulate(torch.zeros(2, 9, 8, 8, device=DEV), torch.zeros(2, 9, 8, 8, device=DEV), lab, ws, 0)
    with pytest.raises(_lib.ChapError, match="8-byte aligned"):
        ops.monitor_accumulate(l, l, lab, torch.zeros(ws.numel() * 2 + 1, dtype=torch.int32, device=DEV)[1:], 0)      # a workspace 4 bytes off
