"""The training monitor's row (include/chap_hip_monitor.h) restated in fp64 with numpy, and the bounds its tests hold the kernels to.

Written down before the first GPU run of the kernels and not changed after it:
  * every count is exact (integers; the ring holds them as fp64, exact below 2^53);
  * a confidence sum is a sum of fp32 soft-max maxima p = 1 / sum_c expf(z_c - zmax), each within kernel_ref.softmax_ref's bound
    (EW + |z - zmax| U32) p of the fp64 value, where |z - zmax| = 0 for the maximum and EW = max(8, C + 4) * 2^-24 counts the chain at C classes
    (class counts); the terms are widened exactly and added in fp64, n adds of partial sums <= sum p: n * 2^-53 * sum p.
    So  |conf - ref| <= EW(C) * sum p + n * 2^-53 * sum p  over the pixels the sum runs over.

The arg-max is chap_pseudo_block's: the first maximum.  The kernels take it over the fp32 soft-max, the restatement over the logits: the two
agree wherever two logits are either equal or further apart than fp32 resolves after expf, which `quantised_logits` guarantees (a grid of
1/32: exact ties are frequent, near ties do not exist)."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def EW(C):
    return max(8, C + 4) * U32


def quantised_logits(rng, shape, scale=2.0):
    """fp32 logits on a grid of 1/32: two classes of a pixel tie exactly or differ by at least 1/32."""
    return (np.round(rng.standard_normal(shape) * scale * 32.0) / 32.0).astype(np.float32)


def _head(z):
    """fp64 [N, C, P] -> (first arg-max [N, P], max soft-max [N, P])."""
    z = z.astype(np.float64)
    m = z.max(1, keepdims=True)
    return z.argmax(1), 1.0 / np.exp(z - m).sum(1)


def row_ref(logits1, logits2, labels, n_first, maps=None):
    """The words of one row, named and shaped as chap_amd.monitor.split_rows names them without the row axis: n, n_disagree [2 groups],
    gt [2, C], n_correct / conf_correct / conf_err [2, 2 heads], inter / pred [2, 2, C] and, with `maps` (two int label maps), inter_f / pred_f;
    plus conf_correct_b / conf_err_b, the bounds above.  logits [N, C, *sp] fp32, labels [N, *sp] int."""
    N, C = logits1.shape[:2]
    lab = np.asarray(labels).reshape(N, -1).astype(np.int64)
    heads = [_head(np.asarray(l).reshape(N, C, -1)) for l in (logits1, logits2)]
    out = {k: np.zeros((2,), np.float64) for k in ("n", "n_disagree")}
    out["gt"] = np.zeros((2, C))
    for k in ("n_correct", "conf_correct", "conf_err", "conf_correct_b", "conf_err_b"):
        out[k] = np.zeros((2, 2))
    for k in ("inter", "pred", "inter_f", "pred_f"):
        out[k] = np.zeros((2, 2, C))
    for g, sl in enumerate((slice(0, n_first), slice(n_first, N))):
        l = lab[sl]
        out["n"][g] = l.size
        out["n_disagree"][g] = (heads[0][0][sl] != heads[1][0][sl]).sum()
        for c in range(C):
            out["gt"][g, c] = (l == c).sum()
        for h, (arg, conf) in enumerate(heads):
            a, p = arg[sl], conf[sl]
            ok = a == l                                     # a label outside [0, C) equals no arg-max: never correct, in no gt[c]
            out["n_correct"][g, h] = ok.sum()
            for name, mask in (("conf_correct", ok), ("conf_err", ~ok)):
                s = p[mask].sum()
                out[name][g, h] = s
                out[name + "_b"][g, h] = EW(C) * s + int(mask.sum()) * U64 * s
            for c in range(C):
                out["pred"][g, h, c] = (a == c).sum()
                out["inter"][g, h, c] = ((a == c) & (l == c)).sum()
            if maps is not None:
                mp = np.asarray(maps[h]).reshape(N, -1)[sl]
                for c in range(C):
                    out["pred_f"][g, h, c] = (mp == c).sum()
                    out["inter_f"][g, h, c] = ((mp == c) & (l == c)).sum()
    return out


COUNT_FIELDS = ("n", "n_disagree", "gt", "n_correct", "inter", "pred")


def stack_rows(refs, iterations=None, scalars=None):
    """Several row_ref results -> the dict split_rows / StepMonitor.read() returns (a leading row axis), for StepMonitor.derive."""
    rows = {k: np.stack([r[k] for r in refs]) for k in COUNT_FIELDS + ("conf_correct", "conf_err", "inter_f", "pred_f")}
    rows["iteration"] = np.arange(1, len(refs) + 1) if iterations is None else np.asarray(iterations)
    rows["scalars"] = np.zeros((len(refs), 16)) if scalars is None else np.asarray(scalars, dtype=np.float64)
    return rows


# ---- acc_conf_analysis (train_ours_2D.py:152-193), restated: six numbers from soft-max outputs [N, 4, H, W] and labels [N, H, W]
def dc(a, b):
    """chap_amd.metrics.dc: 2 |A & B| / (|A| + |B|), 0.0 when both are empty."""
    den = int(a.sum()) + int(b.sum())
    return 2.0 * int((a & b).sum()) / den if den else 0.0


def avg_dice3(pred, gt):
    """calculate_avg_dice: the mean over the foreground classes 1, 2, 3."""
    return sum(dc(pred == c, gt == c) for c in (1, 2, 3)) / 3.0


def acc_conf_numpy(prob, label, labeled_bs):
    """(lab_dice, lab_corr_conf, lab_err_conf, unlab_dice, unlab_corr_conf, unlab_err_conf), the order of the reference's metrics dict."""
    res = []
    for p, gt in ((prob[:labeled_bs], label[:labeled_bs]), (prob[labeled_bs:], label[labeled_bs:])):
        conf, pred = p.max(axis=1), p.argmax(axis=1)
        err = pred != gt
        corr = ~err
        res += [avg_dice3(pred, gt), np.sum(conf * corr) / (np.sum(corr) + 1e-6), np.sum(conf * err) / (np.sum(err) + 1e-6)]
    return res
