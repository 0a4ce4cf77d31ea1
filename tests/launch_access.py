"""Access table of the C ABI (include/chap_hip.h and the opt-in headers chap_hip_ext.h, chap_hip_monitor.h, chap_hip_guard.h): for every
entry point of chap_amd._lib's binding tables (_SIGS, _SIGS_EXT, _SIGS_MONITOR, _SIGS_GUARD), and for chap_pack_multi, which pointer
fields of its params struct a launch reads (R), writes (W) or reads and writes (RW: accumulated outputs, workspaces), and the bytes behind
each pointer.  Host only: ctypes structs in, plain tuples out.  tests/issue_trace.py resolves every recorded launch through accesses();
tests/launch_order.py decides from the result which launches conflict.

A field is named by its path with array indices collapsed: `src.ptr` stands for src[0].ptr and src[1].ptr, `g` for g[0..2], `term.acc`
for term[0..3].acc.  MODES[entry point] classifies every such path (tests/test_launch_access_cpu.py walks the structs and fails on a
pointer field that has no entry, or an entry that names no field).

An extent is the tuple (base, pitch, row_bytes, rows): the bytes [base + i * pitch, base + i * pitch + row_bytes) for i < rows.  A
contiguous range is one row (pitch 0).  The channel slice [coff, coff + C) of pixels of ld elements is (ptr + coff * es, ld * es, C * es,
pixels), so two launches that fill different slots of one concat buffer do not meet.  Every rule is an UPPER bound of what the header lets
the kernel touch -- the sizes the header prescribes for a buffer, never an estimate from below; a pointer field without a rule (wpacked,
bias, the workspaces sized by a chap_*_ws function, everything off the training path) gets None: the
recorder then takes the whole live allocation around the pointer.  What is declared here is what the check sees; that a kernel stays
inside it is the business of the per-element tests with NaN-filled outputs.
"""
import ctypes as C

from chap_amd import _lib as L

R, W, RW = "R", "W", "RW"

_SRC = {"ptr": R, "scale": R, "shift": R, "keep": R, "chan_mul": R}


def _src(prefix):
    return {prefix + "." + k: v for k, v in _SRC.items()}


_CONV = dict(_src("src"), wpacked=R, bias=R, out=W, stats=W, stats_shift=R, out2=W)
_ACT_BWD = dict(_src("r"), g=R, g_pool=R, pool_idx=R, mean=R, invstd=R, gamma=R, sums=RW, gout=W, dgamma=RW, dbeta=RW)
_MIX = dict(logits=R, target_a=R, target_b=R, mask=R, acc=RW, loss=RW, dlogits=RW, gscale_dev=R)
_MIX_MULTI = {"term." + k: v for k, v in _MIX.items()}
_AUG = dict(images=R, labels=R, records=R, image_out=W, label_out=W)
_WINDOW_ACC = dict(logits=R, origins=R, score=RW, cnt=RW)
_SGD = dict(param=RW, grad=RW, grad2=RW, mom=RW, lr=R)
_SGD_EMA = dict({"sgd." + k: v for k, v in _SGD.items()}, ema=RW, coef=R)

MODES = {
    "chap_conv_fwd": _CONV,
    "chap_pack_weights": dict(w=R, out=W),
    "chap_pack_multi": dict(w=R, out=W),                        # per PackEntry of the host-side list
    "chap_conv_c1_fwd": dict(x=R, w=R, bias=R, out=W, stats=W, stats_shift=R),
    "chap_conv_c1_bwd": dict(g=R, w=R, x=R, dx=W, dw=RW, db=RW, ws=RW),
    "chap_wgrad": dict(_src("a"), **_src("b"), dw=RW, db=RW, ws=RW),
    "chap_bn_finalize": dict(stats=R, stats_shift=R, gamma=R, beta=R, running_mean=RW, running_var=RW, num_batches_tracked=RW,
                             scale=W, shift=W, mean=W, invstd=W),
    "chap_bn_eval_affine": dict(gamma=R, beta=R, running_mean=R, running_var=R, scale=W, shift=W),
    "chap_act_bwd_reduce": _ACT_BWD,
    "chap_act_bwd_apply": _ACT_BWD,
    "chap_act_pool2": dict(_src("r"), out=W, idx=W),
    "chap_upsample2x": dict(_src("r"), out=W),
    "chap_upsample2x_bwd": dict(g=R, out=W),
    "chap_planar_to_cl": dict(in_=R, out=W),
    "chap_channel_sum": dict(_src("r"), out=RW, ws=RW),
    "chap_cl_to_planar": dict(_src("r"), out=W),
    "chap_ensemble_argmax": dict(logits1=R, logits2=R, prob=W, label=W),
    "chap_window_accumulate": _WINDOW_ACC,
    "chap_window_finalize": dict(score=RW, cnt=R, label=W),
    "chap_mix_loss_fwd": _MIX,
    "chap_mix_loss_bwd": _MIX,
    "chap_pseudo_block": dict(logits1=R, logits2=R, soft1=W, soft2=W, arg1=W, arg2=W, knowledge=W),
    "chap_kl_fwd_bwd": dict(logits=R, target=R, loss=RW, dlogits=RW, gscale_dev=R, ws=RW),
    "chap_l2_normalize": dict(in_=R, out=W, ws=RW),
    "chap_perturb": dict(x=R, d=R, mask=R, out=W),
    "chap_rand_uniform": dict(out=W, seed_dev=R),
    "chap_keep_mask": dict(keep=W, seed_dev=R),
    "chap_chan_mask": dict(mul=W, seed_dev=R),
    "chap_box_mix": dict(a=R, b=R, out=W, box=R),
    "chap_box_mask": dict(mask=W, box=R),
    "chap_largest_cc": dict(labels=R, out=W, ws=RW),
    "chap_diff_mask": dict(p1=R, p2=R, knowledge=R, out=W, pooled_ws=RW),
    "chap_sgd_step": _SGD,
    "chap_sample_channel_sum": dict(_src("r"), partial=W),
    "chap_channel_drop": dict(pool_partial=R, grad_sim=R, u1=R, u2=R, mul1=W, mul2=W, probs_out=W),
    "chap_fold_perturbed": dict(g=R, mul=R, out=W),
    "chap_grad_sim": dict(gl=R, gu=R, score=RW),
    "chap_metrics": dict(a=R, b=R, classes=R, border_a=W, border_b=W, dist=W, results=W, ws=RW),
    "chap_augment2d": _AUG, "chap_augment3d": _AUG, "chap_augment3d_padded": _AUG,
    "chap_window_gather": dict(volume=R, origins=R, patches=W),
    "chap_window_accumulate_heads": _WINDOW_ACC,
    "chap_mix_loss_multi_fwd": _MIX_MULTI,
    "chap_mix_loss_multi_bwd": _MIX_MULTI,
    "chap_bcp_mix": dict(a=R, b=R, out=W, mask=W, box=R),
    "chap_residual_fwd": dict(_src("r"), **_src("src"), xin=R, out=W),
    "chap_residual_bwd": dict(g=R, out=R, chan_mul=R, gout=W, dxin=W),
    "chap_grad_sum": dict(g=R, out=W),
    # the opt-in entry points (_SIGS_EXT, _SIGS_GUARD, _SIGS_MONITOR): issued only with a teacher, a StepGuard, a StepMonitor attached
    "chap_sgd_ema_step": _SGD_EMA,
    "chap_grad_norm": dict(grad=R, grad2=R, ws=RW, state=RW),           # state: reads `steps`, writes the header and one row
    "chap_sgd_guard_step": dict({"se." + k: v for k, v in _SGD_EMA.items()}, state=R),
    # each accumulate launch writes a region of its own of the workspace (partial rows, nothing to zero), which is what lets the two run on two streams
    "chap_monitor_accumulate": dict(logits=R, labels=R, ws=W),
    "chap_monitor_accumulate_labels": dict(maps=R, labels=R, ws=W),
    "chap_monitor_finalize": dict(ws=R, ring=W, slot_iter=R, scalars=R),
}


def struct_of(name):
    if name == "chap_pack_multi":
        return L.PackEntry
    for table in (L._SIGS, L._SIGS_EXT, L._SIGS_MONITOR, L._SIGS_GUARD):
        if name in table:
            return table[name]
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- struct reflection
def _walk_type(ctype, path):
    """(collapsed path,) of every pointer field of a ctypes type."""
    if isinstance(ctype, type) and issubclass(ctype, C.Array):
        yield from _walk_type(ctype._type_, path)
    elif isinstance(ctype, type) and issubclass(ctype, C.Structure):
        for fname, ftype in ctype._fields_:
            yield from _walk_type(ftype, (path + "." if path else "") + fname)
    elif ctype is C.c_void_p:
        yield path


def pointer_paths(struct_type):
    """The collapsed paths of all pointer fields of a params struct, in declaration order."""
    return list(dict.fromkeys(_walk_type(struct_type, "")))


def _walk_value(value, ctype, path, cpath):
    if issubclass(ctype, C.Array):
        for i in range(ctype._length_):
            yield from _walk_value(value[i], ctype._type_, "%s[%d]" % (path, i), cpath)
    elif issubclass(ctype, C.Structure):
        for fname, ftype in ctype._fields_:
            yield from _walk_value(getattr(value, fname), ftype, (path + "." if path else "") + fname, (cpath + "." if cpath else "") + fname)
    elif ctype is C.c_void_p:
        yield path, cpath, int(value or 0)


def pointer_values(params):
    """(indexed path, collapsed path, address) of every pointer field of a params struct instance; NULL is 0."""
    return list(_walk_value(params, type(params), "", ""))


# ---------------------------------------------------------------------------------------------------------------- extents
def span(ptr, nbytes):
    return (int(ptr or 0), 0, int(nbytes), 1)


def rows(ptr, pitch, row_bytes, nrows):
    """`nrows` rows of `row_bytes` bytes, `pitch` bytes apart; rows that touch or overlap are one range."""
    ptr, pitch, row_bytes, nrows = int(ptr or 0), int(pitch), int(row_bytes), int(nrows)
    if nrows <= 1 or row_bytes >= pitch:
        return span(ptr, (max(nrows, 1) - 1) * pitch + row_bytes if nrows >= 1 else 0)
    return (ptr, pitch, row_bytes, nrows)


def bounds(ext):
    base, pitch, row_bytes, nrows = ext
    return base, base + (nrows - 1) * pitch + row_bytes


def byte_set(ext):
    """Every byte address of an extent (tests: small cases only)."""
    base, pitch, row_bytes, nrows = ext
    return {base + i * pitch + j for i in range(nrows) for j in range(row_bytes)}


def _rows_hit(lo, hi, ext):
    """Does [lo, hi) meet a row of ext?"""
    base, pitch, row_bytes, nrows = ext
    if hi <= lo or row_bytes <= 0:
        return False
    if nrows == 1:
        return base < hi and lo < base + row_bytes
    # rows j with base + j * pitch < hi and base + j * pitch + row_bytes > lo
    j_lo = max(0, (lo - base - row_bytes) // pitch + 1)
    j_hi = min(nrows - 1, (hi - base - 1) // pitch)
    return j_lo <= j_hi


def intersects(a, b):
    """Exact: do the two byte sets share a byte?"""
    if a[2] <= 0 or b[2] <= 0:
        return False
    alo, ahi = bounds(a)
    blo, bhi = bounds(b)
    if ahi <= blo or bhi <= alo:
        return False
    if a[3] > 1 and b[3] > 1 and a[1] == b[1]:
        # equal pitch p, row_bytes <= p: row j of b starts q rows and r bytes behind row 0 of a
        p = a[1]
        q, r = divmod(b[0] - a[0], p)
        # b's row j meets a's row j + q (when r < a.row_bytes) or a's row j + q + 1 (when its tail r + b.row_bytes passes p)
        for shift, hit in ((q, r < a[2]), (q + 1, r + b[2] > p)):
            if hit and max(0, -shift) <= min(b[3] - 1, a[3] - 1 - shift):
                return True
        return False
    if a[3] > b[3]:
        a, b = b, a
    base, pitch, row_bytes, nrows = a
    return any(_rows_hit(base + i * pitch, base + i * pitch + row_bytes, b) for i in range(nrows))


# ---------------------------------------------------------------------------------------------------------------- extent rules
def _es(p):
    return 2 if p.dtype == L.BF16 else 4


def _d(v):
    return max(int(v), 1)


def _src_rules(out, path, s, npix, nsamples, es):
    """A chap_src_t: the channel slice of `npix` pixels, scale and shift [C] (indexed from the pointer: channel c of the slice reads scale[c]),
    the dense keep mask [pixels][C], the multipliers [N][C]."""
    for k in ("scale", "shift"):
        if getattr(s, k):
            out[path + "." + k] = span(getattr(s, k), s.C * 4)
    if s.ptr:
        out[path + ".ptr"] = rows((s.ptr or 0) + s.coff * es, s.ld * es, s.C * es, npix)
    if s.keep:
        out[path + ".keep"] = span(s.keep, npix * s.C)
    if s.chan_mul:
        out[path + ".chan_mul"] = span(s.chan_mul, nsamples * s.C * 4)


def _grads(out, p, n, npix, Cc, es):
    for i in range(n):
        if p.g[i]:
            out["g[%d]" % i] = rows((p.g[i] or 0) + p.g_coff[i] * es, p.g_ld[i] * es, Cc * es, npix)


def _stats(ptr, clog):
    return span(ptr, (L.STATS_HDR + L.STATS_MAX_SLOTS * 2 * clog) * 4)


def _conv(p):
    out, es = {}, _es(p)
    npix, nin = p.N * _d(p.D) * p.H * p.W, p.N * _d(p.ID or p.D) * p.IH * p.IW
    for i in range(p.nsrc):
        _src_rules(out, "src[%d]" % i, p.src[i], nin, p.N, es)
    oes = 4 if (p.out_f32 or p.out_planar) else es
    fine = npix * (1 if p.out_mode == 0 else 8 if p.dims == 3 else 4)
    if p.out_planar:
        if p.out_coff == 0:
            out["out"] = span(p.out, fine * (p.out_Cn if p.out_mode else p.Cout) * 4)
    elif p.out_mode == 1:
        out["out"] = rows((p.out or 0) + p.out_coff * oes, p.out_ld * oes, p.out_Cn * oes, fine)
    else:
        first = p.out2_from if p.out2 else p.Cout
        out["out"] = rows((p.out or 0) + p.out_coff * oes, p.out_ld * oes, first * oes, npix)
        if p.out2:
            out["out2"] = rows((p.out2 or 0) + p.out_coff * oes, p.out_ld * oes, (p.Cout - p.out2_from) * oes, npix)
    if p.stats:
        out["stats"] = _stats(p.stats, p.Cout)
    if p.stats_shift:
        out["stats_shift"] = span(p.stats_shift, (p.out_Cn if p.out_mode else p.Cout) * 4)
    return out


def _conv_c1(p):
    npix = p.N * _d(p.D) * p.H * p.W
    out = {"x": span(p.x, npix * 4), "out": span(p.out, npix * p.Cout * _es(p))}
    if p.stats:
        out["stats"] = _stats(p.stats, p.Cout)
    if p.stats_shift:
        out["stats_shift"] = span(p.stats_shift, p.Cout * 4)
    return out


def _conv_c1_bwd(p):
    npix = p.N * _d(p.D) * p.H * p.W
    return {"g": span(p.g, npix * p.Cout * _es(p)), "x": span(p.x, npix * 4), "dx": span(p.dx, npix * 4),
            "dw": span(p.dw, p.Cout * 3 ** p.dims * 4), "db": span(p.db, p.Cout * 4)}


def _wgrad(p):
    out, es = {}, _es(p)
    nb, na = p.N * _d(p.D) * p.H * p.W, p.N * _d(p.ID or p.D) * p.IH * p.IW
    for i in range(p.na):
        _src_rules(out, "a[%d]" % i, p.a[i], na, p.N, es)
    _src_rules(out, "b", p.b, nb, p.N, es)
    kc = p.kc_valid or (p.a[0].C if (p.combine or p.na == 1) else p.a[0].C + p.a[1].C)
    kn = p.kn_valid or p.b.C
    taps = p.ksize ** p.dims
    # dw[tap * s_tap + kc * s_kc + kn * s_kn]: everything up to the last element written
    out["dw"] = span(p.dw, ((taps - 1) * p.s_tap + (kc - 1) * p.s_kc + (kn - 1) * p.s_kn + 1) * 4)
    out["db"] = span(p.db, kn * 4)                            # db[kn] for kn < kn_valid only, as dw
    if p.ws_bytes:
        out["ws"] = span(p.ws, p.ws_bytes)
    return out


def _bn_finalize(p):
    out = {k: span(getattr(p, k), p.C * 4) for k in ("stats_shift", "gamma", "beta", "running_mean", "running_var", "scale", "shift", "mean", "invstd")}
    out["stats"] = _stats(p.stats, p.Clog)
    out["num_batches_tracked"] = span(p.num_batches_tracked, 8)
    return out


def _bn_eval(p):
    return {k: span(getattr(p, k), p.C * 4) for k in ("gamma", "beta", "running_mean", "running_var", "scale", "shift")}


def _pooled(N, D, H, W):
    return N * (D // 2 if D > 1 else 1) * (H // 2) * (W // 2)


def _act_bwd(p):
    out, es, Cc = {}, _es(p), p.r.C
    npix = p.N * _d(p.D) * p.H * p.W
    _grads(out, p, p.ng, npix, Cc, es)
    _src_rules(out, "r", p.r, npix, p.N, es)
    pooled = _pooled(p.N, _d(p.D), p.H, p.W)
    out["g_pool"], out["pool_idx"] = span(p.g_pool, pooled * Cc * es), span(p.pool_idx, pooled * Cc)
    for k in ("mean", "invstd", "gamma", "dgamma", "dbeta"):
        out[k] = span(getattr(p, k), Cc * 4)
    out["sums"] = span(p.sums, (1 + L.ACT_BWD_SLOTS) * 2 * Cc * 4)
    out["gout"] = span(p.gout, npix * Cc * es)
    return out


def _pool(p):
    out, es = {}, _es(p)
    _src_rules(out, "r", p.r, p.N * _d(p.D) * p.H * p.W, p.N, es)
    pooled = _pooled(p.N, _d(p.D), p.H, p.W)
    out["out"], out["idx"] = span(p.out, pooled * p.r.C * es), span(p.idx, pooled * p.r.C)
    return out


def _upsample(p):
    out, es = {}, _es(p)
    npix = p.N * _d(p.D) * p.H * p.W
    _src_rules(out, "r", p.r, npix, p.N, es)
    out["out"] = rows((p.out or 0) + p.out_coff * es, p.out_ld * es, p.r.C * es, npix * (8 if p.dims == 3 else 4))
    return out


def _upsample_bwd(p):
    es, npix = _es(p), p.N * _d(p.D) * p.H * p.W
    return {"g": rows((p.g or 0) + p.g_coff * es, p.g_ld * es, p.C * es, npix * (8 if p.dims == 3 else 4)), "out": span(p.out, npix * p.C * es)}


def _planar_to_cl(p):
    es = _es(p)
    return {"in_": span(p.in_, p.N * p.C * p.P * 4), "out": rows((p.out or 0) + p.out_coff * es, p.out_ld * es, max(p.C, p.Cpad) * es, p.N * p.P)}


def _cl_to_planar(p):
    out = {"out": span(p.out, p.N * p.r.C * p.P * 4)}
    _src_rules(out, "r", p.r, p.N * p.P, p.N, _es(p))
    return out


def _chansum(p):
    out = {"out": span(p.out, p.r.C * 4), "ws": span(p.ws, L.CHANSUM_SLOTS * p.r.C * 4)}
    _src_rules(out, "r", p.r, p.npix, p.npix // max(p.pix_per_sample, 1), _es(p))
    return out


def _mix_term(out, prefix, t):
    logits, labels = t.N * t.C * t.P * 4, t.N * t.P * 8
    out.update({prefix + "logits": span(t.logits, logits), prefix + "dlogits": span(t.dlogits, logits),
                prefix + "target_a": span(t.target_a, labels), prefix + "target_b": span(t.target_b, labels), prefix + "mask": span(t.mask, labels),
                prefix + "acc": span(t.acc, (1 + L.LOSS_SLOTS) * 2 * (1 + 3 * t.C + 1) * 4),
                prefix + "loss": span(t.loss, 12), prefix + "gscale_dev": span(t.gscale_dev, 4)})


def _mix(p):
    out = {}
    _mix_term(out, "", p)
    return out


def _mix_multi(p):
    out = {}
    for i in range(p.nterms):
        _mix_term(out, "term[%d]." % i, p.term[i])
    return out


def _pseudo(p):
    logits, px = p.N * p.C * p.P * 4, p.N * p.P
    return {"logits1": span(p.logits1, logits), "logits2": span(p.logits2, logits), "soft1": span(p.soft1, logits), "soft2": span(p.soft2, logits),
            "arg1": span(p.arg1, px * 8), "arg2": span(p.arg2, px * 8), "knowledge": span(p.knowledge, px * 4)}


def _kl(p):
    logits = p.N * p.C * p.P * 4
    out = {"loss": span(p.loss, 4), "gscale_dev": span(p.gscale_dev, 4), "ws": span(p.ws, (1 + L.LOSS_SLOTS) * 2 * (3 * p.C + 1) * 4)}
    for h in range(2):
        for k in ("logits", "target", "dlogits"):
            out["%s[%d]" % (k, h)] = span(getattr(p, k)[h] or 0, logits)
    return out


def _l2norm(p):
    return {"in_": span(p.in_, p.N * p.P * 4), "out": span(p.out, p.N * p.P * 4), "ws": span(p.ws, p.N * L.L2NORM_SLOTS * 4)}


def _axpy(p):
    return {k: span(getattr(p, k), p.n * 4) for k in ("x", "d", "mask", "out")}


def _rand(field, elem):
    return lambda p: {field: span(getattr(p, field), p.n * elem), "seed_dev": span(p.seed_dev, 8)}


def _box_mix(p):
    n = p.N * _d(p.D) * p.H * p.W * (8 if p.is_i64 else 4)
    return {"a": span(p.a, n), "b": span(p.b, n), "out": span(p.out, n)}


def _box_mask(p):
    return {"mask": span(p.mask, p.N * _d(p.D) * p.H * p.W * 8)}


def _bcp_mix(p):
    vox = _d(p.D) * p.H * p.W
    out = {"mask": span(p.mask, p.Nm * vox * 8)}
    for h in range(2):
        for k in ("a", "b", "out"):
            out["%s[%d]" % (k, h)] = span(getattr(p, k)[h] or 0, p.N[h] * vox * 4)
    return out


def _lcc(p):
    n = p.N * _d(p.D) * p.H * p.W * 8
    return {"labels": span(p.labels, n), "out": span(p.out, n)}


def _diff_mask(p):
    px = p.N * p.H * p.W
    return {"p1": span(p.p1, px * 8), "p2": span(p.p2, px * 8), "knowledge": span(p.knowledge, px * 4), "out": span(p.out, px * 4),
            "pooled_ws": span(p.pooled_ws, (p.N * (p.H // p.scale) * (p.W // p.scale) + p.N) * 4)}


def _sgd(p, prefix=""):
    out = {prefix + k: span(getattr(p, k), p.n * 4) for k in ("param", "grad", "grad2", "mom")}
    out[prefix + "lr"] = span(p.lr, 4)
    return out


def _sgd_ema(q, prefix=""):
    """chap_sgd_ema_params: the nested chap_sgd_params, the average [n] and its two coefficients (fp32 a, b)."""
    out = _sgd(q.sgd, prefix + "sgd.")
    out[prefix + "ema"], out[prefix + "coef"] = span(q.ema, q.sgd.n * 4), span(q.coef, 8)
    return out


def _grad_norm(p):
    return {"grad": span(p.grad, p.n * 4), "grad2": span(p.grad2, p.n * 4), "ws": span(p.ws, L.GRADNORM_SLOTS * 8),
            "state": span(p.state, C.sizeof(L.GuardState) + p.ring * C.sizeof(L.GuardRow))}         # CHAP_GUARD_STATE_BYTES(ring)


def _sgd_guard(p):
    out = _sgd_ema(p.se, "se.")
    out["state"] = span(p.state, C.sizeof(L.GuardState))        # scale and skip: the header alone, never a row
    return out


# the 8-byte words of the monitor's workspace and ring (the CHAP_MONITOR_* macros of include/chap_hip_monitor.h)
def _mon_label_region(Cc):
    return L.MONITOR_HDR + 2 * L.MONITOR_SLOTS * (8 + 5 * Cc)


def _mon_ws_words(Cc):
    return _mon_label_region(Cc) + L.MONITOR_HDR + 2 * L.MONITOR_SLOTS * 4 * Cc


def _mon_row_words(Cc):
    return 1 + 2 * (8 + 5 * Cc) + 2 * 4 * Cc + L.MONITOR_MAX_SCALARS


def _mon_accumulate(p):
    px = p.N * p.P
    return {"logits[0]": span(p.logits[0], px * p.C * 4), "logits[1]": span(p.logits[1], px * p.C * 4), "labels": span(p.labels, px * 8),
            "ws": span(p.ws, _mon_label_region(p.C) * 8)}                   # the logits region only


def _mon_accumulate_labels(p):
    px, lr = p.N * p.P, _mon_label_region(p.C)
    return {"maps[0]": span(p.maps[0], px * 8), "maps[1]": span(p.maps[1], px * 8), "labels": span(p.labels, px * 8),
            "ws": span((p.ws or 0) + lr * 8, (_mon_ws_words(p.C) - lr) * 8)}    # the label-map region only


def _mon_finalize(p):
    out = {"ws": span(p.ws, _mon_ws_words(p.C) * 8), "ring": span(p.ring, p.ring_rows * _mon_row_words(p.C) * 8), "slot_iter": span(p.slot_iter, 8)}
    out.update({"scalars[%d]" % k: span(p.scalars[k], 4) for k in range(p.nscalars)})
    return out


def _sample_chansum(p):
    out = {"partial": span(p.partial, p.N * p.nchunk * p.r.C * 4)}
    _src_rules(out, "r", p.r, p.N * p.pix_per_sample, p.N, _es(p))
    return out


def _channel_drop(p):
    u, rows_ = p.U * p.C * 4, (p.B + p.U) * p.C * 4
    return {"pool_partial": span(p.pool_partial, p.U * p.nchunk * p.C * 4), "grad_sim": span(p.grad_sim, p.C * 4), "u1": span(p.u1, u), "u2": span(p.u2, u),
            "mul1": span(p.mul1, rows_), "mul2": span(p.mul2, rows_), "probs_out": span(p.probs_out, u)}


def _fold(p):
    es = _es(p)
    return {"g": rows((p.g or 0) + p.coff * es, p.ld * es, p.C * es, (p.B + p.U) * p.pix_per_sample), "mul": span(p.mul, (p.B + p.U) * p.C * 4),
            "out": span(p.out, p.B * p.pix_per_sample * p.C * es)}


def _grad_sim(p):
    return {"gl": span(p.gl, p.C * p.K * 4), "gu": span(p.gu, p.C * p.K * 4), "score": span(p.score, p.C * 4)}


def _residual(p):
    out, es = {}, _es(p)
    npix = p.N * _d(p.D) * p.H * p.W
    _src_rules(out, "r", p.r, npix, p.N, es)
    for i in range(p.nsrc):
        _src_rules(out, "src[%d]" % i, p.src[i], npix, p.N, es)
    out["xin"], out["out"] = span(p.xin, npix * 4), span(p.out, npix * p.r.C * es)
    return out


def _residual_bwd(p):
    out, es = {}, _es(p)
    npix = p.N * _d(p.D) * p.H * p.W
    _grads(out, p, p.ng, npix, p.C, es)
    out.update(out=span(p.out, npix * p.C * es), gout=span(p.gout, npix * p.C * es), chan_mul=span(p.chan_mul, p.N * p.C * 4), dxin=span(p.dxin, npix * 4))
    return out


def _grad_sum(p):
    out, es = {}, _es(p)
    _grads(out, p, p.ng, p.npix, p.C, es)
    out["out"] = span(p.out, p.npix * p.C * es)
    return out


RULES = {
    "chap_conv_fwd": _conv, "chap_conv_c1_fwd": _conv_c1, "chap_conv_c1_bwd": _conv_c1_bwd, "chap_wgrad": _wgrad,
    "chap_bn_finalize": _bn_finalize, "chap_bn_eval_affine": _bn_eval, "chap_act_bwd_reduce": _act_bwd, "chap_act_bwd_apply": _act_bwd,
    "chap_act_pool2": _pool, "chap_upsample2x": _upsample, "chap_upsample2x_bwd": _upsample_bwd,
    "chap_planar_to_cl": _planar_to_cl, "chap_cl_to_planar": _cl_to_planar, "chap_channel_sum": _chansum,
    "chap_mix_loss_fwd": _mix, "chap_mix_loss_bwd": _mix, "chap_mix_loss_multi_fwd": _mix_multi, "chap_mix_loss_multi_bwd": _mix_multi,
    "chap_pseudo_block": _pseudo, "chap_kl_fwd_bwd": _kl, "chap_l2_normalize": _l2norm, "chap_perturb": _axpy,
    "chap_rand_uniform": _rand("out", 4), "chap_keep_mask": _rand("keep", 1), "chap_chan_mask": _rand("mul", 4),
    "chap_box_mix": _box_mix, "chap_box_mask": _box_mask, "chap_bcp_mix": _bcp_mix, "chap_largest_cc": _lcc, "chap_diff_mask": _diff_mask,
    "chap_sgd_step": _sgd, "chap_sample_channel_sum": _sample_chansum, "chap_channel_drop": _channel_drop,
    "chap_fold_perturbed": _fold, "chap_grad_sim": _grad_sim,
    "chap_residual_fwd": _residual, "chap_residual_bwd": _residual_bwd, "chap_grad_sum": _grad_sum,
    "chap_sgd_ema_step": _sgd_ema, "chap_grad_norm": _grad_norm, "chap_sgd_guard_step": _sgd_guard,
    "chap_monitor_accumulate": _mon_accumulate, "chap_monitor_accumulate_labels": _mon_accumulate_labels, "chap_monitor_finalize": _mon_finalize,
}


def accesses(name, params):
    """[(indexed field path, mode, address, extent or None)] for every non-NULL pointer of one launch's params struct: the extent of its
    rule, or None where the field has none (the caller takes the whole live allocation around the address)."""
    modes = MODES[name]
    refined = RULES[name](params) if name in RULES else {}
    return [(path, modes[cpath], addr, refined.get(path)) for path, cpath, addr in pointer_values(params) if addr]


def pack_multi_accesses(entries):
    """chap_pack_multi reads its entries from the device; the accesses come from the PackEntry list the caller built on the host:
    the parameter (Cout * Cin * taps floats, checkpoint layout) and the packed copy (`total` fragments of 64 lanes)."""
    modes, out = MODES["chap_pack_multi"], []
    for i, e in enumerate(entries):
        out.append(("entry[%d].w" % i, modes["w"], int(e.w), span(e.w, e.Cout * e.Cin * e.taps * 4)))
        out.append(("entry[%d].out" % i, modes["out"], int(e.out), None))
    return out
