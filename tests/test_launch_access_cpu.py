"""The access table of the C ABI (tests/launch_access.py): every pointer field of every params struct is classified, and every extent
rule gives exactly the bytes worked out by hand on a small case."""
import ctypes as C
import random

import pytest

from chap_amd import _lib as L
from tests import launch_access as A

# every binding table of chap_amd._lib, found by name: a fifth `_SIGS...` table is walked without anybody remembering to add it here
SIG_TABLES = {attr: getattr(L, attr) for attr in sorted(vars(L)) if attr.startswith("_SIGS")}
LAUNCHED = [name for table in SIG_TABLES.values() for name in table]
ENTRY_POINTS = LAUNCHED + ["chap_pack_multi"]


def _bytes(*ranges):
    """the union of [lo, lo + n) for (lo, n) in ranges"""
    out = set()
    for lo, n in ranges:
        out |= set(range(lo, lo + n))
    return out


def _by_field(name, p):
    return {path: (mode, ext) for path, mode, _, ext in A.accesses(name, p)}


# ---------------------------------------------------------------------------------------------------------------- coverage
def _pointer_paths_by_reflection(ctype, path=""):
    """Independent of launch_access's own walker: the pointer fields of a struct, arrays collapsed."""
    out = []
    for fname, ftype in ctype._fields_:
        here = (path + "." if path else "") + fname
        while isinstance(ftype, type) and issubclass(ftype, C.Array):
            ftype = ftype._type_
        if issubclass(ftype, C.Structure):
            out += _pointer_paths_by_reflection(ftype, here)
        elif ftype is C.c_void_p or (isinstance(ftype, type) and issubclass(ftype, C._Pointer)):
            out.append(here)
    return out


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_pointer_field_is_classified(name):
    assert name in A.MODES, "entry point %s has no classification in tests/launch_access.py" % name
    fields = set(_pointer_paths_by_reflection(A.struct_of(name)))
    assert fields, name
    assert fields - set(A.MODES[name]) == set(), "pointer fields of %s without a classification" % name
    assert set(A.MODES[name]) - fields == set(), "classification of %s names fields its struct does not have" % name
    assert set(A.MODES[name].values()) <= {A.R, A.W, A.RW}
    assert set(A.pointer_paths(A.struct_of(name))) == fields


def test_the_binding_tables_are_the_four_known_ones_and_disjoint():
    assert set(SIG_TABLES) >= {"_SIGS", "_SIGS_EXT", "_SIGS_MONITOR", "_SIGS_GUARD"}
    assert len(LAUNCHED) == len(set(LAUNCHED)) and all(isinstance(t, dict) and t for t in SIG_TABLES.values())
    for name in ("chap_sgd_ema_step", "chap_grad_norm", "chap_sgd_guard_step", "chap_monitor_accumulate", "chap_monitor_accumulate_labels",
                 "chap_monitor_finalize"):
        assert name in ENTRY_POINTS and name not in L._SIGS, name


def test_no_classification_or_rule_for_an_unknown_entry_point():
    assert set(A.MODES) == set(ENTRY_POINTS)
    assert set(A.RULES) <= set(LAUNCHED)
    for name in LAUNCHED:
        assert A.struct_of(name) is next(t[name] for t in SIG_TABLES.values() if name in t)
    with pytest.raises(KeyError):
        A.struct_of("chap_no_such_entry")


def test_accumulated_outputs_and_workspaces_are_read_write():
    for name, field in (("chap_wgrad", "dw"), ("chap_wgrad", "db"), ("chap_wgrad", "ws"), ("chap_conv_c1_bwd", "dw"), ("chap_conv_c1_bwd", "db"),
                        ("chap_act_bwd_reduce", "dgamma"), ("chap_act_bwd_reduce", "dbeta"), ("chap_act_bwd_reduce", "sums"),
                        ("chap_mix_loss_bwd", "dlogits"), ("chap_mix_loss_fwd", "acc"), ("chap_kl_fwd_bwd", "loss"), ("chap_channel_sum", "out"),
                        ("chap_sgd_step", "param"), ("chap_sgd_step", "grad"), ("chap_bn_finalize", "running_mean"), ("chap_largest_cc", "ws"),
                        ("chap_sgd_ema_step", "sgd.param"), ("chap_sgd_ema_step", "sgd.grad"), ("chap_sgd_ema_step", "sgd.grad2"),
                        ("chap_sgd_ema_step", "sgd.mom"), ("chap_sgd_ema_step", "ema"),
                        ("chap_sgd_guard_step", "se.sgd.param"), ("chap_sgd_guard_step", "se.sgd.grad"), ("chap_sgd_guard_step", "se.sgd.grad2"),
                        ("chap_sgd_guard_step", "se.sgd.mom"), ("chap_sgd_guard_step", "se.ema"),
                        ("chap_grad_norm", "ws"), ("chap_grad_norm", "state")):
        assert A.MODES[name][field] == A.RW, (name, field)
    # what the optimizer launches only read: the schedule words and the guard's verdict
    for name, field in (("chap_sgd_ema_step", "sgd.lr"), ("chap_sgd_ema_step", "coef"), ("chap_sgd_guard_step", "se.sgd.lr"),
                        ("chap_sgd_guard_step", "se.coef"), ("chap_sgd_guard_step", "state"), ("chap_grad_norm", "grad"), ("chap_grad_norm", "grad2")):
        assert A.MODES[name][field] == A.R, (name, field)


def test_null_pointers_give_no_access_and_a_field_without_rule_gives_none():
    p = L.ConvParams()
    assert A.accesses("chap_conv_fwd", p) == []
    p.nsrc, p.wpacked, p.bias = 1, 4096, 8192
    got = _by_field("chap_conv_fwd", p)
    assert got == {"wpacked": ("R", None), "bias": ("R", None)}         # the recorder takes the whole allocation


# ---------------------------------------------------------------------------------------------------------------- extents and their intersection
def test_rows_that_touch_are_one_range():
    assert A.rows(100, 8, 8, 4) == (100, 0, 32, 1)
    assert A.rows(100, 16, 8, 1) == (100, 0, 8, 1)
    assert A.rows(100, 16, 8, 3) == (100, 16, 8, 3)
    assert A.byte_set(A.rows(100, 16, 8, 3)) == _bytes((100, 8), (116, 8), (132, 8))


def test_intersection_is_exact_against_brute_force():
    rnd = random.Random(5)
    seen = {True: 0, False: 0}
    for _ in range(4000):
        def ext():
            pitch = rnd.choice((0, 8, 12, 16, 24))
            return A.rows(rnd.randrange(0, 64), pitch, rnd.randrange(1, 13), rnd.randrange(1, 6)) if pitch else A.span(rnd.randrange(0, 96), rnd.randrange(1, 20))
        a, b = ext(), ext()
        want = bool(A.byte_set(a) & A.byte_set(b))
        assert A.intersects(a, b) == want == A.intersects(b, a), (a, b)
        seen[want] += 1
    assert min(seen.values()) > 400          # both answers are exercised
    # inside each other's bounding box, yet disjoint: the channel slices [0, 4) and [4, 8) of one fp32 concat buffer of 8 channels
    lo, hi = A.rows(1000, 32, 16, 100), A.rows(1016, 32, 16, 100)
    assert not A.intersects(lo, hi) and A.intersects(lo, A.rows(1012, 32, 16, 100))


def _src(s, ptr, Cc, ld, coff, keep=None, chan_mul=None):
    s.ptr, s.C, s.ld, s.coff, s.keep, s.chan_mul = ptr, Cc, ld, coff, keep, chan_mul


def test_conv_sources_and_split_output_2d_kernel_on_a_stack_of_slices():
    """dims = 2 with D = 2 (the kernel does not extend over D: both slices count), fp32, a source that is channels [1, 3) of 4-channel
    pixels, the output split into two halves (out2) that each fill channels [2, 4) of 6-channel pixels."""
    p = L.ConvParams()
    p.nsrc, p.dtype, p.dims, p.ksize, p.stride = 1, L.F32, 2, 3, 1
    p.N, p.D, p.H, p.W, p.ID, p.IH, p.IW = 1, 2, 1, 2, 2, 1, 2                     # 4 pixels
    _src(p.src[0], 1000, 2, 4, 1, keep=3000, chan_mul=4000)
    p.src[0].scale, p.src[0].shift = 6000, 7000
    p.out, p.out2, p.Cout, p.out2_from, p.out_ld, p.out_coff = 5000, 9000, 4, 2, 6, 2
    p.stats, p.stats_shift = 20000, 30000
    got = _by_field("chap_conv_fwd", p)
    assert A.byte_set(got["src[0].ptr"][1]) == _bytes((1004, 8), (1020, 8), (1036, 8), (1052, 8))
    assert got["src[0].scale"] == ("R", (6000, 0, 8, 1)) and got["src[0].shift"] == ("R", (7000, 0, 8, 1))      # [C] from the pointer, not [ld]
    assert A.byte_set(got["src[0].keep"][1]) == _bytes((3000, 8))                  # dense [4 pixels][2 channels] bytes
    assert A.byte_set(got["src[0].chan_mul"][1]) == _bytes((4000, 8))              # [1 sample][2 channels] floats
    assert A.byte_set(got["out"][1]) == _bytes((5008, 8), (5032, 8), (5056, 8), (5080, 8))
    assert A.byte_set(got["out2"][1]) == _bytes((9008, 8), (9032, 8), (9056, 8), (9080, 8))
    assert got["stats"][1] == (20000, 0, (L.STATS_HDR + L.STATS_MAX_SLOTS * 2 * 4) * 4, 1)
    assert got["stats_shift"][1] == (30000, 0, 16, 1)
    assert [got[k][0] for k in ("src[0].ptr", "out", "out2", "stats", "stats_shift")] == ["R", "W", "W", "W", "R"]
    assert "src[1].ptr" not in got


def test_conv_depth_to_space_and_planar_outputs():
    p = L.ConvParams()
    p.nsrc, p.dtype, p.dims, p.ksize, p.stride = 1, L.BF16, 3, 1, 1
    p.N, p.D, p.H, p.W, p.ID, p.IH, p.IW = 1, 1, 1, 1, 1, 1, 1
    _src(p.src[0], 1000, 4, 4, 0)
    p.out, p.Cout, p.out_mode, p.out_Cn, p.out_ld, p.out_coff = 5000, 16, 1, 2, 4, 2     # 8 fine voxels, 2 of 4 bf16 channels each
    got = _by_field("chap_conv_fwd", p)
    assert A.byte_set(got["src[0].ptr"][1]) == _bytes((1000, 8))
    assert A.byte_set(got["out"][1]) == _bytes(*[(5004 + 8 * i, 4) for i in range(8)])
    p.out_mode, p.out_planar, p.out_coff, p.Cout, p.N, p.W = 0, 1, 0, 3, 2, 5              # fp32 [2][3][5] logits
    assert _by_field("chap_conv_fwd", p)["out"][1] == (5000, 0, 2 * 3 * 5 * 4, 1)


def test_wgrad_operands_and_the_accumulated_gradient():
    p = L.WgradParams()
    p.na, p.dtype, p.dims, p.ksize, p.stride = 2, L.F32, 2, 3, 1
    p.N, p.D, p.H, p.W, p.ID, p.IH, p.IW = 1, 1, 2, 2, 1, 2, 2
    _src(p.a[0], 1000, 2, 2, 0)
    _src(p.a[1], 2000, 1, 3, 2)
    _src(p.b, 3000, 2, 4, 2)
    p.dw, p.db, p.ws, p.ws_bytes = 10000, 20000, 30000, 48
    p.s_kn, p.s_kc, p.s_tap = 27, 9, 1                                            # checkpoint layout [Cout 2][Cin 3][9 taps]
    got = _by_field("chap_wgrad", p)
    assert A.byte_set(got["a[0].ptr"][1]) == _bytes((1000, 32))
    assert A.byte_set(got["a[1].ptr"][1]) == _bytes(*[(2008 + 12 * i, 4) for i in range(4)])
    assert A.byte_set(got["b.ptr"][1]) == _bytes(*[(3008 + 16 * i, 8) for i in range(4)])
    assert got["dw"] == ("RW", (10000, 0, 2 * 3 * 9 * 4, 1))
    assert got["db"] == ("RW", (20000, 0, 8, 1))
    assert got["ws"] == ("RW", (30000, 0, 48, 1))
    p.kc_valid, p.kn_valid = 2, 1                                                 # a padded head: only kc < 2, kn < 1 are written
    assert _by_field("chap_wgrad", p)["dw"][1] == (10000, 0, (8 + 9 + 0 + 1) * 4, 1)
    assert _by_field("chap_wgrad", p)["db"][1] == (20000, 0, 4, 1)


def test_upsample_and_its_adjoint():
    p = L.UpsampleParams()
    p.dtype, p.dims, p.N, p.D, p.H, p.W = L.BF16, 2, 1, 2, 1, 1                   # dims = 2 with D = 2: 2 coarse pixels, 8 fine ones
    _src(p.r, 1000, 2, 2, 0)
    p.out, p.out_ld, p.out_coff = 5000, 8, 4
    got = _by_field("chap_upsample2x", p)
    assert A.byte_set(got["r.ptr"][1]) == _bytes((1000, 8))
    assert A.byte_set(got["out"][1]) == _bytes(*[(5008 + 16 * i, 4) for i in range(8)])
    q = L.UpsampleBwdParams()
    q.dtype, q.dims, q.N, q.D, q.H, q.W, q.C = L.F32, 3, 1, 1, 1, 1, 2
    q.g, q.g_ld, q.g_coff, q.out = 5000, 3, 1, 9000
    got = _by_field("chap_upsample2x_bwd", q)
    assert A.byte_set(got["g"][1]) == _bytes(*[(5004 + 12 * i, 8) for i in range(8)])
    assert got["out"] == ("W", (9000, 0, 8, 1))


def test_layout_helpers_and_fold():
    p = L.PlanarToClParams()
    p.in_, p.out, p.N, p.C, p.P, p.out_ld, p.out_coff, p.Cpad, p.dtype = 1000, 5000, 2, 1, 3, 8, 2, 4, L.F32
    got = _by_field("chap_planar_to_cl", p)
    assert got["in_"] == ("R", (1000, 0, 24, 1))
    assert A.byte_set(got["out"][1]) == _bytes(*[(5008 + 32 * i, 16) for i in range(6)])      # channels [C, Cpad) are zero-filled: written
    q = L.ClToPlanarParams()
    q.N, q.P, q.dtype, q.out = 2, 3, L.BF16, 9000
    _src(q.r, 1000, 2, 4, 1)
    got = _by_field("chap_cl_to_planar", q)
    assert A.byte_set(got["r.ptr"][1]) == _bytes(*[(1002 + 8 * i, 4) for i in range(6)])
    assert got["out"] == ("W", (9000, 0, 2 * 2 * 3 * 4, 1))
    f = L.FoldParams()
    f.g, f.mul, f.out, f.B, f.U, f.C, f.ld, f.coff, f.pix_per_sample, f.dtype = 1000, 2000, 3000, 2, 1, 2, 4, 2, 2, L.F32
    got = _by_field("chap_fold_perturbed", f)
    assert A.byte_set(got["g"][1]) == _bytes(*[(1008 + 16 * i, 8) for i in range(6)])         # (B + U) * 2 pixels
    assert got["mul"] == ("R", (2000, 0, 3 * 2 * 4, 1))
    assert got["out"] == ("W", (3000, 0, 2 * 2 * 2 * 4, 1))


def test_residual_kernels_and_grad_sum():
    p = L.ResidualParams()
    p.N, p.D, p.H, p.W, p.dtype, p.nsrc, p.out = 1, 1, 1, 2, L.F32, 2, 9000
    _src(p.r, 1000, 8, 8, 0)
    _src(p.src[0], 2000, 8, 16, 8)
    _src(p.src[1], 3000, 8, 8, 0, chan_mul=4000)
    got = _by_field("chap_residual_fwd", p)
    assert got["r.ptr"][1] == (1000, 0, 64, 1) and got["out"] == ("W", (9000, 0, 64, 1))
    assert A.byte_set(got["src[0].ptr"][1]) == _bytes((2032, 32), (2096, 32))
    assert got["src[1].chan_mul"][1] == (4000, 0, 32, 1)
    q = L.ResidualBwdParams()
    q.N, q.D, q.H, q.W, q.C, q.dtype, q.ng = 1, 1, 1, 2, 8, L.BF16, 2
    q.g[0], q.g_ld[0], q.g_coff[0] = 1000, 8, 0
    q.g[1], q.g_ld[1], q.g_coff[1] = 2000, 24, 8
    q.out, q.gout, q.dxin, q.chan_mul = 3000, 4000, 5000, 6000
    got = _by_field("chap_residual_bwd", q)
    assert got["g[0]"][1] == (1000, 0, 32, 1)
    assert A.byte_set(got["g[1]"][1]) == _bytes((2016, 16), (2064, 16))
    assert got["out"] == ("R", (3000, 0, 32, 1)) and got["gout"] == ("W", (4000, 0, 32, 1))
    assert got["dxin"] == ("W", (5000, 0, 8, 1)) and got["chan_mul"] == ("R", (6000, 0, 32, 1))
    s = L.GradSumParams()
    s.ng, s.npix, s.C, s.dtype, s.out = 2, 3, 2, L.F32, 9000
    s.g[0], s.g_ld[0], s.g_coff[0] = 1000, 2, 0
    s.g[1], s.g_ld[1], s.g_coff[1] = 2000, 6, 4
    got = _by_field("chap_grad_sum", s)
    assert got["g[0]"][1] == (1000, 0, 24, 1) and got["out"] == ("W", (9000, 0, 24, 1))
    assert A.byte_set(got["g[1]"][1]) == _bytes((2016, 8), (2040, 8), (2064, 8))


def test_statistics_buffers():
    p = L.BnFinalizeParams()
    p.stats, p.stats_shift, p.gamma, p.running_mean, p.num_batches_tracked, p.scale = 1000, 2000, 3000, 4000, 5000, 6000
    p.C, p.Clog = 4, 16                       # a transposed conv: four sub-positions per channel in every slot row
    got = _by_field("chap_bn_finalize", p)
    assert got["stats"] == ("R", (1000, 0, (L.STATS_HDR + L.STATS_MAX_SLOTS * 2 * 16) * 4, 1))
    assert got["stats_shift"] == ("R", (2000, 0, 16, 1)) and got["gamma"] == ("R", (3000, 0, 16, 1))
    assert got["running_mean"] == ("RW", (4000, 0, 16, 1)) and got["num_batches_tracked"] == ("RW", (5000, 0, 8, 1))
    assert got["scale"] == ("W", (6000, 0, 16, 1))
    c1 = L.ConvC1Params()
    c1.x, c1.out, c1.stats, c1.N, c1.D, c1.H, c1.W, c1.Cout, c1.dtype = 1000, 2000, 3000, 2, 1, 2, 2, 16, L.BF16
    got = _by_field("chap_conv_c1_fwd", c1)
    assert got["x"] == ("R", (1000, 0, 32, 1)) and got["out"] == ("W", (2000, 0, 8 * 16 * 2, 1))
    assert got["stats"] == ("W", (3000, 0, (L.STATS_HDR + L.STATS_MAX_SLOTS * 2 * 16) * 4, 1))
    a = L.ActBwdParams()
    a.N, a.D, a.H, a.W, a.dtype, a.ng = 1, 1, 2, 2, L.F32, 1
    _src(a.r, 1000, 2, 2, 0)
    a.g[0], a.g_ld[0], a.g_coff[0] = 2000, 4, 2
    a.g_pool, a.pool_idx, a.sums, a.gout, a.dgamma = 3000, 4000, 5000, 6000, 7000
    got = _by_field("chap_act_bwd_reduce", a)
    assert A.byte_set(got["g[0]"][1]) == _bytes(*[(2008 + 16 * i, 8) for i in range(4)])
    assert got["g_pool"][1] == (3000, 0, 8, 1) and got["pool_idx"][1] == (4000, 0, 2, 1)
    assert got["sums"] == ("RW", (5000, 0, (1 + L.ACT_BWD_SLOTS) * 2 * 2 * 4, 1))
    assert got["gout"] == ("W", (6000, 0, 32, 1)) and got["dgamma"] == ("RW", (7000, 0, 8, 1))


def test_pack_multi_takes_its_accesses_from_the_host_side_entries():
    e = (L.PackEntry * 2)()
    e[0].w, e[0].out, e[0].Cin, e[0].Cout, e[0].taps = 1000, 5000, 2, 3, 9
    e[1].w, e[1].out, e[1].Cin, e[1].Cout, e[1].taps = 2000, 6000, 1, 16, 27
    assert A.pack_multi_accesses(e) == [("entry[0].w", "R", 1000, (1000, 0, 216, 1)), ("entry[0].out", "W", 5000, None),
                                        ("entry[1].w", "R", 2000, (2000, 0, 1728, 1)), ("entry[1].out", "W", 6000, None)]


# ---------------------------------------------------------------------------------------------------------------- the remaining rules, one small case each
def _spans(got, **want):
    """got[field] == (mode, one range of `bytes` at `ptr`) for field=(mode, ptr, bytes)"""
    for field, (mode, ptr, nbytes) in want.items():
        assert got[field.replace("__", ".")] == (mode, (ptr, 0, nbytes, 1)), field


def test_first_layer_backward():
    p = L.ConvC1BwdParams()
    p.g, p.w, p.x, p.dx, p.dw, p.db, p.ws = 1000, 2000, 3000, 4000, 5000, 6000, 7000
    p.N, p.D, p.H, p.W, p.dims, p.Cout, p.dtype = 1, 2, 1, 2, 3, 2, L.BF16          # 4 voxels, 2 bf16 channels, 27 taps
    got = _by_field("chap_conv_c1_bwd", p)
    _spans(got, g=("R", 1000, 4 * 2 * 2), x=("R", 3000, 4 * 4), dx=("W", 4000, 4 * 4), dw=("RW", 5000, 2 * 27 * 4), db=("RW", 6000, 2 * 4))
    assert got["w"] == ("R", None) and got["ws"] == ("RW", None)                    # no rule: the whole allocation
    p.dims, p.dtype = 2, L.F32                                                      # 9 taps, fp32 gradient
    _spans(_by_field("chap_conv_c1_bwd", p), g=("R", 1000, 4 * 2 * 4), dw=("RW", 5000, 2 * 9 * 4))


def test_eval_affine():
    p = L.BnEvalParams()
    p.gamma, p.beta, p.running_mean, p.running_var, p.scale, p.shift, p.C = 1000, 2000, 3000, 4000, 5000, 6000, 3
    _spans(_by_field("chap_bn_eval_affine", p), gamma=("R", 1000, 12), beta=("R", 2000, 12), running_mean=("R", 3000, 12),
           running_var=("R", 4000, 12), scale=("W", 5000, 12), shift=("W", 6000, 12))


def test_max_pool_2d_and_3d():
    p = L.PoolParams()
    p.N, p.D, p.H, p.W, p.dtype, p.out, p.idx = 1, 0, 4, 2, L.F32, 5000, 6000       # 2D (D unset): 8 pixels -> 2 x 1 pooled
    _src(p.r, 1000, 2, 2, 0)
    _spans(_by_field("chap_act_pool2", p), r__ptr=("R", 1000, 8 * 2 * 4), out=("W", 5000, 2 * 2 * 4), idx=("W", 6000, 2 * 2))
    p.D, p.dtype = 2, L.BF16                                                        # 3D: 16 voxels -> 1 x 2 x 1 pooled: D is halved too
    _spans(_by_field("chap_act_pool2", p), r__ptr=("R", 1000, 16 * 2 * 2), out=("W", 5000, 2 * 2 * 2), idx=("W", 6000, 2 * 2))
    a = L.ActBwdParams()                                                            # the pooled gradient of the backward, 3D
    a.N, a.D, a.H, a.W, a.dtype, a.g_pool, a.pool_idx = 1, 2, 2, 4, L.F32, 3000, 4000
    _src(a.r, 1000, 2, 2, 0)
    _spans(_by_field("chap_act_bwd_apply", a), g_pool=("R", 3000, 2 * 2 * 4), pool_idx=("R", 4000, 2 * 2))


def test_channel_sums():
    p = L.ChanSumParams()
    p.out, p.ws, p.npix, p.pix_per_sample, p.dtype = 5000, 6000, 6, 3, L.F32
    _src(p.r, 1000, 2, 4, 2, chan_mul=2000)
    got = _by_field("chap_channel_sum", p)
    assert A.byte_set(got["r.ptr"][1]) == _bytes(*[(1008 + 16 * i, 8) for i in range(6)])
    _spans(got, r__chan_mul=("R", 2000, 2 * 2 * 4), out=("RW", 5000, 8), ws=("RW", 6000, L.CHANSUM_SLOTS * 2 * 4))
    q = L.SampleChanSumParams()
    q.partial, q.N, q.nchunk, q.pix_per_sample, q.dtype = 5000, 2, 3, 2, L.BF16
    _src(q.r, 1000, 2, 2, 0)
    _spans(_by_field("chap_sample_channel_sum", q), r__ptr=("R", 1000, 4 * 2 * 2), partial=("W", 5000, 2 * 3 * 2 * 4))


def _mix_term(t, base, N):
    t.logits, t.target_a, t.target_b, t.mask, t.acc, t.loss, t.dlogits, t.gscale_dev = (base + 1000 * i for i in range(1, 9))
    t.N, t.C, t.P = N, 3, 5


def _mix_want(prefix, base, N):
    logits, labels = N * 3 * 5 * 4, N * 5 * 8                                       # fp32 [N][C][P]; int64 [N][P]
    acc = (1 + L.LOSS_SLOTS) * 2 * (1 + 3 * 3 + 1) * 4
    return {prefix + "logits": ("R", base + 1000, logits), prefix + "target_a": ("R", base + 2000, labels), prefix + "target_b": ("R", base + 3000, labels),
            prefix + "mask": ("R", base + 4000, labels), prefix + "acc": ("RW", base + 5000, acc), prefix + "loss": ("RW", base + 6000, 12),
            prefix + "dlogits": ("RW", base + 7000, logits), prefix + "gscale_dev": ("R", base + 8000, 4)}


def test_mix_loss_single_and_batched_terms():
    p = L.MixLossParams()
    _mix_term(p, 0, 2)
    for name in ("chap_mix_loss_fwd", "chap_mix_loss_bwd"):
        got = _by_field(name, p)
        assert got == {k: (m, (ptr, 0, n, 1)) for k, (m, ptr, n) in _mix_want("", 0, 2).items()}
    m = L.MixLossMultiParams()
    m.nterms = 2
    _mix_term(m.term[0], 0, 2)
    _mix_term(m.term[1], 100000, 1)
    want = dict(_mix_want("term[0].", 0, 2), **_mix_want("term[1].", 100000, 1))
    for name in ("chap_mix_loss_multi_fwd", "chap_mix_loss_multi_bwd"):
        assert _by_field(name, m) == {k: (mode, (ptr, 0, n, 1)) for k, (mode, ptr, n) in want.items()}


def test_pseudo_labels_and_vat_distance():
    p = L.PseudoParams()
    p.logits1, p.logits2, p.soft1, p.soft2, p.arg1, p.arg2, p.knowledge, p.N, p.C, p.P = 1000, 2000, 3000, 4000, 5000, 6000, 7000, 2, 3, 5
    _spans(_by_field("chap_pseudo_block", p), logits1=("R", 1000, 120), logits2=("R", 2000, 120), soft1=("W", 3000, 120), soft2=("W", 4000, 120),
           arg1=("W", 5000, 80), arg2=("W", 6000, 80), knowledge=("W", 7000, 40))     # int64 arg-max, fp32 knowledge
    k = L.KlParams()
    k.N, k.C, k.P, k.loss, k.gscale_dev, k.ws = 2, 3, 5, 7000, 8000, 9000
    for h in range(2):
        k.logits[h], k.target[h], k.dlogits[h] = 1000 + 100000 * h, 2000 + 100000 * h, 3000 + 100000 * h
    got = _by_field("chap_kl_fwd_bwd", k)
    for h in range(2):
        assert got["logits[%d]" % h] == ("R", (1000 + 100000 * h, 0, 120, 1)) and got["target[%d]" % h] == ("R", (2000 + 100000 * h, 0, 120, 1))
        assert got["dlogits[%d]" % h] == ("RW", (3000 + 100000 * h, 0, 120, 1))
    _spans(got, loss=("RW", 7000, 4), gscale_dev=("R", 8000, 4), ws=("RW", 9000, (1 + L.LOSS_SLOTS) * 2 * (3 * 3 + 1) * 4))
    k.dlogits[1] = None
    assert "dlogits[1]" not in _by_field("chap_kl_fwd_bwd", k)


def test_vat_helpers_and_random_numbers():
    n = L.L2NormParams()
    n.in_, n.out, n.ws, n.N, n.P = 1000, 2000, 3000, 2, 5
    _spans(_by_field("chap_l2_normalize", n), in_=("R", 1000, 40), out=("W", 2000, 40), ws=("RW", 3000, 2 * L.L2NORM_SLOTS * 4))
    a = L.AxpyParams()
    a.x, a.d, a.mask, a.out, a.n = 1000, 2000, 3000, 4000, 7
    _spans(_by_field("chap_perturb", a), x=("R", 1000, 28), d=("R", 2000, 28), mask=("R", 3000, 28), out=("W", 4000, 28))
    for name, struct, field, elem in (("chap_rand_uniform", L.RandParams, "out", 4), ("chap_keep_mask", L.KeepMaskParams, "keep", 1),
                                      ("chap_chan_mask", L.ChanMaskParams, "mul", 4)):
        r = struct()
        setattr(r, field, 1000)
        r.seed_dev, r.n = 2000, 7
        assert _by_field(name, r) == {field: ("W", (1000, 0, 7 * elem, 1)), "seed_dev": ("R", (2000, 0, 8, 1))}     # a one-byte keep mask, a uint64 seed word


def test_box_kernels_and_largest_component_on_volumes():
    b = L.BoxMixParams()
    b.a, b.b, b.out, b.box, b.N, b.D, b.H, b.W, b.is_i64 = 1000, 2000, 3000, 4000, 2, 3, 2, 2, 1       # 24 voxels of int64
    got = _by_field("chap_box_mix", b)
    _spans(got, a=("R", 1000, 192), b=("R", 2000, 192), out=("W", 3000, 192))
    assert got["box"] == ("R", None)
    b.D, b.is_i64 = 0, 0                                                            # 2D (D unset), fp32
    _spans(_by_field("chap_box_mix", b), a=("R", 1000, 32), out=("W", 3000, 32))
    m = L.BoxMaskParams()
    m.mask, m.box, m.N, m.D, m.H, m.W = 1000, 2000, 2, 3, 2, 2
    assert _by_field("chap_box_mask", m) == {"mask": ("W", (1000, 0, 192, 1)), "box": ("R", None)}
    c = L.BcpMixParams()
    c.mask, c.box, c.Nm, c.D, c.H, c.W = 7000, 8000, 3, 2, 2, 2                      # 8 voxels per sample
    for h, n in enumerate((1, 2)):
        c.a[h], c.b[h], c.out[h], c.N[h] = 1000 + 100000 * h, 2000 + 100000 * h, 3000 + 100000 * h, n
    got = _by_field("chap_bcp_mix", c)
    for h, n in enumerate((1, 2)):
        assert got["a[%d]" % h] == ("R", (1000 + 100000 * h, 0, n * 8 * 4, 1)) and got["b[%d]" % h] == ("R", (2000 + 100000 * h, 0, n * 8 * 4, 1))
        assert got["out[%d]" % h] == ("W", (3000 + 100000 * h, 0, n * 8 * 4, 1))
    assert got["mask"] == ("W", (7000, 0, 3 * 8 * 8, 1)) and got["box"] == ("R", None)
    l = L.LccParams()
    l.labels, l.out, l.ws, l.N, l.D, l.H, l.W = 1000, 2000, 3000, 2, 3, 2, 2
    assert _by_field("chap_largest_cc", l) == {"labels": ("R", (1000, 0, 192, 1)), "out": ("W", (2000, 0, 192, 1)), "ws": ("RW", None)}
    l.D = 0
    assert _by_field("chap_largest_cc", l)["labels"] == ("R", (1000, 0, 64, 1))


def test_diff_mask_sgd_channel_drop_and_grad_sim():
    d = L.DiffMaskParams()
    d.p1, d.p2, d.knowledge, d.out, d.pooled_ws, d.N, d.H, d.W, d.scale = 1000, 2000, 3000, 4000, 5000, 2, 4, 8, 4
    _spans(_by_field("chap_diff_mask", d), p1=("R", 1000, 512), p2=("R", 2000, 512), knowledge=("R", 3000, 256), out=("W", 4000, 256),
           pooled_ws=("RW", 5000, (2 * 1 * 2 + 2) * 4))
    s = L.SgdParams()
    s.param, s.grad, s.grad2, s.mom, s.lr, s.n = 1000, 2000, 3000, 4000, 5000, 10
    _spans(_by_field("chap_sgd_step", s), param=("RW", 1000, 40), grad=("RW", 2000, 40), grad2=("RW", 3000, 40), mom=("RW", 4000, 40), lr=("R", 5000, 4))
    c = L.ChannelDropParams()
    c.pool_partial, c.grad_sim, c.u1, c.u2, c.mul1, c.mul2, c.probs_out = 1000, 2000, 3000, 4000, 5000, 6000, 7000
    c.nchunk, c.B, c.U, c.C = 2, 2, 3, 4
    _spans(_by_field("chap_channel_drop", c), pool_partial=("R", 1000, 3 * 2 * 4 * 4), grad_sim=("R", 2000, 16), u1=("R", 3000, 48), u2=("R", 4000, 48),
           mul1=("W", 5000, 5 * 4 * 4), mul2=("W", 6000, 5 * 4 * 4), probs_out=("W", 7000, 48))
    g = L.GradSimParams()
    g.gl, g.gu, g.score, g.C, g.K = 1000, 2000, 3000, 3, 5
    _spans(_by_field("chap_grad_sim", g), gl=("R", 1000, 60), gu=("R", 2000, 60), score=("RW", 3000, 12))


# ---------------------------------------------------------------------------------------------------------------- the opt-in entry points
def _sgd_fields(s, n):
    s.param, s.grad, s.grad2, s.mom, s.lr, s.n = 1000, 2000, 3000, 4000, 5000, n


def test_mean_teacher_optimizer():
    q = L.SgdEmaParams()
    _sgd_fields(q.sgd, 10)
    q.ema, q.coef = 6000, 7000
    _spans(_by_field("chap_sgd_ema_step", q), sgd__param=("RW", 1000, 40), sgd__grad=("RW", 2000, 40), sgd__grad2=("RW", 3000, 40),
           sgd__mom=("RW", 4000, 40), sgd__lr=("R", 5000, 4), ema=("RW", 6000, 40), coef=("R", 7000, 8))        # coef: two fp32 words, a and b
    q.sgd.grad2 = None
    assert "sgd.grad2" not in _by_field("chap_sgd_ema_step", q) and len(_by_field("chap_sgd_ema_step", q)) == 6


def test_gradient_guard_norm_and_guarded_optimizer():
    g = L.GradNormParams()
    g.grad, g.grad2, g.ws, g.state, g.n, g.ring = 2000, 3000, 20000, 9000, 10, 3      # the two buckets of _sgd_fields
    # 512 fp64 partials; the state block: a header of 8 int32 words, then 3 rows of 4 words
    _spans(_by_field("chap_grad_norm", g), grad=("R", 2000, 40), grad2=("R", 3000, 40), ws=("RW", 20000, 512 * 8), state=("RW", 9000, 32 + 3 * 16))
    assert C.sizeof(L.GuardState) == 32 and C.sizeof(L.GuardRow) == 16 and L.GRADNORM_SLOTS == 512
    q = L.SgdGuardParams()
    _sgd_fields(q.se.sgd, 10)
    q.se.ema, q.se.coef, q.state = 6000, 7000, 9000
    _spans(_by_field("chap_sgd_guard_step", q), se__sgd__param=("RW", 1000, 40), se__sgd__grad=("RW", 2000, 40), se__sgd__grad2=("RW", 3000, 40),
           se__sgd__mom=("RW", 4000, 40), se__sgd__lr=("R", 5000, 4), se__ema=("RW", 6000, 40), se__coef=("R", 7000, 8),
           state=("R", 9000, 32))                                                   # the header alone: scale and skip, never a row
    q.se.ema, q.se.coef = None, None                                                # without a teacher: chap_sgd_step's fields and the state
    assert sorted(_by_field("chap_sgd_guard_step", q)) == ["se.sgd.grad", "se.sgd.grad2", "se.sgd.lr", "se.sgd.mom", "se.sgd.param", "state"]
    # the norm launch rewrites what the guarded optimizer reads, and both touch the buckets
    norm, opt = _by_field("chap_grad_norm", g), _by_field("chap_sgd_guard_step", q)
    assert A.intersects(norm["state"][1], opt["state"][1]) and A.intersects(norm["grad"][1], opt["se.sgd.grad"][1])


def _monitor_params():
    """C = 2: a group row is 8 + 5 * 2 = 18 words, a label-map row 4 * 2 = 8 words, 512 partial rows per group and two groups; the logits region is
    2 + 1024 * 18 = 18434 words, the label-map region 2 + 1024 * 8 = 8194 words behind it; a ring row is 1 + 2 * 18 + 2 * 8 + 16 = 69 words."""
    a = L.MonitorParams()
    a.logits[0], a.logits[1], a.labels, a.ws, a.N, a.C, a.P = 1000, 2000, 3000, 100000, 2, 2, 5
    b = L.MonitorLabelsParams()
    b.maps[0], b.maps[1], b.labels, b.ws, b.N, b.C, b.P = 4000, 5000, 3000, 100000, 2, 2, 5
    f = L.MonitorFinalizeParams()
    f.ws, f.ring, f.slot_iter, f.C, f.ring_rows, f.nscalars = 100000, 400000, 6000, 2, 3, 2
    f.scalars[0], f.scalars[1], f.scalars[2] = 7000, 7004, 7008                     # nscalars = 2: the third pointer is not read
    return a, b, f


def test_monitor_accumulate_launches_and_finalize():
    a, b, f = _monitor_params()
    assert (L.MONITOR_HDR, L.MONITOR_SLOTS, L.MONITOR_MAX_SCALARS) == (2, 512, 16)
    acc = _by_field("chap_monitor_accumulate", a)
    _spans(acc, labels=("R", 3000, 2 * 5 * 8), ws=("W", 100000, 18434 * 8))
    assert acc["logits[0]"] == ("R", (1000, 0, 2 * 2 * 5 * 4, 1)) and acc["logits[1]"] == ("R", (2000, 0, 80, 1))
    lab = _by_field("chap_monitor_accumulate_labels", b)
    _spans(lab, labels=("R", 3000, 80), ws=("W", 100000 + 18434 * 8, 8194 * 8))
    assert lab["maps[0]"] == ("R", (4000, 0, 80, 1)) and lab["maps[1]"] == ("R", (5000, 0, 80, 1))
    fin = _by_field("chap_monitor_finalize", f)
    _spans(fin, ws=("R", 100000, (18434 + 8194) * 8), ring=("W", 400000, 3 * 69 * 8), slot_iter=("R", 6000, 8))
    assert fin["scalars[0]"] == ("R", (7000, 0, 4, 1)) and fin["scalars[1]"] == ("R", (7004, 0, 4, 1))
    assert fin["scalars[2]"] == ("R", None)                                         # beyond nscalars: no rule, and the step never sets it
    assert sorted(k for k in fin if k.startswith("scalars")) == ["scalars[0]", "scalars[1]", "scalars[2]"]


def test_the_two_monitor_accumulate_launches_share_a_workspace_without_meeting():
    """One `ws` pointer, two regions: the launches may run on two streams (ChapStep issues the label-map one on pass B's stream), and the
    finalize launch, which reads both regions, needs an order against each."""
    a, b, f = _monitor_params()
    acc, lab, fin = (_by_field(n, p)["ws"][1] for n, p in (("chap_monitor_accumulate", a), ("chap_monitor_accumulate_labels", b), ("chap_monitor_finalize", f)))
    assert a.ws == b.ws == f.ws
    assert not A.intersects(acc, lab) and A.bounds(acc)[1] == A.bounds(lab)[0]       # back to back: no gap, no shared byte
    assert A.intersects(acc, fin) and A.intersects(lab, fin)
    assert A.bounds(fin) == (A.bounds(acc)[0], A.bounds(lab)[1])
    for Cc in range(2, 9):                                                          # every class count the kernels are built for
        a.C = b.C = f.C = Cc
        acc, lab, fin = (_by_field(n, p)["ws"][1] for n, p in (("chap_monitor_accumulate", a), ("chap_monitor_accumulate_labels", b), ("chap_monitor_finalize", f)))
        assert not A.intersects(acc, lab) and A.intersects(acc, fin) and A.intersects(lab, fin), Cc


def test_every_rule_has_a_case_in_this_file():
    """A rule added later without a hand-worked case fails here: every entry point of RULES is named by a test of this module."""
    import inspect
    import sys
    source = inspect.getsource(sys.modules[__name__])
    assert [name for name in A.RULES if '"%s"' % name not in source] == []
