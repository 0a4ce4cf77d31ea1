"""Residual V-Net blocks (has_residual=True), the CPU side: the functional restatement tests/vnet_residual_ref.py against the imported
reference's outputs (tests/golden/vnet_residual_32.npz, tools/gen_golden_residual.py), the constructors and their program, and the C-ABI
boundary of chap_residual_fwd / chap_residual_bwd / chap_grad_sum (argument errors with no launch, struct sizes from the header)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import init as oinit
from tests import vnet_residual_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = (slice(None), slice(None), slice(None, None, 2), slice(None, None, 2), slice(None, None, 2))


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "vnet_residual_32.npz"), allow_pickle=False)


def test_restatement_reproduces_the_reference(fixture):
    """Every array of the fixture within 1e-5 relative (max norm): the same ops in the same order; the BLAS / threading order may differ."""
    g = fixture
    x = torch.from_numpy(g["x"])
    sd = oinit.dual_decoder_3d_state(int(g["state_seed"]))
    sv = oinit.vnet_state(int(g["vnet_state_seed"]))
    with torch.no_grad():
        o1, o2 = rref.dual_decoder_3d(sd, x, train=False, has_dropout=False)
        ov = rref.vnet_3d(sv, x, train=False, has_dropout=False)
        assert relerr(o1, g["eval_logits0"]) < 1e-5 and relerr(o2, g["eval_logits1"]) < 1e-5 and relerr(ov, g["vnet_eval_logits"]) < 1e-5
        t1, t2 = rref.dual_decoder_3d(sd, x, train=True, has_dropout=False)          # updates sd's running statistics, as the module does
        tv = rref.vnet_3d(sv, x, train=True, has_dropout=False)
    assert relerr(t1[SUB], g["train_logits0_sub"]) < 1e-5 and relerr(t2[SUB], g["train_logits1_sub"]) < 1e-5
    assert relerr(tv[SUB], g["vnet_train_logits_sub"]) < 1e-5
    for k in g["bn_layers"]:
        assert relerr(sd[str(k) + ".running_mean"], g["after_rm_" + str(k)]) < 1e-5, k
        assert relerr(sd[str(k) + ".running_var"], g["after_rv_" + str(k)]) < 1e-5, k
    assert int(sd["encoder.block_two.conv.4.num_batches_tracked"]) == 1


def test_residual_and_plain_nets_differ_on_the_fixture(fixture):
    """The fixture discriminates: the plain V-Net with the same weights is far from it."""
    from oracle import nets as onets
    g = fixture
    with torch.no_grad():
        p1, _ = onets.dual_decoder_3d(oinit.dual_decoder_3d_state(int(g["state_seed"])), torch.from_numpy(g["x"]), train=False, has_dropout=False)
    assert relerr(p1, g["eval_logits0"]) > 0.1


def test_restatement_runs_in_fp64_with_injected_masks(fixture):
    g = fixture
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    sd = rref.cast_state(oinit.dual_decoder_3d_state(int(g["state_seed"])), torch.float64)
    masks = oinit.drop_masks_3d(5, 2)
    o1, o2 = rref.dual_decoder_3d(sd, x, train=True, drop=masks, has_dropout=True)
    n1, _ = rref.dual_decoder_3d(rref.cast_state(oinit.dual_decoder_3d_state(int(g["state_seed"])), torch.float64), x, train=True, has_dropout=True)
    assert o1.dtype == torch.float64 and float((o1 - n1).detach().abs().max()) > 0          # the masks act
    (o1.sum() + o2.sum()).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0


def test_constructors_keys_and_program():
    from chap_amd.networks import DualDecoder3d, VNet
    kw = dict(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True)
    for cls, ndec in ((DualDecoder3d, 2), (VNet, 1)):
        m, plain = cls(has_residual=True, **kw), cls(has_residual=False, **kw)
        sd, sp = m.state_dict(), plain.state_dict()
        assert list(sd.keys()) == list(sp.keys()) and [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in sp.values()]
        ops_ = m._exec.prog.ops
        res = [op for op in ops_ if op.kind == "res"]
        assert sum(op.branch == 0 for op in res) == 5
        for b in range(1, ndec + 1):
            assert sum(op.branch == b for op in res) == 4
        assert not any(op.kind == "res" or op.noact for op in plain._exec.prog.ops)
        # the value a 'res' op reads first is a conv + BatchNorm without activation, and nothing else reads that value
        by_out = {op.out: op for op in ops_}
        for op in res:
            last = by_out[op.srcs[0]]
            assert last.noact and last.bn and m._exec.prog.consumers[last.out] == [op]
        assert res[0].srcs == ["b1.last"]                                 # block_one: the image is the block's input
        assert [op.out for op in ops_ if op.drop] == ["b5"] + ["%s.x9" % r for r in (("decoder1", "decoder2") if ndec == 2 else ("decoder",))]
        assert all(op.kind == "res" for op in ops_ if op.drop)            # the Dropout3d sites moved to the 'res' ops
    m = DualDecoder3d(has_residual=True, **kw)
    m.load_state_dict(oinit.dual_decoder_3d_state(3), strict=True)        # a checkpoint of either setting loads into both
    z = m._exec._zipped()
    assert sum(len(p) == 2 and p[0].kind == "res" for p in z) == 4        # the decoders' residual adds pair up into grouped steps


def test_unsupported_configurations():
    from chap_amd.networks import DualDecoder3d, VNet
    for cls in (DualDecoder3d, VNet):
        with pytest.raises(ValueError, match="broadcast"):
            cls(n_channels=3, n_classes=2, normalization="batchnorm", has_residual=True)
        with pytest.raises(NotImplementedError):
            cls(n_channels=1, n_classes=2, normalization="groupnorm", has_residual=True)
        with pytest.raises(NotImplementedError):
            cls(n_channels=1, n_classes=2, normalization="groupnorm")
        cls(n_channels=3, n_classes=2, normalization="batchnorm")          # without residual blocks three channels still build


def test_train_entry_reads_has_residual(tmp_path, monkeypatch):
    """train_ours_3D.train passes args['has_residual'] to the class it builds; without it the factory's network is unchanged.  Host logic only."""
    from chap_amd import train_ours_3D as T
    built = []

    class Stop(Exception):
        pass

    def fake_step(model, a):
        built.append(model)
        raise Stop()

    monkeypatch.setattr(T, "ChapStep", fake_step)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch, "device", lambda *a, **k: "cpu")
    for flag in (True, False):
        with pytest.raises(Stop):
            T.train(dict(has_residual=flag, max_iterations=1), str(tmp_path / ("run%d" % flag)))
    assert any(op.kind == "res" for op in built[0]._exec.prog.ops) and not any(op.kind == "res" for op in built[1]._exec.prog.ops)
    assert type(built[0]).__name__ == type(built[1]).__name__ == "DualDecoder3d"


def _src(L, C=16, ld=None, coff=0, ptr=64, act=0):
    s = L.Src()
    s.ptr, s.C, s.ld, s.coff, s.act = ptr, C, C if ld is None else ld, coff, act
    return s


def _fwd(L, **kw):
    p = L.ResidualParams()
    p.r = _src(L, **{k[2:]: v for k, v in kw.items() if k.startswith("r_")})
    p.src[0] = _src(L)
    p.nsrc, p.out, p.N, p.D, p.H, p.W, p.dtype = 1, 64, 1, 2, 2, 2, L.F32
    for k, v in kw.items():
        if not k.startswith("r_"):
            setattr(p, k, v)
    return p


def _bwd(L, **kw):
    p = L.ResidualBwdParams()
    p.g[0], p.g_ld[0], p.ng, p.out, p.gout = 64, 32, 1, 64, 64
    p.N, p.D, p.H, p.W, p.C, p.dtype = 1, 2, 2, 2, 16, L.F32
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _gsum(L, **kw):
    p = L.GradSumParams()
    for i in range(2):
        p.g[i], p.g_ld[i] = 64, 16
    p.ng, p.out, p.npix, p.C, p.dtype = 2, 64, 8, 16, L.F32
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_argument_errors_without_a_launch():
    """Every check runs before any launch: the pointers are never dereferenced on the host (64 stands for 'not null')."""
    from chap_amd import _lib as L
    for name, st in (("chap_residual_fwd", L.ResidualParams), ("chap_residual_bwd", L.ResidualBwdParams), ("chap_grad_sum", L.GradSumParams)):
        assert name in L._SIGS
        with pytest.raises(L.ChapError, match=name + ": null"):
            L.call(name, st(), 0)
    cases = [("chap_residual_fwd", _fwd(L, r_C=12), "multiple of 8"), ("chap_residual_fwd", _fwd(L, r_act=1), "r.act=1"),
             ("chap_residual_fwd", _fwd(L, nsrc=3), "nsrc=3"), ("chap_residual_fwd", _fwd(L, nsrc=0), "exactly one"),
             ("chap_residual_fwd", _fwd(L, xin=64), "exactly one"), ("chap_residual_fwd", _fwd(L, N=1 << 20, D=1 << 10, H=4, W=1), "32-bit"),
             ("chap_residual_fwd", _fwd(L, r_ld=24, r_coff=12), "8-aligned"),
             ("chap_residual_bwd", _bwd(L, C=20), "multiple of 8"), ("chap_residual_bwd", _bwd(L, ng=0), "ng=0"), ("chap_residual_bwd", _bwd(L, ng=4), "ng=4"),
             ("chap_residual_bwd", _bwd(L, ng=2), r"g\[1\] is null"), ("chap_residual_bwd", _bwd(L, N=1 << 30, D=2, H=1, W=1), "32-bit"),
             ("chap_residual_bwd", _bwd(L, C=24, dxin=64), "power of two"),
             ("chap_grad_sum", _gsum(L, C=4), "multiple of 8"), ("chap_grad_sum", _gsum(L, ng=1), "ng=1"), ("chap_grad_sum", _gsum(L, ng=5), "ng=5"),
             ("chap_grad_sum", _gsum(L, ng=3), r"g\[2\] is null"), ("chap_grad_sum", _gsum(L, npix=1 << 31), "32-bit")]
    for name, p, msg in cases:
        with pytest.raises(L.ChapError, match=name + ".*" + msg):
            L.call(name, p, 0)
    with pytest.raises(L.ChapError, match="g_ld|8-aligned"):
        p = _bwd(L)
        p.g_ld[0], p.g_coff[0] = 16, 8                                   # channels [8, 24) of a 16-channel row
        L.call("chap_residual_bwd", p, 0)
    assert L.lib().chap_abi_version() == L.ABI_VERSION == 9               # additive: no version change


def test_new_structs_match_the_header(tmp_path):
    """sizeof and the offset of the last field of the new structs, from a C program compiled against include/chap_hip.h."""
    from chap_amd import _lib as L
    pairs = {"chap_residual_params": (L.ResidualParams, "dtype"), "chap_residual_bwd_params": (L.ResidualBwdParams, "dtype"),
             "chap_grad_sum_params": (L.GradSumParams, "dtype")}
    c = tmp_path / "sz.c"
    body = "".join('printf("%s %%zu %%zu\\n", sizeof(%s), offsetof(%s, %s));\n' % (n, n, n, f) for n, (_, f) in pairs.items())
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        name, size, off = line.split()
        st, f = pairs[name]
        assert int(size) == ctypes.sizeof(st), (name, size, ctypes.sizeof(st))
        assert int(off) == getattr(st, f).offset, (name, off)


def test_more_than_three_contributions_fold_the_oldest_first():
    """The executor's fold of a value's gradient contributions (engine.fold_oldest_first, used by backward's incoming3): chap_act_bwd_* and
    chap_residual_bwd take three, chap_grad_sum up to four.  A skip feature of a residual DualDecoder3d has five -- the down conv and, per decoder,
    the block's first conv and its residual add, in program order: ((c0 + c1) + c2) by chap_grad_sum, then ((t + c3) + c4) in the consumer.
    Symbolic summands here; the per-launch values are checked in tests/test_step_launches_gpu.py."""
    from chap_amd.engine import fold_oldest_first
    calls = []

    def fold(group):
        calls.append(list(group))
        return tuple(group)

    assert fold_oldest_first(None, fold) is None and fold_oldest_first([], fold) == [] and fold_oldest_first([0, 1, 2], fold) == [0, 1, 2] and not calls
    assert fold_oldest_first([0, 1, 2, 3], fold) == [(0, 1), 2, 3]
    assert fold_oldest_first([0, 1, 2, 3, 4], fold) == [(0, 1, 2), 3, 4]
    assert fold_oldest_first([0, 1, 2, 3, 4, 5], fold) == [(0, 1, 2, 3), 4, 5]
    assert fold_oldest_first(list(range(8)), fold) == [((0, 1, 2, 3), 4, 5), 6, 7]              # two launches: four, then the sum and two more
    assert all(2 <= len(g) <= 4 for g in calls)                                                  # what chap_grad_sum accepts
    # the net that needs it: every skip feature of the residual DualDecoder3d is read by five ops, block outputs elsewhere by fewer
    from chap_amd.networks.vnet import build_program
    prog = build_program(2, 16, [("decoder1", 0), ("decoder2", 0)], True, has_residual=True)
    readers = {}
    for op in prog.ops:
        for sname in op.srcs:
            readers[sname] = readers.get(sname, 0) + 1
    assert sorted(readers.values())[-4:] == [5, 5, 5, 5] and max(readers.values()) == 5
