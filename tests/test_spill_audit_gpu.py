"""The conv_fwd_kernel instances whose register allocation the spill audit changed (csrc/conv_kernel.h: epilogue offsets pinned to their point of use,
the staging wave index as a scalar, bias / statistics shift in LDS for the 2D k2 s2 instances with 64 output channels per block), at the smallest
grids on which they can go wrong, per element against the fp64 restatements of tests/kernel_ref.py under the bounds of tests/k3_conv_cases.py /
tests/small_conv_cases.py (kernel_ref.conv_bound, stats_ref):

* 2D k2 s2, bf16: 64 -> 64 (two K chunks, one full NT 4 group) and 32 -> 128 (two NT groups); N = 2 on a 6 x 10 output grid (ragged against the
  8 x 16 tile: one partial tile per image) and N = 1 at 9 x 17 (a second tile in both directions); plain and lazy (BatchNorm affine + LeakyReLU)
  sources, with bias and the statistics epilogue -- the values that moved to LDS;
* 1x1 + depth-to-space: 32 -> 4 x 16 and 64 -> 4 x 32 on 5 x 9 and 8 x 16 inputs (grids this small plan one channel tile per block, NT 1 MR 1; the
  NT 4 instances of the family run in tests/test_small_conv_families_gpu.py, d2s_128_64_mr1 / _mr2);
* 3D bricks on staged weights: 64 -> 64 and 64 add 64 -> 64 at 5 x 6 x 18 (ragged in all three brick dimensions) and 4 x 4 x 16 (one brick), N = 1.

Outputs sit in a channel slot of a wider NaN buffer with a NaN guard behind it, the statistics slots are NaN before the launch.  The first test
(no GPU) asks the host-only planner that every case reaches the (KC, NT, MR) it names."""
import time

import pytest
import torch

from tests import k3_conv_cases as kc
from tests import kernel_ref as kr
from tests import small_conv_cases as sc
from tests.plan_probe import KNOBS, probe                  # noqa: F401 (fixture)

DEV, DT = "cuda", "bf16"
CF, DF = kr.PACK_CONV_FWD, kr.PACK_DECONV_FWD

# ---- 2D k2 s2 and depth-to-space: rows of tests/small_conv_cases.py's table (grid = the launch's output grid; d2s: the coarse grid)
K2_GRIDS = ((2, (6, 10)), (1, (9, 17)))
SMALL = []
for cin, cout, chunks in ((64, 64, 2), (32, 128, 1)):
    for N, grid in K2_GRIDS:
        for src in ("p", "ar"):
            SMALL.append(sc._fwd("k2_%d_%d_n%d_%s" % (cin, cout, N, src), "k2", 2, N, grid, cin, cout, (32, 4, 2), CF, src, stats=True, chunks=chunks))
for cin, cout in ((32, 16), (64, 32)):
    for grid in ((5, 9), (8, 16)):
        SMALL.append(sc._fwd("d2s_%d_%d_%dx%d" % (cin, cout, *grid), "d2s", 2, 2, grid, cin, cout, (32, 1, 1), DF, "ar", stats=True, chunks=cin // 32))
SMALL_BY_NAME = {c["name"]: c for c in SMALL}

# ---- 3D bricks on staged weights: rows of tests/k3_conv_cases.py's table
BRICK = []
for grid in ((5, 6, 18), (4, 4, 16)):
    tag = "x".join(map(str, grid))
    BRICK.append(kc._fwd("b3_64_64_" + tag, 3, 1, grid, 64, 64, (16, 2, 4), "ar", kc.gen(2, 4), stats=True, dts=kc.BF, wlds={"bf16": False}))
    BRICK.append(kc._fwd("b3_add_64_64_" + tag, 3, 1, grid, (64, 64), 64, (16, 2, 4), ("ar", "sl"), kc.gen(2, 4), arr="add", stats=True, dts=kc.BF,
                         wlds={"bf16": False}))
BRICK_BY_NAME = {c["name"]: c for c in BRICK}


def test_every_case_plans_the_instance_it_names(probe):
    plans = probe([sc.fwd_request(c, DT) for c in SMALL])
    for c, p in zip(SMALL, plans):
        assert p["rc"] == 0 and p["route"] == "generic", (c["name"], p)
        assert (p["KC"], p["NT"], p["MR"], p["nchunks"]) == c["plan"] + (c["chunks"],), (c["name"], p)
    for c in BRICK:
        p = probe([kc.setenv_line(c), kc.fwd_request(c, DT)])[0]
        assert p["rc"] == 0 and p["route"] == "generic" and (p["KC"], p["NT"], p["MR"]) == c["plan"], (c["name"], p)
        assert kc.case_lds(c, DT)[0] is False, c["name"] + ": the weights are resident"
        assert kc.fwd_instance(c, DT) == "conv_fwd_kernel<bf16,3,1,true,16,2,4,%s,false,true,%s>" % (("true", "false") if c["arr"] == "add" else ("false", "true"))


def nan_stats(ops, clog):
    st = ops.stats_buffer(clog, DEV)
    st.fill_(float("nan"))
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SMALL_BY_NAME))
def test_k2s2_and_depth_to_space(name):
    from chap_amd import ops
    from tests.test_small_conv_families_gpu import g4, lazy_of
    t0 = time.perf_counter()
    c, dtype = SMALL_BY_NAME[name], sc.DTYPES[DT]
    inp = sc.fwd_inputs(c, DT)
    srcs = [lazy_of(s, dtype) for s in inp["srcs"]]
    wp = ops.pack_weights(inp["w"].to(DEV), c["kind"], dtype, *sc.pack_args(c))
    flat, out = sc.new_out(c, dtype, DEV)
    Cl, M = sc.launch_cout(c), c["cout"]
    stats = nan_stats(ops, Cl)
    k = 2 if c["op"] == "k2" else 1
    kw = dict(out_ld=out.shape[-1], out_coff=sc.SLOT_COFF)
    if c["op"] == "d2s":
        kw.update(out_mode=1, out_cn=M)
    ops.conv_fwd(srcs, wp, inp["bias"].to(DEV), Cl, out, grid=(c["N"],) + g4(c["grid"]), in_dims=g4(sc.in_spatial(c)), ksize=k, stride=k, dims=2, stats=stats,
                 stats_shift=inp["shift"].to(DEV), **kw)
    torch.cuda.synchronize()
    slots = int(stats[:1].view(torch.int32).item())
    totals = ops.stats_totals(stats, Cl, M).cpu()
    worst = sc.fwd_check(c, DT, sc.fwd_reference(c, DT, inp), flat.cpu(), totals)
    print("spill audit %-22s KC%d NT%d MR%d slots %d: worst err/bound %s  (%.2f s)" % (name, *c["plan"], slots, " ".join("%.3f" % v for v in worst), time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BRICK_BY_NAME))
def test_staged_bricks_3d(name, monkeypatch):
    from chap_amd import ops
    from tests.test_small_conv_families_gpu import lazy_of
    t0 = time.perf_counter()
    c, dtype = BRICK_BY_NAME[name], kc.DTYPES[DT]
    inp = kc.fwd_inputs(c, DT)
    srcs = [lazy_of(s, dtype) for s in inp["srcs"]]
    wp = ops.pack_weights(inp["w"].to(DEV), c["kind"], dtype, *kc.pack_args(c))
    M = c["cout"]
    D, H, W = kc.spatial(c)
    for k_ in KNOBS:
        monkeypatch.delenv(k_, raising=False)
    for k_, v in c["knobs"].items():
        monkeypatch.setenv(k_, str(v))
    outs = kc.new_outs(c, DT, DEV)
    out = outs[0][1]
    stats = nan_stats(ops, M)
    ops.conv_fwd(srcs, wp, inp["bias"].to(DEV), M, out, grid=(c["N"], D, H, W), in_dims=(D, H, W), ksize=3, stride=1, dims=3, combine=int(c["arr"] == "add"),
                 stats=stats, stats_shift=inp["shift"].to(DEV), out_ld=out.shape[-1], out_coff=sc.SLOT_COFF)
    torch.cuda.synchronize()
    totals = ops.stats_totals(stats, M).cpu()
    worst = kc.fwd_check(c, DT, kc.fwd_reference(c, DT, inp), [f.cpu() for f, _ in outs], totals)
    print("spill audit %-22s %s: worst err/bound %s  (%.2f s)" % (name, kc.fwd_instance(c, DT), " ".join("%.3f" % v for v in worst), time.perf_counter() - t0))
