"""Bitwise A/B of the MFMA convolution family (chap_conv_fwd, chap_conv_c1_fwd, chap_wgrad) between two builds (CHAP_LIBPATH):
run `save PATH` under each build, then `cmp A B` (CPU only).  Saved per case: the raw bytes of every output tensor and the raw statistics
buffer (header word + the slots in use); for the weight-gradient cases dW and db.  The cases are small, ragged (non-`full` paths) and give a
block several items; each kernel of the family and each of its routes is reached through the library's own knobs, and every conv case asks
the host-only planner (conv_plan.h, through the probe of tests/test_launch_plan_cpu.py) which route it takes: a case that is not planned onto
the kernel it names stops the run."""
import os, subprocess, sys, tempfile
sys.path.insert(0, os.getcwd())
import torch

GENERIC = {"CHAP_CONV_WP": "0", "CHAP_CONV_KPAR": "0"}        # conv_fwd_kernel whatever the planner would pick
BF, F32 = torch.bfloat16, torch.float32


def planner():
    """request line -> dict of the plan (route, KC, NT, MR, cpar, ...), under the knobs of the environment at the time of the call"""
    from tests.plan_probe import PROBE, ROOT, CSRC
    d = tempfile.mkdtemp(prefix="plan_probe")
    open(os.path.join(d, "probe.cpp"), "w").write(PROBE)
    exe = os.path.join(d, "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(d, "probe.cpp"), "-o", exe], check=True)

    def plan(request):
        line = subprocess.run([exe], input=request + "\n", check=True, capture_output=True, text=True).stdout.strip()
        assert line.startswith("rc=0 "), (request, line)
        return dict(t.split("=") for t in line.split()[1:])
    return plan


def run_cases():
    from chap_amd import _lib as L, ops
    plan = planner()
    dev = "cuda"
    g = torch.Generator().manual_seed(5)
    out = {}

    def rnd(*shape, dtype=F32):
        return torch.randn(*shape, generator=g).to(dev).to(dtype)

    def lazy(N, sp, c, dtype, affine=True, keep=False, chan_mul=False):
        x = rnd(N, *sp, c, dtype=dtype)
        if not affine:
            return ops.Lazy(x)
        km = (torch.rand(N, *sp, c, generator=g) > 0.3).to(torch.uint8).to(dev) if keep else None
        cm = ((torch.rand(N, c, generator=g) > 0.3).float() * 1.5).to(dev) if chan_mul else None
        return ops.Lazy(x, (torch.rand(c, generator=g) + 0.5).to(dev), (torch.randn(c, generator=g) * 0.1).to(dev), True, 0.01,
                        keep=km, keep_scale=1.25 if keep else 1.0, chan_mul=cm)

    def raw(t):
        return t.contiguous().view(torch.uint8).cpu().clone()

    def stats_raw(st, clog):
        n = int(st[:1].view(torch.int32).item())
        return raw(st[:L.STATS_HDR + n * 2 * clog])

    def env(knobs):
        old = {k: os.environ.get(k) for k in knobs}
        os.environ.update(knobs)
        return old

    def unenv(old):
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def conv(name, srcs, cin, cout, grid, in_dims, dtype, *, route="generic", ksize=3, stride=1, dims=2, knobs=GENERIC, kind=None, taps=None, bias=True,
             stats=True, clog=None, outs=None, **kw):
        """One chap_conv_fwd launch; clog: logical output channels (transposed convs: sub-lattices x real channels); route: the planned route it
        has to take, "kpar2" / "kpar4" with the number of chunks side by side."""
        clog = cout if clog is None else clog
        taps = ksize ** dims if taps is None else taps
        wshape = {None: [cout, cin] + [ksize] * dims}.get(kind, [cin, cout] + [2] * dims)
        w = torch.randn(*wshape, generator=g).to(dev) / (cin * taps) ** 0.5
        wp = ops.pack_weights(w, L.PACK_CONV_FWD if kind is None else kind, dtype, cin, cout, taps)
        nb = cout if kind is not None else clog
        b = (torch.randn(nb, generator=g) * 0.1).to(dev) if bias else None
        st = ops.stats_buffer(clog, dev) if stats else None
        sh = (torch.randn(nb, generator=g) * 0.1).to(dev) if stats else None
        if outs is None:
            outs = [torch.full((*grid, clog), float("nan"), device=dev, dtype=dtype)]
        old = env(knobs)
        try:
            assert len(outs) == 1 or route != "kpar"          # (the probe has no out2; only the K-parallel route asks for it)
            q = plan("conv dims=%d k=%d s=%d N=%d D=%d H=%d W=%d Cout=%d nsrc=%d combine=%d C0=%d C1=%d dtype=%d keep0=%d keep1=%d cm0=%d cm1=%d d2s=%d Cn=%d planar=%d "
                     "f32out=%d stats=%d" % (dims, ksize, stride, *grid, clog, len(srcs), kw.get("combine", 0), srcs[0].C, srcs[1].C if len(srcs) > 1 else 0,
                                             L.F32 if dtype == F32 else L.BF16, srcs[0].keep is not None, len(srcs) > 1 and srcs[1].keep is not None,
                                             srcs[0].chan_mul is not None, len(srcs) > 1 and srcs[1].chan_mul is not None, kw.get("out_mode", 0), kw.get("out_cn", 0),
                                             kw.get("out_planar", False), kw.get("out_f32", False), stats))
            got = q["route"] + (q["cpar"] if q["route"] == "kpar" else "")
            assert got == route, "%s: planned onto %s, not %s (%s)" % (name, got, route, q)
            name = "%s [%s KC%s NT%s MR%s]" % (name, got, q["KC"], q["NT"], q["MR"])
            ops.conv_fwd(srcs, wp, b, clog, outs[0], grid=grid, in_dims=in_dims, ksize=ksize, stride=stride, dims=dims, stats=st, stats_shift=sh,
                         out2=outs[1] if len(outs) > 1 else None, **kw)
            torch.cuda.synchronize()
        finally:
            unenv(old)
        out[name] = [raw(o) for o in outs] + ([stats_raw(st, clog)] if stats else [])

    def tname(dtype):
        return str(dtype)[6:]

    # ---- generic 2D k3 (conv_fwd_kernel), both dtypes
    for dtype in (BF, F32):
        t = tname(dtype)
        for (N, hw, cin, cout) in ((4, (250, 254), 16, 16), (12, (62, 66), 64, 64), (6, (126, 130), 32, 16)):
            conv("generic2d %s %d->%d %dx%dx%d" % (t, cin, cout, N, *hw), [lazy(N, (1, *hw), cin, dtype)], cin, cout, (N, 1, *hw), (1, *hw), dtype)
        for (c0, c1) in ((16, 16), (24, 8)):          # two concatenated sources; 24 + 8: the chunk straddles them (lane select)
            conv("generic2d %s concat %d+%d" % (t, c0, c1), [lazy(3, (1, 37, 52), c0, dtype, keep=True), lazy(3, (1, 37, 52), c1, dtype)], c0 + c1, 32,
                 (3, 1, 37, 52), (1, 37, 52), dtype)
        conv("generic2d %s out2 16->32" % t, [lazy(3, (1, 40, 33), 16, dtype)], 16, 32, (3, 1, 40, 33), (1, 40, 33), dtype,
             outs=[torch.full((3, 1, 40, 33, 16), float("nan"), device=dev, dtype=dtype) for _ in range(2)])
        conv("generic2d %s add-combine" % t, [lazy(2, (1, 20, 24), 16, dtype, chan_mul=True), lazy(2, (1, 20, 24), 16, dtype, affine=False)], 16, 16,
             (2, 1, 20, 24), (1, 20, 24), dtype, combine=1)
        # ---- other geometries
        # (32 input channels: a 16-channel bf16 head takes conv_head1x1_kernel, which is not of this family)
        conv("1x1 %s planar head" % t, [lazy(2, (1, 10, 18), 32, dtype)], 32, 4, (2, 1, 10, 18), (1, 10, 18), dtype, ksize=1, stats=False,
             outs=[torch.full((2, 4, 10, 18), float("nan"), device=dev)], out_planar=True, out_f32=True)
        conv("1x1 %s Cout 20" % t, [lazy(2, (1, 10, 18), 32, dtype)], 32, 20, (2, 1, 10, 18), (1, 10, 18), dtype, ksize=1)
        conv("k2s2 %s 2D" % t, [lazy(2, (1, 26, 40), 16, dtype)], 16, 32, (2, 1, 13, 20), (1, 26, 40), dtype, ksize=2, stride=2)
        conv("k2s2 %s 3D" % t, [lazy(1, (18, 26, 40), 16, dtype)], 16, 32, (1, 9, 13, 20), (18, 26, 40), dtype, ksize=2, stride=2, dims=3)
        conv("depth-to-space %s 2D" % t, [lazy(2, (1, 13, 20), 64, dtype)], 64, 32, (2, 1, 13, 20), (1, 13, 20), dtype, ksize=1, kind=L.PACK_DECONV_FWD, taps=4,
             clog=4 * 32, outs=[torch.full((2, 1, 26, 40, 32), float("nan"), device=dev, dtype=dtype)], out_mode=1, out_cn=32)
        conv("depth-to-space %s 3D" % t, [lazy(1, (9, 13, 20), 64, dtype)], 64, 32, (1, 9, 13, 20), (9, 13, 20), dtype, ksize=1, dims=3, kind=L.PACK_DECONV_FWD,
             taps=8, clog=8 * 32, outs=[torch.full((1, 18, 26, 40, 32), float("nan"), device=dev, dtype=dtype)], out_mode=1, out_cn=32)
    # ---- generic 3D k3: the routes of tests/test_kernels_gpu.py CONV3D_ROUTES, add-combine on bricks
    for route, shape, c, knobs in (("brick64", (3, 10, 14, 14), 64, {"CHAP_CONV_KPAR": "0", "CHAP_CONV_MR": "4", "CHAP_CONV_NT": "2"}),
                                   ("slab64", (3, 10, 14, 14), 64, {"CHAP_CONV_KPAR": "0"}), ("kpar128", (2, 10, 14, 14), 128, {"CHAP_CONV_KPAR": "1"})):
        conv("3d %s" % route, [lazy(shape[0], shape[1:], c, BF, chan_mul=True)], c, c, shape, shape[1:], BF, dims=3, knobs=knobs,
             route="kpar4" if route == "kpar128" else "generic")
    # ---- the instances on staged weights with 64 output channels per block: 2D k2 s2 (two K chunks; 32 -> 128: two channel groups), the V-Net skip add on bricks
    conv("k2s2 bf16 2D 64->64 staged", [lazy(2, (1, 30, 44), 64, BF)], 64, 64, (2, 1, 15, 22), (1, 30, 44), BF, ksize=2, stride=2)
    conv("k2s2 bf16 2D 32->128 staged", [lazy(2, (1, 30, 44), 32, BF, keep=True)], 32, 128, (2, 1, 15, 22), (1, 30, 44), BF, ksize=2, stride=2)
    conv("3d bricks add-combine 64+64 staged", [lazy(1, (10, 14, 30), 64, BF, chan_mul=True), lazy(1, (10, 14, 30), 64, BF, affine=False)], 64, 64, (1, 10, 14, 30),
         (10, 14, 30), BF, dims=3, combine=1, knobs={"CHAP_CONV_KPAR": "0", "CHAP_CONV_MR": "4", "CHAP_CONV_NT": "2"})
    conv("3d bricks add-combine", [lazy(2, (12, 18, 30), 16, BF, chan_mul=True), lazy(2, (12, 18, 30), 16, BF, affine=False)], 16, 16, (2, 12, 18, 30), (12, 18, 30),
         BF, dims=3, combine=1, knobs={"CHAP_CONV_KPAR": "0"})
    # ---- wave-private (conv_wp_kernel): the parameter sets of test_conv_wave_private_2d
    for (cins, cout, hw, keep, split) in (([16], 16, (37, 52), True, False), ([16], 32, (40, 33), False, True), ([32], 32, (24, 40), False, False),
                                         ([16, 16], 16, (19, 50), True, False), ([32], 64, (21, 36), False, False)):
        srcs = [lazy(3, (1, *hw), c, BF, keep=keep and i == 0) for i, c in enumerate(cins)]
        outs = [torch.full((3, 1, *hw, cout // 2), float("nan"), device=dev, dtype=BF) for _ in range(2)] if split else None
        conv("wave-private %s->%d %dx%d" % ("+".join(map(str, cins)), cout, *hw), srcs, sum(cins), cout, (3, 1, *hw), (1, *hw), BF, knobs={"CHAP_CONV_WP": "1"}, outs=outs,
             route="wp")
    # ---- K-parallel: 3D cpar 2 and 4 (16-channel chunks: 96 channels = 6 chunks take two side by side, 64 and 128 four), 2D single round /
    # two rounds / two sources, and two chunks side by side
    kp = {"CHAP_CONV_KPAR": "1"}
    conv("kpar 3d cpar2", [lazy(2, (9, 13, 20), 96, BF, chan_mul=True)], 96, 96, (2, 9, 13, 20), (9, 13, 20), BF, dims=3, knobs=kp, route="kpar2")
    conv("kpar 3d cpar4 one round", [lazy(2, (9, 13, 20), 64, BF, chan_mul=True)], 64, 64, (2, 9, 13, 20), (9, 13, 20), BF, dims=3, knobs=kp, route="kpar4")
    conv("kpar 3d cpar4", [lazy(2, (10, 14, 14), 128, BF, chan_mul=True)], 128, 128, (2, 10, 14, 14), (10, 14, 14), BF, dims=3, knobs=kp, route="kpar4")
    conv("kpar 2d single", [lazy(4, (1, 30, 34), 128, BF, keep=True)], 128, 128, (4, 1, 30, 34), (1, 30, 34), BF, knobs=kp, route="kpar4")
    conv("kpar 2d two rounds", [lazy(4, (1, 16, 16), 256, BF, keep=True)], 256, 256, (4, 1, 16, 16), (1, 16, 16), BF, knobs=kp, route="kpar4")
    conv("kpar 2d 128+128", [lazy(4, (1, 17, 40), 128, BF, keep=True), lazy(4, (1, 17, 40), 128, BF)], 256, 128, (4, 1, 17, 40), (1, 17, 40), BF, knobs=kp,
         route="kpar4")
    conv("kpar 2d cpar2", [lazy(2, (1, 20, 24), 64, BF, keep=True)], 64, 64, (2, 1, 20, 24), (1, 20, 24), BF, knobs=kp, route="kpar2")
    # ---- first conv (conv_c1_mfma_kernel) with statistics
    for shape in ((3, 1, 37, 90), (1, 9, 21, 70)):
        dims = 3 if shape[1] > 1 else 2
        x = torch.rand(*shape, generator=g).to(dev)
        w = (torch.randn(16, 3 ** dims, generator=g) / 3).to(dev)
        o = torch.full((*shape, 16), float("nan"), device=dev, dtype=BF)
        st = ops.stats_buffer(16, dev)
        ops.conv_c1_fwd(x, w, (torch.randn(16, generator=g) * 0.1).to(dev), o, dims=dims, stats=st, stats_shift=(torch.randn(16, generator=g) * 0.1).to(dev))
        torch.cuda.synchronize()
        out["first conv %s" % "x".join(map(str, shape))] = [raw(o), stats_raw(st, 16)]
    # ---- weight gradient: wave-private 2D, 3D bricks and slabs
    def wgrad(name, srcs, cin, cout, grid, dims, knobs, combine=0):
        gy = ops.Lazy(rnd(*grid, cout, dtype=BF))
        dw = torch.full([cout, cin] + [3] * dims, 0.5, device=dev)
        db = torch.zeros(cout, device=dev)
        old = env(knobs)
        try:
            q = plan("wgrad dims=%d k=3 s=1 N=%d D=%d H=%d W=%d na=%d combine=%d C0=%d C1=%d Cb=%d keep0=%d cm0=%d" % (
                dims, *grid, len(srcs), combine, srcs[0].C, srcs[1].C if len(srcs) > 1 else 0, cout, srcs[0].keep is not None, srcs[0].chan_mul is not None))
            assert q["brick"] == ("2" if dims == 2 else knobs["CHAP_WGRAD_BRICK"]), (name, q)          # 2: the wave-private kernel
            name = "%s [brick %s KC%s bn%s mr%s nsplit %s]" % (name, q["brick"], q["KC"], q["bn"], q["mr"], q["nsplit"])
            ops.wgrad(srcs, gy, dw, (1, 3 ** dims, cin * 3 ** dims), grid=grid, in_dims=grid[1:], ksize=3, stride=1, dims=dims, combine=combine, db=db)
            torch.cuda.synchronize()
        finally:
            unenv(old)
        out[name] = [raw(dw), raw(db)]

    wgrad("wgrad_wp 16->16", [lazy(4, (1, 61, 70), 16, BF, keep=True)], 16, 16, (4, 1, 61, 70), 2, {"CHAP_WGRAD_WP": "1"})
    wgrad("wgrad_wp 16+16->16", [lazy(4, (1, 61, 70), 16, BF, keep=True), lazy(4, (1, 61, 70), 16, BF)], 32, 16, (4, 1, 61, 70), 2, {"CHAP_WGRAD_WP": "1"})
    for brick in (1, 0):
        wgrad("wgrad 3d %s" % ("bricks" if brick else "slabs"), [lazy(2, (12, 18, 30), 16, BF, chan_mul=True)], 16, 16, (2, 12, 18, 30), 3, {"CHAP_WGRAD_BRICK": str(brick)})
    return out


if sys.argv[1] == "save":
    torch.save(run_cases(), sys.argv[2])
else:
    a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    assert list(a) == list(b), "the two files hold different cases"
    bad = 0
    for k in a:
        assert len(a[k]) == len(b[k]), "%s: %d and %d tensors" % (k, len(a[k]), len(b[k]))
        nds = [int((x != y).sum()) if x.shape == y.shape else max(x.numel(), y.numel()) for x, y in zip(a[k], b[k])]
        bad += sum(nds) != 0
        print("%-44s %d differing bytes (per tensor %s of %s)" % (k, sum(nds), "+".join(map(str, nds)), "+".join(str(x.numel()) for x in a[k])))
    print("%d cases, %d differ" % (len(a), bad))
    sys.exit(1 if bad else 0)
