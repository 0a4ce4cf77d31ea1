// The launch plan of chap_conv_fwd and the K-side blocking it shares with the weight packer: argument checks, blocking, geometry family,
// (NT, MR) heuristics and the routing to the special kernels, as integer arithmetic on the params struct.  Host-only (no HIP): conv_api.hip
// makes the plan and the launchers consume it; what needs the device (occupancy, CU count, resident-weights fit) stays in conv_dispatch.inc.
#pragma once
#include "host.h"
#include "knobs.h"

enum conv_route { CONV_ROUTE_HEAD, CONV_ROUTE_WP, CONV_ROUTE_KPAR, CONV_ROUTE_GENERIC };
struct conv_blocking { int KC, GPT, NP, STEPS, nchunks, ntiles; };
// NT = 16-channel tiles per block, MR = 16-pixel rows per wave: the template arguments of the instance the route launches
// (head: unused); cpar = K-chunks side by side (K-parallel route only)
struct conv_plan { conv_route route; int geom; conv_blocking b; int NT, MR, cpar; };

// K-side geometry shared by the packer and the kernel: Ck = GEMM-K channels, taps = kernel taps.
static inline conv_blocking conv_blocking_for(int Ck, int taps, int Cout_logical) {
    conv_blocking b;
    b.KC = (Ck >= 32 && Ck % 32 == 0) ? 32 : 16;      // e.g. 16 + 32 concatenated channels (unet_3D) walk in chunks of 16
    // (tried in round 2: 64-channel chunks for the deep 2D layers, to halve the chain of dependent chunk round trips of a tile --
    //  weights then stream from L2 to keep two blocks per CU; single layers -0..6 %, the whole 2D iteration 7.83 -> 8.26 ms: dropped)
    // 3D 3x3x3 with <= 32 input channels (the large-volume levels): chunks of 16 keep the 6x6x18 halo brick at 41 KB
    // (two buffers), which leaves LDS for the staged weights and registers for a pipelined tap loop: 32->16 at
    // 80x112x112 runs 1.9x faster than with KC = 32 (weights streamed from L2 inside the tap loop)
    // 3D 3x3x3: 16-channel chunks for EVERY layer (round 1: only for 32 input channels, from stand-alone timings; on the whole iteration:
    // CHAP_CONV_KC16_MAXC = 32 / 64 / 128 / 256 -> 16.18 / 16.00 / 15.49 / 15.37 ms per 3D step -- half the halo LDS per block, more
    // blocks per CU beside the kernels of the other streams).  Lab knobs, read once: the pack and the conv get the same value.
    if (taps == 27 && Ck >= 32 && Ck <= chap_knob(KNOB_CONV_KC16_MAXC)) b.KC = 16;
    if (taps == 9 && Ck >= 32 && Ck <= chap_knob(KNOB_CONV_KC16_MAXC2D)) b.KC = 16;
    b.GPT = b.KC / 8;
    b.NP = taps * b.GPT;
    b.STEPS = (b.NP + 3) / 4;
    b.nchunks = Ck / b.KC;
    b.ntiles = (Cout_logical + 15) / 16;
    return b;
}

static inline int conv_check_src(const chap_src_t& s, const char* what) {
    CHAP_CHECK_ARG(s.ptr != nullptr, "%s: null tensor", what);
    CHAP_CHECK_ARG(s.C > 0 && s.C % 8 == 0, "%s: C=%d must be a positive multiple of 8", what, s.C);
    CHAP_CHECK_ARG(s.ld >= s.coff + s.C && s.ld % 8 == 0 && s.coff % 8 == 0, "%s: ld=%d coff=%d C=%d not 8-aligned / too small", what, s.ld, s.coff, s.C);
    CHAP_CHECK_ARG((s.scale == nullptr) == (s.shift == nullptr), "%s: scale and shift must come together", what);
    return CHAP_OK;
}

static inline int conv_make_plan(const chap_conv_params* p, conv_plan* q) {
    CHAP_CHECK_ARG(p != nullptr, "chap_conv_fwd: null params");
    CHAP_CHECK_ARG(p->nsrc == 1 || p->nsrc == 2, "chap_conv_fwd: nsrc=%d", p->nsrc);
    for (int i = 0; i < p->nsrc; ++i) { int r = conv_check_src(p->src[i], "chap_conv_fwd src"); if (r) return r; }
    CHAP_CHECK_ARG(p->combine == 0 || (p->nsrc == 1 || p->src[0].C == p->src[1].C), "chap_conv_fwd: add-combine needs equal C");
    // (the staging of an add-combined pair applies keep mask and channel multipliers of the FIRST source only: conv_kernel.h halo_commit_impl)
    if (p->combine == 1 && p->nsrc == 2 && (p->src[1].keep || p->src[1].chan_mul)) { chap_set_error("chap_conv_fwd: add-combine takes a keep mask / channel multipliers on the first source only"); return CHAP_EUNSUPPORTED; }
    CHAP_CHECK_ARG(p->N > 0 && p->D > 0 && p->H > 0 && p->W > 0, "chap_conv_fwd: empty grid");
    CHAP_CHECK_ARG(p->dims == 2 || p->dims == 3, "chap_conv_fwd: dims=%d", p->dims);
    CHAP_CHECK_ARG(p->wpacked && p->out && p->Cout > 0, "chap_conv_fwd: null weights/out");
    const int sd = p->dims == 3 ? p->stride : 1;
    CHAP_CHECK_ARG(p->ID == (p->stride == 1 ? p->D : p->D * sd) && p->IH == p->H * p->stride && p->IW == p->W * p->stride,
                   "chap_conv_fwd: input dims (%d,%d,%d) do not match grid (%d,%d,%d) stride %d", p->ID, p->IH, p->IW, p->D, p->H, p->W, p->stride);
    if (p->dims == 3 && (p->src[0].keep || (p->nsrc > 1 && p->src[1].keep))) { chap_set_error("chap_conv_fwd: element keep masks are built for 2D only (3D: channel multipliers)"); return CHAP_EUNSUPPORTED; }
    if (p->out_mode == 1) CHAP_CHECK_ARG(p->out_Cn > 0 && p->out_Cn % 16 == 0 && p->Cout % p->out_Cn == 0, "chap_conv_fwd: depth-to-space needs Cn%%16==0");
    if (!p->out_planar) CHAP_CHECK_ARG(p->out_ld % 4 == 0 && p->out_coff % 4 == 0, "chap_conv_fwd: out_ld/out_coff must be multiples of 4");
    if (p->out2) CHAP_CHECK_ARG(p->out_mode == 0 && !p->out_planar && !p->out_f32 && (p->Cout & 3) == 0 && p->out2_from > 0 && p->out2_from % 16 == 0 && p->out2_from < p->Cout &&
                                p->ksize == 3 && p->stride == 1, "chap_conv_fwd: out2 needs a channel-last k3 s1 output, out2_from %% 16 == 0 inside (0, Cout)");
    const int Ck = p->combine == 0 ? p->src[0].C + (p->nsrc > 1 ? p->src[1].C : 0) : p->src[0].C;
    const int taps = p->ksize * p->ksize * (p->dims == 3 ? p->ksize : 1);
    const conv_blocking b = q->b = conv_blocking_for(Ck, taps, p->Cout);
    CHAP_CHECK_ARG(Ck % b.KC == 0, "chap_conv_fwd: K channels %d not a multiple of %d", Ck, b.KC);
    // geometry family
    const bool d3 = p->dims == 3;
    int geom;
    if (p->ksize == 3 && p->stride == 1) geom = d3 ? 2 : 1;
    else if (p->ksize == 1 && p->stride == 1) geom = 3;
    else if (p->ksize == 2 && p->stride == 2) geom = d3 ? 5 : 4;
    else { chap_set_error("chap_conv_fwd: unsupported (ksize=%d, stride=%d)", p->ksize, p->stride); return CHAP_EUNSUPPORTED; }
    if (p->combine == 1 && p->nsrc == 2 && geom != 2 && geom != 1) { chap_set_error("chap_conv_fwd: add-combine is built for k3 s1 only"); return CHAP_EUNSUPPORTED; }
    q->geom = geom;
    q->cpar = 0;
    // blocking: NT = 16-channel tiles per block, MR = 16-pixel rows per wave.  Large tiles (halo overhead,
    // weight reuse) when the layer has plenty of pixels; small tiles when it would not fill 256 CUs.
    int NT = b.ntiles >= 4 ? 4 : (b.ntiles >= 2 ? 2 : 1);
    int MR = (geom == 2 || geom == 5) ? 1 : 2;
    const bool bf = p->dtype == CHAP_BF16;
    if (geom == 2 && bf) {
        // 3D 3x3x3 (measured on the V-Net shapes, tools/lab/conv_lab.hip sweeps): z-per-wave bricks (MR = 4) once
        // the grid has >= 64 bricks, with the widest NT that still gives >= 128 blocks; the deep, tiny layers run
        // 1 x 4 x 16 slabs with NT = 2 (two blocks per CU, weights staged through LDS).  Round-2 sweep over (NT, MR)
        // on the real layers (tools/lab/sweep_conv.sh, gpurun_out/conv_sweep3d.log): at 14x14x10, N = 2 (32 bricks) the slabs
        // win -- 128->128 22.0 vs 30.2 us, 128+128->128 24.4 vs 34.7, 256->128 37.4 vs 48.7 -- at 28x28x20 (196 bricks) the bricks
        // do (28.1 vs 41.6).
        const long bricks = (long)p->N * cdiv(p->D, 4) * cdiv(p->H, 4) * cdiv(p->W, 16);
        if (bricks >= 64) {
            MR = 4;
            // at most 32 output channels per block: the stand-alone sweeps preferred 64 for the 64-channel level (28x28x20), the whole
            // 3D iteration does not (17.09 -> 16.79 ms per step with NT = 2: more, smaller blocks share the CUs with the other streams)
            if (NT > 2) NT = 2;
            while (NT > 1 && bricks * cdiv(b.ntiles, NT) < 128) NT >>= 1;
        } else if (b.KC == 32 && NT > 2) {
            NT = 2;
        }
    }
    if (geom == 1 || geom == 3) {
        auto blocks = [&](int mr, int nt) { return (long)p->N * p->D * cdiv(p->H, 4 * mr) * cdiv(p->W, 16) * cdiv(b.ntiles, nt); };
        if (geom == 1 && bf && b.KC == 32 && b.ntiles >= 4) {
            // deep 2D layers (Cout >= 64): 8 x 16 tiles x 32 channels -- two blocks per CU hide each other's
            // staging latency and the staged weights fit; best or within 5% of best for 64@64 .. 256@16, N = 12 / 24
            MR = 2; NT = 2;
        } else if (geom == 1 && b.KC == 16 && blocks(4, NT) >= 512) MR = 4;
        else if (blocks(2, NT) >= 384) MR = 2;
        else {
            MR = 1;
            while (NT > 1 && blocks(1, NT) < 384) NT >>= 1;
        }
    }
    // lab knobs (tools/shape_table.py sweeps): CHAP_CONV_NT / CHAP_CONV_MR override the blocking of the k3 s1 layers with
    // at least CHAP_CONV_MINC (default 64) input channels
    if ((geom == 1 || geom == 2) && Ck >= chap_knob(KNOB_CONV_MINC)) {
        const long nt = chap_knob(KNOB_CONV_NT), mr = chap_knob(KNOB_CONV_MR);
        if (nt > 0 && nt <= b.ntiles) NT = (int)nt;
        if (mr > 0) MR = (int)mr;
    }
    q->route = CONV_ROUTE_GENERIC; q->NT = NT; q->MR = MR;
    // ---- the V-Net heads: 1x1x1 conv of a 16-channel lazy activation to <= 8 classes, fp32 planar logits (conv_head1x1_kernel, conv_kernel.h)
    if (bf && geom == 3 && p->out_planar && p->Cout <= 8 && p->nsrc == 1 && Ck == 16 && p->src[0].C == 16 && !p->stats && p->out_mode == 0) {
        q->route = CONV_ROUTE_HEAD;
        return CHAP_OK;
    }
    // ---- the 2D full-resolution layers (all input channels in ONE chunk of 16 or 32): wave-private pipelines (conv_wp.h), bf16.  CHAP_CONV_WP (lab knob):
    // 0 = never, N = from N tiles of 4 x 16 pixels up (default 1: every eligible layer).  Stand-alone (profiles/r04_conv_wp_ab.log): 16->32 at 256 x 256
    // 34.1 -> 29.1 us, 32->16 32.0 -> 25.1, 32->64 at 128 x 128 20.6 -> 17.9, 16->32 at 128 x 128 14.9 -> 13.0; the 16->16 layer with BatchNorm prologue and
    // statistics 20.8 -> 20.5 (it is VALU-bound in its staging, not short of loads in flight), 32->32 with statistics 14.7 -> 15.3.  Whole 2D iteration, three
    // A/B pairs: 6.451 -> 6.406 ms.  Outputs are bit-identical to conv_fwd_kernel's.
    // (D == 1: the kernel walks N images of H x W; dims = 2 with D > 1 -- N*D slices -- takes the generic kernel)
    if (bf && geom == 1 && p->D == 1 && p->out_mode == 0 && !p->out_planar && !p->out_f32 && (p->Cout & 15) == 0 && p->Cout <= 64 && p->combine == 0 &&
        Ck == b.KC && (p->nsrc == 1 || (b.KC == 32 && p->src[0].C == 16 && p->src[1].C == 16))) {
        const long wp_min = chap_knob(KNOB_CONV_WP);
        const long t4 = (long)p->N * cdiv(p->H, 4) * cdiv(p->W, 16);
        if (wp_min > 0 && t4 >= wp_min) {
            q->route = CONV_ROUTE_WP; q->NT = b.ntiles == 1 ? 1 : 2; q->MR = 1;      // (64 output channels: two block rows; four 16-channel tiles per wave spill)
            return CHAP_OK;
        }
    }
    // ---- the deep, small 3x3(x3) layers: K-chunks side by side (conv_kpar.h) instead of one after the other
    if (bf && (geom == 1 || geom == 2) && p->out_mode == 0 && !p->out_planar && (p->Cout & 3) == 0 && !p->out2 &&
        (p->nsrc == 1 || (p->combine == 0 && p->src[0].C % b.KC == 0)) && !(d3 && (p->src[0].keep || (p->nsrc > 1 && p->src[1].keep)))) {
        // Measured per layer shape (tools/shape_table.py with CHAP_CONV_KPAR = 0 / 1, gpurun_out/kpar*.log), kernel alone: it wins while the
        // launch is about one wave of blocks -- 3D 256->256 at 7x7x5 23.3 -> 14.4 us, 128->128 at 14x14x10 20.5 -> 17.0, 256->128 39.1 -> 29.6;
        // 2D 128->256 at 32x32 20.4 -> 14.7, 256->256 at 16x16 15.2 -> 10.8, 128+128->128 23.5 -> 19.2 -- and loses where a CU gets several
        // tiles, which conv_fwd_kernel's persistent blocks overlap (3D 64->64 at 28x28x20, 1120 blocks: 24.4 -> 30.8).  Inside the
        // iteration the 3D step gains 0.8 % (18.32 -> 18.17 ms, three A/B pairs); the 2D step does NOT (7.62 -> 7.69 ms: there the
        // weights are not L2-hot as in the stand-alone timing, and a wave's fragment ring covers an L2 hit, not a MALL round trip), so
        // by default only the 3D layers take this kernel.
        const long mode = chap_knob(KNOB_CONV_KPAR);
        const int cpar = b.nchunks % 4 == 0 ? 4 : (b.nchunks % 2 == 0 ? 2 : 0);
        const long kblocks = (long)p->N * p->D * cdiv(p->H, d3 ? 4 : 8) * cdiv(p->W, 16) * cdiv(b.ntiles, 2);
        if (cpar && Ck >= 64 && (mode == 1 || (mode == 2 && d3 && kblocks <= chap_knob(KNOB_CONV_KPAR_MAX)))) {
            q->route = CONV_ROUTE_KPAR; q->NT = 2; q->MR = d3 ? 1 : 2; q->cpar = cpar;
            return CHAP_OK;
        }
    }
    if (p->dtype != CHAP_BF16 && p->dtype != CHAP_F32) { chap_set_error("chap_conv_fwd: dtype=%d", p->dtype); return CHAP_EINVAL; }
    return CHAP_OK;
}

// ---- the weight packer's side: the same blocking, from the pack parameters
struct pack_geom { int Ck, Ck_real, Cn_logical, ctaps; };   // Ck = K channels padded to 16 (tiny heads)
static inline int conv_pack_blocking(const chap_pack_params* p, const char* who, pack_geom* g, conv_blocking* b) {
    switch (p->kind) {
        case CHAP_PACK_CONV_FWD:     g->Ck = p->Cin;  g->Cn_logical = p->Cout;           g->ctaps = p->taps; break;
        case CHAP_PACK_CONV_DGRAD:   g->Ck = p->Cout; g->Cn_logical = p->Cin;            g->ctaps = p->taps; break;
        case CHAP_PACK_DECONV_FWD:   g->Ck = p->Cin;  g->Cn_logical = p->taps * p->Cout; g->ctaps = 1;       break;
        case CHAP_PACK_DECONV_DGRAD: g->Ck = p->Cout; g->Cn_logical = p->Cin;            g->ctaps = p->taps; break;
        case CHAP_PACK_DOWN_DGRAD:   g->Ck = p->Cout; g->Cn_logical = p->taps * p->Cin;  g->ctaps = 1;       break;
        default: chap_set_error("chap_pack: kind=%d", p->kind); return CHAP_EINVAL;
    }
    g->Ck_real = g->Ck;
    g->Ck = (g->Ck + 15) / 16 * 16;
    *b = conv_blocking_for(g->Ck, g->ctaps, g->Cn_logical);
    CHAP_CHECK_ARG(g->Ck % b->KC == 0, "%s: K channels %d not a multiple of %d", who, g->Ck, b->KC);
    return CHAP_OK;
}
