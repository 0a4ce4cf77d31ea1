// The launch plan of chap_wgrad: kernel family, chunk / tile widths, split count and workspace size, as integer arithmetic on the params
// struct.  Host-only (no HIP).  chap_wgrad_ws sizes the workspace from it, wgrad_dispatch.inc picks the instance from it, the reduction sums
// its nsplit slabs: one B-tile width bn for all three.
#pragma once
#include <cstdio>
#include "host.h"
#include "knobs.h"

// brick: 0 = slab kernel, 1 = 3D 4 x 4 x 16 bricks, 2 = 2D wave-private pipelines; bn = B-tile width (16 / 32);
// mr = tile rows per wave / 4 of the wave-private kernel (brick == 2 only, else 0)
struct wg_plan { int Ca, Cb, KC, taps, nsplit, brick, bn, mr; long ntiles; size_t slab, bytes; };

static inline int wg_make_plan(const chap_wgrad_params* p, wg_plan* q) {
    CHAP_CHECK_ARG(p->na == 1 || p->na == 2, "chap_wgrad: na=%d", p->na);
    q->Ca = p->combine == 0 ? p->a[0].C + (p->na > 1 ? p->a[1].C : 0) : p->a[0].C;
    q->Cb = p->b.C;
    CHAP_CHECK_ARG(q->Ca % 16 == 0 && q->Cb % 8 == 0, "chap_wgrad: Ca=%d must be a multiple of 16, Cb=%d of 8", q->Ca, q->Cb);
    // (the staging of an add-combined pair applies keep mask and channel multipliers of the FIRST source only: conv_kernel.h halo_commit_impl)
    if (p->combine == 1 && p->na == 2 && (p->a[1].keep || p->a[1].chan_mul)) { chap_set_error("chap_wgrad: add-combine takes a keep mask / channel multipliers on the first source only"); return CHAP_EUNSUPPORTED; }
    q->KC = (q->Ca >= 32 && q->Ca % 32 == 0) ? 32 : 16;
    if (p->dtype == CHAP_F32 && p->ksize == 2) q->KC = 16;      // fp32 k2 s2 halos: two buffers of 32 channels exceed the 160 KiB LDS
    // 3D 3x3x3, bf16: 4 x 4 x 16 bricks with 16-channel A chunks (the 1 x 4 x 16 slab stages 5.1 A-pixels per output pixel and pays a
    // barrier + a prefetch round trip per 64 pixels; the brick 2.5 and one per 256).  Threshold swept on the whole 3D iteration
    // (CHAP_WGRAD_BRICK = 2048 / 512 / 128 / 16 / 4 bricks: 17.87 / 17.65 / 17.33 / 17.17 / 17.17 ms per step): everything but the 7x7x5 level
    // (8 bricks, all the same) gains.
    q->brick = 0;
    {
        const long min_bricks = chap_knob(KNOB_WGRAD_BRICK);
        const long bricks = (long)p->N * cdiv(p->D, 4) * cdiv(p->H, 4) * cdiv(p->W, 16);
        if (p->dims == 3 && p->ksize == 3 && p->stride == 1 && p->dtype == CHAP_BF16 && min_bricks > 0 && bricks >= min_bricks &&
            p->a[0].C <= 256 && (p->na < 2 || p->a[1].C <= 256) && p->b.C <= 256) { q->brick = 1; q->KC = 16; }      // (<= 256 channels per source: the brick kernels' scale/shift cache)
    }
    // 2D 3x3 layers, bf16, <= 256 channels per source: wave-private pipelines (wgrad_wp.h; brick == 2), 16-channel A chunks.  CHAP_WGRAD_WP (lab knob):
    // 0 = never, N = from N tiles (8 x 16 pixels) up.  Default 1 = every eligible layer: the large images gain most (16->16 at 256 x 256 36.8 -> 25.2 us),
    // the deep layers 10-18 % (128->128 at 32 x 32 29.2 -> 25.9 us, 64+64->64 at 64 x 64 41.0 -> 33.8); whole 2D iteration, three A/B pairs per setting:
    // threshold 1024 / 256 / 64 / 1 -> 6.513 / 6.513 / 6.506 / 6.476 ms (profiles/r04_wgrad_wp_ab.log).
    {
        const long wp_min = chap_knob(KNOB_WGRAD_WP);        // (live: the tests force the kernel onto small ragged grids)
        const long t8 = (long)p->N * cdiv(p->H, 8) * cdiv(p->W, 16);
        // (D == 1: the kernel walks N images of H x W; dims = 2 with D > 1 -- N*D slices -- takes the slab kernel)
        if (p->dims == 2 && p->D == 1 && p->ksize == 3 && p->stride == 1 && p->combine == 0 && p->dtype == CHAP_BF16 && wp_min > 0 && t8 >= wp_min &&
            p->a[0].C <= 256 && p->a[0].C % 16 == 0 && (p->na < 2 || (p->a[1].C <= 256 && p->a[1].C % 16 == 0)) && p->b.C <= 256) { q->brick = 2; q->KC = 16; }
    }
    // (tried: 16 x 16 tiles for the 2D 16-channel levels -- 16->16 at 256x256 35.8 -> 32.9 us with 512 blocks, 16+16->16 unchanged: not kept)
    CHAP_CHECK_ARG(q->Ca % q->KC == 0, "chap_wgrad: Ca=%d not a multiple of %d", q->Ca, q->KC);
    q->taps = p->ksize * p->ksize * (p->dims == 3 ? p->ksize : 1);
    const bool small_tile = (p->dims == 3 && p->ksize >= 2);   // 3D geometries use 4 x 16 tiles (MR = 1)
    const int TH = small_tile ? 4 : 8;
    q->ntiles = (long)p->N * (q->brick == 1 ? cdiv(p->D, 4) : p->D) * cdiv(p->H, TH) * cdiv(p->W, 16);
    // layers with <= 16 output channels (the full-resolution levels) use 16-channel B tiles: half the B staging and MFMAs; the 3D bricks
    // up to CHAP_WGRAD_BN16_MAXC B channels (lab knob)
    const int bn = q->bn = (q->Cb <= 16 || (q->brick == 1 && q->Cb <= chap_knob(KNOB_WGRAD_BN16_MAXC))) ? 16 : 32;
    // wave-private kernel: 8 x 16 tiles per wave (mr = 2) with 16-wide B tiles unless CHAP_WGRAD_WP_MR = 1 (lab knob); 4 x 16 with 32-wide B tiles
    q->mr = q->brick != 2 ? 0 : (bn == 32 || chap_knob(KNOB_WGRAD_WP_MR) == 1) ? 1 : 2;
    const long pairs = (long)(q->Ca / q->KC) * cdiv(q->Cb, bn);
    // Persistent, pipelined blocks.  What bounds the small-channel layers (most of the bytes) is memory-level parallelism --
    // a block keeps a few KB in flight -- so they take as many blocks as stay resident (LDS: 3 per CU with 16-channel chunks,
    // 2 with 32); their slabs are tiny (9-37 KB).  The wide layers keep about one block per CU: more splits only add slab
    // bytes to reduce.  Targets measured per layer shape (tools/shape_table.py --only wgrad with CHAP_WGRAD_BLOCKS = 256 / 512 /
    // 768 / 1024 / 2048, gpurun_out/wgrad_sweep*.log): e.g. 16->16 at 256x256 58 / 41 / 37 / 43 / 49 us, 16+16->16 80 / 55 / 65 / 60 /
    // 72, 32+32->32 at 128x128 47 / 35 / 44 / 44 / 58, k2 s2 layers 17-23 / 20-25 / 24-28; 3D 16->16 at 112x112x80 209 / 129 / - / 134 / 145,
    // 3D 32->32 at 56x56x40 67 / 79 / - / 80 / 79.
    long target = 256;
    const bool d3 = p->dims == 3;
    const long forced = chap_knob(KNOB_WGRAD_BLOCKS);          // lab knob for those sweeps
    if (forced) target = forced;
    else if (q->brick == 2) target = chap_knob(KNOB_WGRAD_WP_BLOCKS);
    else if (p->ksize == 2) target = 256;
    else if (q->brick) target = bn == 16 ? 512 : chap_knob(KNOB_WGRAD_BRICK_BLOCKS);      // 16-wide B tiles leave LDS for two bricks per CU (3D 16->16 at 112x112x80: 88 / 66 / 85 us with 256 / 512 / 768 blocks)
    else if (q->KC == 16) target = d3 ? 512 : 768;
    // (the stand-alone timings above also favoured 512 blocks for the 2D two-source / 32-channel layers; on the whole iteration the default
    //  256 is better -- CHAP_WGRAD_TARGETS sweep, final tree: 768,512,256 -> 7.25 ms, 768,256,256 -> 7.16 ms per 2D step)
    {   // lab knob: CHAP_WGRAD_TARGETS="a,b,c" = split targets of (2D 16-channel chunks, 2D two-source / <= 32 channels, everything else k3/k1)
        const char* et = chap_knob_text(KNOB_WGRAD_TARGETS);
        long ta = 0, tb = 0, tc = 0;
        if (et && !forced && sscanf(et, "%ld,%ld,%ld", &ta, &tb, &tc) == 3 && p->ksize != 2 && !q->brick) {      // (brick: 3D bricks = 1, wave-private 2D = 2)
            if (q->KC == 16) { if (!d3 && ta > 0) target = ta; }
            else if (!d3 && (p->na == 2 || q->Ca <= 32)) { if (tb > 0) target = tb; }      // (the class that used to have its own default)
            else if (tc > 0) target = tc;
        }
    }
    long ns = target / pairs;
    if (ns < 1) ns = 1;
    if (ns > q->ntiles) ns = q->ntiles;
    q->slab = (size_t)q->taps * q->Ca * q->Cb * sizeof(float);
    const size_t cap = (size_t)96 << 20;
    while (ns > 1 && (size_t)ns * q->slab > cap) ns /= 2;
    q->nsplit = (int)ns;
    q->bytes = (size_t)q->nsplit * (q->slab + (size_t)q->Cb * sizeof(float));
    return CHAP_OK;
}
