// chap_conv_fwd / chap_pack_weights: make the plan (conv_plan.h), launch what it names; the weight packing kernel.
#include "launchers.h"
#include "launch.h"

extern "C" int chap_conv_fwd(const chap_conv_params* p, void* stream) {
    conv_plan q;
    if (int r = conv_make_plan(p, &q)) return r;
    hipStream_t s = (hipStream_t)stream;
    typedef int (*conv_launch_fn)(const chap_conv_params*, const conv_plan&, hipStream_t);
    static const conv_launch_fn table[2][5] = {
        {chap_conv_launch_f32_g1, chap_conv_launch_f32_g2, chap_conv_launch_f32_g3, chap_conv_launch_f32_g4, chap_conv_launch_f32_g5},
        {chap_conv_launch_bf16_g1, chap_conv_launch_bf16_g2, chap_conv_launch_bf16_g3, chap_conv_launch_bf16_g4, chap_conv_launch_bf16_g5}};
    switch (q.route) {
        case CONV_ROUTE_HEAD: return chap_conv_launch_head_bf16(p, s);
        case CONV_ROUTE_WP:   return chap_conv_launch_wp_bf16(p, q, s);
        case CONV_ROUTE_KPAR: return chap_conv_launch_kpar_bf16(p, q, s);
        default:              return table[p->dtype == CHAP_BF16][q.geom - 1](p, q, s);
    }
}

// ---- weight packing ------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void pack_body(const float* __restrict__ w, T* __restrict__ out, int kind, int Cin, int Cout, int taps,
                                          int KC, int GPT, int NP, int STEPS, int nchunks, int ntiles, int Cn_logical, int Ck_real,
                                          long first, long stride) {
    const long total = (long)nchunks * STEPS * ntiles * 64;
    // The units are enumerated with (tap, 8-channel group) fastest, NOT in output order: neighbouring threads then read neighbouring
    // taps of the same checkpoint rows (a load instruction touches a few cache lines instead of 64 -- the kernel is gather-bound) and
    // each writes its 16-byte unit to its place in the fragment layout.
    const int PPS = STEPS * 4;
    for (long q = first; q < total; q += stride) {
        const int pp = (int)(q % PPS);
        long r = q / PPS;
        const int n16 = (int)(r & 15); r >>= 4;
        const int nt = (int)(r % ntiles);
        const int chunk = (int)(r / ntiles);
        const int step = pp >> 2, g = pp & 3;
        const long i = ((long)(chunk * STEPS + step) * ntiles + nt) * 64 + g * 16 + n16;
        const int nl = nt * 16 + n16;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = 0.f;
            if (pp < NP && nl < Cn_logical) {
                const int tap = pp / GPT, c = chunk * KC + (pp % GPT) * 8 + j;
                long a = -1;
                if (c < Ck_real)
                switch (kind) {
                    case CHAP_PACK_CONV_FWD:     a = ((long)nl * Cin + c) * taps + tap; break;
                    case CHAP_PACK_CONV_DGRAD:   a = ((long)c * Cin + nl) * taps + (taps - 1 - tap); break;
                    case CHAP_PACK_DECONV_FWD:   a = ((long)c * Cout + (nl % Cout)) * taps + (nl / Cout); break;
                    case CHAP_PACK_DECONV_DGRAD: a = ((long)nl * Cout + c) * taps + tap; break;
                    default:                     a = ((long)c * Cin + (nl % Cin)) * taps + (nl / Cin); break;  // DOWN_DGRAD
                }
                if (a >= 0) x = w[a];
            }
            v[j] = x;
        }
        st8(out + i * 8, v);
    }
}

template <typename T>
__global__ void pack_kernel(const float* __restrict__ w, T* __restrict__ out, int kind, int Cin, int Cout, int taps,
                            int KC, int GPT, int NP, int STEPS, int nchunks, int ntiles, int Cn_logical, int Ck_real) {
    pack_body<T>(w, out, kind, Cin, Cout, taps, KC, GPT, NP, STEPS, nchunks, ntiles, Cn_logical, Ck_real,
                 (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

__global__ void pack_multi_kernel(const chap_pack_entry* __restrict__ E) {
    const chap_pack_entry e = E[blockIdx.y];
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    if (first >= e.total) return;
    if (e.dtype == CHAP_BF16) pack_body<bf16_t>(e.w, (bf16_t*)e.out, e.kind, e.Cin, e.Cout, e.taps, e.KC, e.GPT, e.NP, e.STEPS, e.nchunks, e.ntiles, e.Cn_logical, e.Ck_real, first, stride);
    else pack_body<float>(e.w, (float*)e.out, e.kind, e.Cin, e.Cout, e.taps, e.KC, e.GPT, e.NP, e.STEPS, e.nchunks, e.ntiles, e.Cn_logical, e.Ck_real, first, stride);
}

extern "C" int chap_pack_describe(const chap_pack_params* p, chap_pack_entry* e) {
    CHAP_CHECK_ARG(p && e && p->w && p->out, "chap_pack_describe: null argument");
    pack_geom g;
    conv_blocking b;
    if (int r = conv_pack_blocking(p, "chap_pack_describe", &g, &b)) return r;
    e->w = p->w; e->out = p->out; e->kind = p->kind; e->Cin = p->Cin; e->Cout = p->Cout; e->taps = p->taps; e->dtype = p->dtype;
    e->KC = b.KC; e->GPT = b.GPT; e->NP = b.NP; e->STEPS = b.STEPS; e->nchunks = b.nchunks; e->ntiles = b.ntiles;
    e->Cn_logical = g.Cn_logical; e->Ck_real = g.Ck_real;
    e->total = (int64_t)b.nchunks * b.STEPS * b.ntiles * 64;
    return CHAP_OK;
}

extern "C" int chap_pack_multi(const chap_pack_entry* entries_dev, int32_t n, int64_t max_total, void* stream) {
    CHAP_CHECK_ARG(entries_dev && n > 0 && max_total > 0, "chap_pack_multi: bad argument");
    CHAP_NOT_IN_GROUP("chap_pack_multi");
    // one fragment unit (8 gathered values) per thread and loop step: the largest layer sets the time (3D 256x256x27: 221k units), so it gets
    // up to 1024 blocks -- 64 made this launch, the first of every iteration, 33 us (2D) / 164 us (3D), now 24 / 103; the small entries'
    // blocks exit at once.  (Tried: one block per (K-chunk, 16-channel tile) reading its runs of the checkpoint tensor coalesced into
    // LDS: fewer, longer blocks -- 58 / 153 us.)
    long bx = (max_total + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(pack_multi_kernel, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, entries_dev);
    CHAP_LAUNCH_CHECK("chap_pack_multi");
    return CHAP_OK;
}

extern "C" size_t chap_pack_size(const chap_pack_params* p) {
    pack_geom g;
    conv_blocking b;
    if (!p || conv_pack_blocking(p, "chap_pack_size", &g, &b)) return 0;
    return (size_t)b.nchunks * b.STEPS * b.ntiles * 64 * 8 * (p->dtype == CHAP_BF16 ? 2 : 4);
}

extern "C" int chap_pack_weights(const chap_pack_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->w && p->out, "chap_pack_weights: null argument");
    CHAP_NOT_IN_GROUP("chap_pack_weights");
    pack_geom g;
    conv_blocking b;
    if (int r = conv_pack_blocking(p, "chap_pack_weights", &g, &b)) return r;
    const long total = (long)b.nchunks * b.STEPS * b.ntiles * 64;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    if (p->dtype == CHAP_BF16)
        hipLaunchKernelGGL(pack_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p->w, (bf16_t*)p->out, p->kind, p->Cin, p->Cout, p->taps,
                           b.KC, b.GPT, b.NP, b.STEPS, b.nchunks, b.ntiles, g.Cn_logical, g.Ck_real);
    else if (p->dtype == CHAP_F32)
        hipLaunchKernelGGL(pack_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p->w, (float*)p->out, p->kind, p->Cin, p->Cout, p->taps,
                           b.KC, b.GPT, b.NP, b.STEPS, b.nchunks, b.ntiles, g.Cn_logical, g.Ck_real);
    else { chap_set_error("chap_pack_weights: dtype=%d", p->dtype); return CHAP_EINVAL; }
    CHAP_LAUNCH_CHECK("chap_pack_weights");
    return CHAP_OK;
}
