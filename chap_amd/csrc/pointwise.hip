#include <cstdlib>
// Element-wise / reduction kernels around the convolutions: first-layer (Cin = 1) direct conv,
// BatchNorm finalize, lazy-activation max-pool, align_corners 2x upsample (+ adjoint), the
// BN/activation backward pair, layout converters.  All HBM-bound: 16-byte vector accesses along
// the channel axis, wave64 shuffle reductions, one float atomic per block and channel.
#include "common.h"
#include "launch.h"
#include "actbwd_math.h"
#include "conv_c1_mfma.h"

// Fixed-order wave reduction in fp64 (xor butterfly: the same pairing on every run).
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// =========================================================================================
// First conv, Cin = 1, k3 s1 "same" (unet.py:50 with in_chns=1; vnet.py:19 with n_channels=1).
// One thread per output pixel computes all Cout (<= 32) channels; weights + bias live in LDS.
template <typename T, bool D3, int CO>
__device__ __forceinline__ void conv_c1_fwd_kernel(const chap_conv_c1_params& P) {
    constexpr int KD = D3 ? 3 : 1, TAPS = KD * 9;
    __shared__ float ws[CO * TAPS + 2 * CO];
    __shared__ float bstat[4][2 * CO];
    for (int i = threadIdx.x; i < CO * TAPS; i += 256) ws[i] = P.w[i];
    for (int i = threadIdx.x; i < CO; i += 256) { ws[CO * TAPS + i] = P.bias ? P.bias[i] : 0.f; ws[CO * TAPS + CO + i] = (P.stats && P.stats_shift) ? P.stats_shift[i] : 0.f; }
    __syncthreads();
    const long npix = (long)P.N * P.D * P.H * P.W;
    float ssum[CO], ssq[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) { ssum[c] = 0.f; ssq[c] = 0.f; }
    for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (long)gridDim.x * 256) {
        const u32 up = (u32)pix;
        const int x = (int)(up % (u32)P.W); u32 r = up / (u32)P.W;
        const int y = (int)(r % (u32)P.H); r /= (u32)P.H;
        const int z = (int)(r % (u32)P.D); const int n = (int)(r / (u32)P.D);
        float in[TAPS];
#pragma unroll
        for (int dz = 0; dz < KD; ++dz)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int zz = z + dz - (D3 ? 1 : 0), yy = y + dy - 1, xx = x + dx - 1;
                    const bool ib = (unsigned)zz < (unsigned)P.D && (unsigned)yy < (unsigned)P.H && (unsigned)xx < (unsigned)P.W;
                    in[(dz * 3 + dy) * 3 + dx] = ib ? P.x[(((long)n * P.D + zz) * P.H + yy) * P.W + xx] : 0.f;
                }
        float acc[CO];
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            float a = ws[CO * TAPS + c];
#pragma unroll
            for (int t = 0; t < TAPS; ++t) a = fmaf(in[t], ws[c * TAPS + t], a);
            acc[c] = a;
            const float as = a - ws[CO * TAPS + CO + c];        // shifted moments (chap_hip.h, "stats")
            ssum[c] += as; ssq[c] += as * as;
        }
        T* o = (T*)P.out + pix * CO;
#pragma unroll
        for (int c = 0; c < CO; c += 8) st8(o + c, acc + c);
    }
    if (P.stats) {          // this block's partial slot, the format of conv_stats_flush (conv_parts.h): CO channels per thread, so a fixed-order wave butterfly, then the four waves in the same fixed order
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            const float s = wave_sum(ssum[c]), q = wave_sum(ssq[c]);
            if ((threadIdx.x & 63) == 0) { bstat[threadIdx.x >> 6][c] = s; bstat[threadIdx.x >> 6][CO + c] = q; }
        }
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x == 0) *(int*)P.stats = (int)gridDim.x;
        for (int i = threadIdx.x; i < 2 * CO; i += 256)
            P.stats[CHAP_STATS_HDR + (long)blockIdx.x * 2 * CO + i] = (bstat[0][i] + bstat[1][i]) + (bstat[2][i] + bstat[3][i]);
    }
}

extern "C" int chap_conv_c1_fwd(const chap_conv_c1_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->x && p->w && p->out, "chap_conv_c1_fwd: null argument");
    CHAP_CHECK_ARG(p->Cout == 16, "chap_conv_c1_fwd: Cout=%d (only 16 built)", p->Cout);
    CHAP_CHECK_ARG(p->dims == 2 || p->dims == 3, "chap_conv_c1_fwd: dims=%d", p->dims);
    const long npix = (long)p->N * p->D * p->H * p->W;
    dim3 grid((unsigned)(cdiv(npix, 256) < CHAP_STATS_MAX_SLOTS ? cdiv(npix, 256) : CHAP_STATS_MAX_SLOTS));   // one statistics slot per block
    hipStream_t s = (hipStream_t)stream;
    const bool d3 = p->dims == 3, bf = p->dtype == CHAP_BF16;
    if (bf) {
        // bf16: the taps as the K dimension of one MFMA per 16 pixels (conv_c1_mfma.h).  CHAP_C1_MFMA=0 (lab knob): the scalar kernel below.
        if (chap_knob(KNOB_C1_MFMA) != 0) {
            CHAP_CHECK_ARG(npix < (1l << 31), "chap_conv_c1_fwd: %ld pixels", npix);
            auto waste = [&](int txt) { const int tx = 16 * txt; return cdiv(p->W, tx) * tx - p->W; };
            const int txt = waste(5) < waste(4) ? 5 : 4;         // 16-pixel tiles per block row: W = 80 (LA patches) takes 5, powers of two 4
            const int ty = d3 ? 4 : 8, tz = d3 ? 2 : 1;
            const long ntiles = (long)p->N * cdiv(p->D, tz) * cdiv(p->H, ty) * cdiv(p->W, 16 * txt);
            dim3 g((unsigned)(ntiles < CHAP_STATS_MAX_SLOTS ? ntiles : CHAP_STATS_MAX_SLOTS));      // persistent blocks, one statistics slot each
            if (d3 && txt == 5) return chap_launch<chap_conv_c1_params, conv_c1_mfma_kernel<true, 5>, 256>(g, dim3(256), 0, s, *p, "chap_conv_c1_fwd(mfma)");
            if (d3) return chap_launch<chap_conv_c1_params, conv_c1_mfma_kernel<true, 4>, 256>(g, dim3(256), 0, s, *p, "chap_conv_c1_fwd(mfma)");
            if (txt == 5) return chap_launch<chap_conv_c1_params, conv_c1_mfma_kernel<false, 5>, 256>(g, dim3(256), 0, s, *p, "chap_conv_c1_fwd(mfma)");
            return chap_launch<chap_conv_c1_params, conv_c1_mfma_kernel<false, 4>, 256>(g, dim3(256), 0, s, *p, "chap_conv_c1_fwd(mfma)");
        }
    }
    if (bf && d3) return chap_launch<chap_conv_c1_params, conv_c1_fwd_kernel<bf16_t, true, 16>, 256>(grid, dim3(256), 0, s, *p, "chap_conv_c1_fwd");
    if (bf) return chap_launch<chap_conv_c1_params, conv_c1_fwd_kernel<bf16_t, false, 16>, 256>(grid, dim3(256), 0, s, *p, "chap_conv_c1_fwd");
    if (d3) return chap_launch<chap_conv_c1_params, conv_c1_fwd_kernel<float, true, 16>, 256>(grid, dim3(256), 0, s, *p, "chap_conv_c1_fwd");
    return chap_launch<chap_conv_c1_params, conv_c1_fwd_kernel<float, false, 16>, 256>(grid, dim3(256), 0, s, *p, "chap_conv_c1_fwd");
}

// Backward of the first conv: dx (VAT needs dL/dx), dw, db.
//   dx[p]      = sum_{tap,c} g[p - tap + pad][c] * w[c][tap]
//   dw[c][tap] = sum_p x[p + tap - pad] * g[p][c]      (block partials -> ws, then one reduce pass)
struct c1_bwd_args { chap_conv_c1_bwd_params P; int nblocks; };
template <typename T, bool D3, int CO>
__device__ __forceinline__ void conv_c1_bwd_kernel(const c1_bwd_args& A) {
    const chap_conv_c1_bwd_params& P = A.P;
    const int nblocks = A.nblocks;
    constexpr int KD = D3 ? 3 : 1, TAPS = KD * 9;
    __shared__ float ws[CO * TAPS];
    __shared__ float part[4][CO * TAPS + CO];
    for (int i = threadIdx.x; i < CO * TAPS; i += 256) ws[i] = P.w[i];
    __syncthreads();
    const long npix = (long)P.N * P.D * P.H * P.W;
    const T* g = (const T*)P.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- dx ----
    if (P.dx) {
        for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (long)nblocks * 256) {
            const u32 up = (u32)pix;
            const int x = (int)(up % (u32)P.W); u32 r = up / (u32)P.W;
            const int y = (int)(r % (u32)P.H); r /= (u32)P.H;
            const int z = (int)(r % (u32)P.D); const int n = (int)(r / (u32)P.D);
            float a = 0.f;
#pragma unroll
            for (int dz = 0; dz < KD; ++dz)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int zz = z - dz + (D3 ? 1 : 0), yy = y - dy + 1, xx = x - dx + 1;
                        if ((unsigned)zz < (unsigned)P.D && (unsigned)yy < (unsigned)P.H && (unsigned)xx < (unsigned)P.W) {
                            const long q = (((long)n * P.D + zz) * P.H + yy) * P.W + xx;
                            const int tap = (dz * 3 + dy) * 3 + dx;
#pragma unroll
                            for (int c = 0; c < CO; c += 8) {
                                float v[8];
                                ld8(g + q * CO + c, v);
#pragma unroll
                                for (int j = 0; j < 8; ++j) a = fmaf(v[j], ws[(c + j) * TAPS + tap], a);
                            }
                        }
                    }
            P.dx[pix] = a;
        }
    }
    // ---- dw / db partials: thread t handles channel c = t % CO and pixel-lane q = t / CO ----
    if (P.dw || P.db) {
        constexpr int PL = 256 / CO;          // pixels processed in parallel per block step
        const int c = threadIdx.x % CO, q = threadIdx.x / CO;
        float a[TAPS], ab = 0.f;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) a[t] = 0.f;
        for (long pix = (long)blockIdx.x * PL + q; pix < npix; pix += (long)nblocks * PL) {
            const u32 up = (u32)pix;
            const int x = (int)(up % (u32)P.W); u32 r = up / (u32)P.W;
            const int y = (int)(r % (u32)P.H); r /= (u32)P.H;
            const int z = (int)(r % (u32)P.D); const int n = (int)(r / (u32)P.D);
            const float gv = elem<T>::get(g[pix * CO + c]);
            ab += gv;
#pragma unroll
            for (int dz = 0; dz < KD; ++dz)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int zz = z + dz - (D3 ? 1 : 0), yy = y + dy - 1, xx = x + dx - 1;
                        const bool ib = (unsigned)zz < (unsigned)P.D && (unsigned)yy < (unsigned)P.H && (unsigned)xx < (unsigned)P.W;
                        const float xv = ib ? P.x[(((long)n * P.D + zz) * P.H + yy) * P.W + xx] : 0.f;
                        a[(dz * 3 + dy) * 3 + dx] = fmaf(xv, gv, a[(dz * 3 + dy) * 3 + dx]);
                    }
        }
        // reduce over q (threads with equal c): lanes c, c+CO, c+2CO, ... inside a wave, then across waves via LDS
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            float v = a[t];
            for (int o = CO; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            if (lane < CO) part[wave][c * TAPS + t] = v;
        }
        {
            float v = ab;
            for (int o = CO; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            if (lane < CO) part[wave][CO * TAPS + c] = v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < CO * TAPS + CO; i += 256)
            P.ws[(long)blockIdx.x * (CO * TAPS + CO) + i] = part[0][i] + part[1][i] + part[2][i] + part[3][i];
    }
}

struct c1_reduce_args { const float* ws; int nblocks, taps; float* dw; float* db; };
template <int CO>
__device__ __forceinline__ void conv_c1_reduce_kernel(const c1_reduce_args& A) {
    const float* ws = A.ws; const int nblocks = A.nblocks, taps = A.taps; float* dw = A.dw; float* db = A.db;
    __shared__ float red[4];
    const int i = blockIdx.x;                    // one block per output element, threads stride the block partials
    const int tot = CO * taps + CO;
    float s = 0.f;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += ws[(long)b * tot + i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = (red[0] + red[1]) + (red[2] + red[3]);
        if (i < CO * taps) { if (dw) dw[i] += s; } else if (db) db[i - CO * taps] += s;
    }
}

static int c1_bwd_blocks(const chap_conv_c1_bwd_params* p) {
    const long npix = (long)p->N * p->D * p->H * p->W;
    long b = (npix + 255) / 256;
    return (int)(b < 1024 ? b : 1024);
}
extern "C" size_t chap_conv_c1_bwd_ws(const chap_conv_c1_bwd_params* p) {
    const int taps = p->dims == 3 ? 27 : 9;
    return (size_t)c1_bwd_blocks(p) * (p->Cout * taps + p->Cout) * sizeof(float);
}
extern "C" int chap_conv_c1_bwd(const chap_conv_c1_bwd_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->g && p->w, "chap_conv_c1_bwd: null argument");
    CHAP_CHECK_ARG(p->Cout == 16, "chap_conv_c1_bwd: Cout=%d (only 16 built)", p->Cout);
    CHAP_CHECK_ARG(!(p->dw || p->db) || (p->ws && p->x), "chap_conv_c1_bwd: dw/db need x and ws");
    const int nb = c1_bwd_blocks(p);
    hipStream_t s = (hipStream_t)stream;
    const bool d3 = p->dims == 3, bf = p->dtype == CHAP_BF16;
    const c1_bwd_args a = {*p, nb};
    int r;
    if (bf && d3) r = chap_launch<c1_bwd_args, conv_c1_bwd_kernel<bf16_t, true, 16>, 256>(dim3(nb), dim3(256), 0, s, a, "chap_conv_c1_bwd");
    else if (bf) r = chap_launch<c1_bwd_args, conv_c1_bwd_kernel<bf16_t, false, 16>, 256>(dim3(nb), dim3(256), 0, s, a, "chap_conv_c1_bwd");
    else if (d3) r = chap_launch<c1_bwd_args, conv_c1_bwd_kernel<float, true, 16>, 256>(dim3(nb), dim3(256), 0, s, a, "chap_conv_c1_bwd");
    else r = chap_launch<c1_bwd_args, conv_c1_bwd_kernel<float, false, 16>, 256>(dim3(nb), dim3(256), 0, s, a, "chap_conv_c1_bwd");
    if (r) return r;
    if (p->dw || p->db) {
        const int taps = d3 ? 27 : 9, tot = 16 * taps + 16;
        const c1_reduce_args ra = {(const float*)p->ws, nb, taps, p->dw, p->db};
        return chap_launch<c1_reduce_args, conv_c1_reduce_kernel<16>, 256>(dim3(tot), dim3(256), 0, s, ra, "chap_conv_c1_bwd(reduce)");
    }
    return CHAP_OK;
}

// =========================================================================================
// BatchNorm finalize: batch statistics -> (scale, shift) of the lazy activation; running stats
// follow F.batch_norm(training=True): running = (1-m)*running + m*batch, unbiased variance.
// One wave per channel: lane l sums slots l, l+64, ... (and the sub-lattice rows of a transposed conv) in fp64, then a
// fixed xor butterfly -- the same order on every run.  mean = c + S/n, var = Q/n - (S/n)^2 with the moments taken about
// the conv's shift c (no cancellation once c tracks the mean), evaluated in fp64.
__device__ __forceinline__ void bn_finalize_kernel(const chap_bn_finalize_params& Pk) {
    const chap_bn_finalize_params P = chap_args_once(Pk);       // one scalar load and wait in front of the kernel instead of six
    typedef const CHAP_GLOBAL float* gf;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= P.C) return;
    // slots in use: the header word the producing conv wrote (a host-side note of the conv's grid was tried in round 3 to save this
    // load: no measurable difference, and a hidden coupling between two calls -- removed)
    const int nslots = *(const CHAP_GLOBAL int*)P.stats;
    // the per-channel parameters are requested NOW, next to the header and the slots: behind the reduction they were a third
    // dependent memory round trip of a kernel that is nothing but latency
    const bool upd = P.momentum > 0.f && P.running_mean;
    const float gam = ((gf)P.gamma)[c], bet = ((gf)P.beta)[c], sft = P.stats_shift ? ((gf)P.stats_shift)[c] : 0.f;
    const float rm0 = upd ? ((gf)P.running_mean)[c] : 0.f, rv0 = upd ? ((gf)P.running_var)[c] : 0.f;
    const int nsub = P.Clog / P.C;
    const gf st = (gf)P.stats + CHAP_STATS_HDR;
    double s = 0.0, q = 0.0;
    // a lane's slots are lane, lane + 64, ...: at most CHAP_STATS_MAX_SLOTS / 64 = 16 of them.  All loads of a batch are issued
    // before the first add (the kernel is pure latency: one dependent load per iteration made it 6.7 us), the adds keep the
    // fixed order b = lane, lane + 64, ...
    constexpr int NB = CHAP_STATS_MAX_SLOTS / 64;
    for (int k = 0; k < nsub; ++k) {
        float vs[NB], vq[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int b = lane + 64 * i;
            const gf row = st + (long)(b < nslots ? b : 0) * 2 * P.Clog + k * P.C + c;
            vs[i] = row[0]; vq[i] = row[P.Clog];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const bool ok = lane + 64 * i < nslots;
            s += ok ? (double)vs[i] : 0.0; q += ok ? (double)vq[i] : 0.0;
        }
    }
    s = wave_sum_f64(s); q = wave_sum_f64(q);
    if (lane != 0) return;
    if (c == 0 && P.num_batches_tracked && P.momentum > 0.f) *(CHAP_GLOBAL int64_t*)P.num_batches_tracked += 1;
    const double cnt = (double)P.count;
    const double ms = s / cnt;                                   // mean of (x - shift)
    double var = q / cnt - ms * ms;
    var = var > 0.0 ? var : 0.0;
    const float mean = (float)((double)sft + ms);
    const float invstd = (float)(1.0 / sqrt(var + (double)P.eps));
    const float sc = gam * invstd;
    typedef CHAP_GLOBAL float* gw;
    ((gw)P.scale)[c] = sc;
    ((gw)P.shift)[c] = bet - mean * sc;
    if (P.mean) { ((gw)P.mean)[c] = mean; ((gw)P.invstd)[c] = invstd; }
    if (upd) {
        const float unb = (float)(cnt > 1.0 ? var * cnt / (cnt - 1.0) : var);
        ((gw)P.running_mean)[c] = (1.f - P.momentum) * rm0 + P.momentum * mean;
        ((gw)P.running_var)[c] = (1.f - P.momentum) * rv0 + P.momentum * unb;
    }
}
extern "C" int chap_bn_finalize(const chap_bn_finalize_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->stats && p->gamma && p->beta && p->scale && p->shift && p->C > 0 && p->count > 0, "chap_bn_finalize: bad argument");
    CHAP_CHECK_ARG(p->Clog >= p->C && p->Clog % p->C == 0, "chap_bn_finalize: Clog=%d must be a multiple of C=%d", p->Clog, p->C);
    if (chap_lab_skip(KNOB_LAB_SKIP_BNFIN)) return CHAP_OK;      // lab builds only (tools/lab, loaded through CHAP_LIBPATH): timing bound, wrong numerics
    return chap_launch<chap_bn_finalize_params, bn_finalize_kernel, 256>(dim3(cdiv(p->C, 4)), dim3(256), 0, (hipStream_t)stream, *p, "chap_bn_finalize");
}

__device__ __forceinline__ void bn_eval_kernel(const chap_bn_eval_params& P) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= P.C) return;
    const float sc = P.gamma[c] * rsqrtf(P.running_var[c] + P.eps);
    P.scale[c] = sc;
    P.shift[c] = P.beta[c] - P.running_mean[c] * sc;
}
extern "C" int chap_bn_eval_affine(const chap_bn_eval_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->gamma && p->beta && p->running_mean && p->running_var && p->scale && p->shift && p->C > 0, "chap_bn_eval_affine: bad argument");
    return chap_launch<chap_bn_eval_params, bn_eval_kernel, 64>(dim3(cdiv(p->C, 64)), dim3(64), 0, (hipStream_t)stream, *p, "chap_bn_eval_affine");
}

// =========================================================================================
// A lazy source (chap_src_t) as the streaming kernels below ask for it: src_load8 (common.h) with its loads taken out of its branches.
// src_load8 loads the raw values, then -- each behind a branch on a pointer of the argument block -- scale and shift, the keep mask and
// the channel multipliers: up to three dependent memory round trips per pixel, and a kernel that walks several pixels per output
// (a pool window, the corners of an up-sampling cell) in a loop pays them once per pixel.  Here, as in act_issue below:
//  * the argument block is read once (chap_args_once) into a wave-uniform src_plan: byte base and byte stride of every part, presence;
//  * src_issue requests the keep mask and the raw values of one pixel, src_issue_cm the multipliers of one sample, with no branch between
//    the requests: a part the source does not have points at the 16 bytes of the pixel's own raw load -- a valid address whose line is
//    requested anyway -- and its value is never used.  A kernel requests ALL pixels of an output before it uses the first;
//  * src_finish applies affine -> LeakyReLU -> keep -> multipliers with src_load8's operations in src_load8's order: the same bits;
//  * scale and shift are requested once per thread, in front of the loop, where the thread's channel group is the same on every trip
//    (FIXC: gridDim.x * 256 a multiple of C / 8), and by src_issue_aff with the trip's loads otherwise;
//  * KM = false is the source without keep mask and multipliers: it requests raw only;
//  * A32: byte offsets are 32-bit, added to a scalar base, where the entry point saw every tensor below 4 GB; 64-bit otherwise.
// Who uses it: channel_sum_kernel, every instance; the 2D pool and the up-sampling cell kernel for KM = false and A32 = true (the "plain" kernels) --
// with a keep mask or multipliers in flight for 4 / 8 pixels they need more registers than the waves per SIMD of the general kernels allow
// (DESIGN.md section 5), so those sources, and tensors of 4 GB and more, keep the general kernels on src_load8.
template <typename T> struct act_pk;                        // 8 channels as loaded
template <> struct act_pk<bf16_t> { u32x4n v; };
template <> struct act_pk<float> { f32x4n a, b; };
__device__ __forceinline__ void pk_ld(chap_gptr p, act_pk<bf16_t>& r) { r.v = ldg<u32x4n>(p); }
__device__ __forceinline__ void pk_ld(chap_gptr p, act_pk<float>& r) { r.a = ldg<f32x4n>(p); r.b = ldg<f32x4n>(p + 16); }
__device__ __forceinline__ void pk_unpack(const act_pk<bf16_t>& r, float v[8]) {      // the conversions of ld8 (common.h)
    v[0] = __uint_as_float(r.v.x << 16); v[1] = __uint_as_float(r.v.x & 0xffff0000u);
    v[2] = __uint_as_float(r.v.y << 16); v[3] = __uint_as_float(r.v.y & 0xffff0000u);
    v[4] = __uint_as_float(r.v.z << 16); v[5] = __uint_as_float(r.v.z & 0xffff0000u);
    v[6] = __uint_as_float(r.v.w << 16); v[7] = __uint_as_float(r.v.w & 0xffff0000u);
}
__device__ __forceinline__ void pk_unpack(const act_pk<float>& r, float v[8]) {
    v[0] = r.a.x; v[1] = r.a.y; v[2] = r.a.z; v[3] = r.a.w; v[4] = r.b.x; v[5] = r.b.y; v[6] = r.b.z; v[7] = r.b.w;
}

template <bool A32> struct src_off { typedef u32 t; };
template <> struct src_off<false> { typedef unsigned long t; };
// wave-uniform: lives in scalar registers.  Element i of a part sits at base + i * stride + (the lane's channel offset), in bytes
struct src_plan {
    chap_gptr raw, keep, cm, scale, shift;
    u32 raw_stride, keep_stride, cm_stride;                 // per pixel (raw, keep mask), per sample (multipliers); an absent part has raw's
    bool has_aff, act, has_keep, has_cm;
    int cm_hi, aff_hi;                                      // byte offset of channels 4..7 of the multipliers / of scale and shift (0 where they alias the raw load)
    float slope, keep_scale;
};
template <typename T>
__device__ __forceinline__ src_plan src_make_plan(const chap_src_t& r) {
    constexpr u32 ES = sizeof(T);
    src_plan S;
    const u32 C = (u32)r.C;
    S.raw = chap_global(r.ptr) + (long)r.coff * ES; S.raw_stride = (u32)r.ld * ES;
    S.has_aff = r.scale != nullptr; S.act = r.act != 0; S.has_keep = r.keep != nullptr; S.has_cm = r.chan_mul != nullptr;
    S.scale = chap_global(r.scale); S.shift = chap_global(r.shift);
    S.keep = S.has_keep ? chap_global(r.keep) : S.raw; S.keep_stride = S.has_keep ? C : S.raw_stride;
    S.cm = S.has_cm ? chap_global(r.chan_mul) : S.raw; S.cm_stride = S.has_cm ? C * 4 : S.raw_stride;
    S.cm_hi = S.has_cm ? 16 : 0; S.aff_hi = S.has_aff ? 16 : 0;
    S.slope = r.slope; S.keep_scale = r.keep_scale;
    return S;
}
// the lane's channel offset in bytes: of the element type (raw), of the byte mask (an absent mask reads the first 8 bytes of the lane's own
// raw unit or of an earlier one of the same pixel: c8 <= c8 * sizeof(T)), of the multipliers, of scale and shift
struct src_lane { int t, b, cm, c4; };
template <typename T>
__device__ __forceinline__ src_lane src_make_lane(const src_plan& S, int c8) { return {c8 * (int)sizeof(T), c8, S.has_cm ? c8 * 4 : c8 * (int)sizeof(T), c8 * 4}; }

template <typename T> struct src_trip { act_pk<T> raw; u32x2n keep; };       // one pixel as loaded
struct src_vec8 { f32x4n lo, hi; };                                          // 8 floats as loaded: multipliers, scale, shift
__device__ __forceinline__ void vec8_unpack(const src_vec8& m, float v[8]) { v[0] = m.lo.x; v[1] = m.lo.y; v[2] = m.lo.z; v[3] = m.lo.w; v[4] = m.hi.x; v[5] = m.hi.y; v[6] = m.hi.z; v[7] = m.hi.w; }

template <bool A32>
__device__ __forceinline__ chap_gptr src_addr(chap_gptr base, u32 stride, typename src_off<A32>::t i, int lane) {
    typedef typename src_off<A32>::t OFF;
    return base + (OFF)(i * (OFF)stride + (OFF)lane);       // A32: scalar base + 32-bit lane offset, no 64-bit address kept or computed per lane
}
// keep mask and raw values of pixel `pix`.  The raw load goes LAST: loads return in order, so the wait in front of a pixel's first use covers the pixel
template <typename T, bool KM, bool A32>
__device__ __forceinline__ void src_issue(const src_plan& S, const src_lane& L, typename src_off<A32>::t pix, src_trip<T>& t) {
    if (KM) t.keep = ldg<u32x2n>(src_addr<A32>(S.keep, S.keep_stride, pix, L.b));
    pk_ld(src_addr<A32>(S.raw, S.raw_stride, pix, L.t), t.raw);
}
// the multipliers of sample `n`; `pix`: any pixel the caller requests on this trip (what an absent part aliases)
template <bool KM, bool A32>
__device__ __forceinline__ void src_issue_cm(const src_plan& S, const src_lane& L, int n, typename src_off<A32>::t pix, src_vec8& m) {
    typedef typename src_off<A32>::t OFF;
    if (!KM) return;
    const chap_gptr cp = src_addr<A32>(S.cm, S.cm_stride, S.has_cm ? (OFF)n : pix, L.cm);
    m.lo = ldg<f32x4n>(cp); m.hi = ldg<f32x4n>(cp + S.cm_hi);
}
// scale and shift of the lane's channels with a trip's loads (the kernels whose threads change their channel group between trips)
template <bool A32>
__device__ __forceinline__ void src_issue_aff(const src_plan& S, const src_lane& L, typename src_off<A32>::t pix, src_vec8& a, src_vec8& b) {
    const chap_gptr rp = src_addr<A32>(S.raw, S.raw_stride, pix, L.t);
    const chap_gptr ap = S.has_aff ? S.scale + L.c4 : rp, bp = S.has_aff ? S.shift + L.c4 : rp;
    a.lo = ldg<f32x4n>(ap); a.hi = ldg<f32x4n>(ap + S.aff_hi); b.lo = ldg<f32x4n>(bp); b.hi = ldg<f32x4n>(bp + S.aff_hi);
}
// ... in front of the loop (one wave-uniform branch, once per thread)
__device__ __forceinline__ void src_load_aff(const src_plan& S, const src_lane& L, float sa[8], float sb[8]) {
    if (S.has_aff) { ld8g(S.scale + L.c4, sa); ld8g(S.shift + L.c4, sb); }
}
// src_load8's arithmetic on a loaded pixel: v = cm * keep * keep_scale * leaky(scale * raw + shift), every step where the source has it
template <typename T, bool KM>
__device__ __forceinline__ void src_finish(const src_plan& S, const src_trip<T>& t, const src_vec8& m, const float sa[8], const float sb[8], float v[8]) {
    pk_unpack(t.raw, v);
    if (S.has_aff) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaf(v[j], sa[j], sb[j]);
    }
    if (S.act) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] > 0.f ? v[j] : v[j] * S.slope;
    }
    if (KM && S.has_keep) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t w = j < 4 ? t.keep.x : t.keep.y;
            v[j] = ((w >> (8 * (j & 3))) & 0xff) ? v[j] * S.keep_scale : 0.f;
        }
    }
    if (KM && S.has_cm) {
        float a[8];
        vec8_unpack(m, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= a[j];
    }
}
// what an entry point needs to pick the instance: KM = the source has a keep mask or multipliers
static inline bool src_has_km(const chap_src_t& r) { return r.keep != nullptr || r.chan_mul != nullptr; }
// ... and whether `pixels` pixels of a tensor with pixel stride `ld` elements stay below the 4 GB that 32-bit byte offsets reach
static inline bool src_fits32(long pixels, long ld, int dtype) { return pixels * ld * (dtype == CHAP_BF16 ? 2 : 4) < (1l << 32); }

// =========================================================================================
// 2x2 max-pool of a lazy activation. One thread per (pooled pixel, 8 channels).
// The general form: any source, any size, one sample of the window at a time through src_load8.
template <typename T>
__device__ __forceinline__ void act_pool2_kernel(const chap_pool_params& P) {
    const int D = P.D > 1 ? P.D : 1, KZ = P.D > 1 ? 2 : 1;
    const int C8 = P.r.C / 8, OD = D / KZ, OH = P.H / 2, OW = P.W / 2;
    const long total = (long)P.N * OD * OH * OW * C8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; u32 r = ui / (u32)C8;
        const int ox = (int)(r % (u32)OW); r /= (u32)OW;
        const int oy = (int)(r % (u32)OH); r /= (u32)OH;
        const int oz = (int)(r % (u32)OD); const int n = (int)(r / (u32)OD);
        float best[8]; uint32_t bi[8];
        for (int k = 0; k < 4 * KZ; ++k) {
            const long pix = (((long)n * D + KZ * oz + (k >> 2)) * P.H + 2 * oy + ((k >> 1) & 1)) * P.W + 2 * ox + (k & 1);
            float v[8];
            src_load8<T>(P.r, n, pix, c8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k == 0 || v[j] > best[j] || v[j] != v[j]) { best[j] = v[j]; bi[j] = k; }
        }
        const long op = (((long)n * OD + oz) * OH + oy) * OW + ox;
        st8((T*)P.out + op * P.r.C + c8, best);
        if (P.idx) {
            uint2 m;
            m.x = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
            m.y = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
            *(uint2*)(P.idx + op * P.r.C + c8) = m;
        }
    }
}
// The 2D pool of a plain source (neither keep mask nor channel multipliers) below 4 GB -- every pool of the 2D training step.
// All 4 samples of the window are requested together, then compared in the window's order k = 0, 1, 2, 3: the first maximum wins, a NaN replaces.
// (Not the 3D window: 8 samples in flight take 122 to 126 registers, and one z plane at a time still more than the 80 of the 6 waves per SIMD the
// general form runs at; nor keep mask / multipliers: 85 to 96.)
template <typename T, bool FIXC>
__device__ __forceinline__ void act_pool2_plain_body(const chap_pool_params& P, const src_plan& S) {
    constexpr int ES = sizeof(T);
    const int C = P.r.C, C8 = C / 8, OH = P.H / 2, OW = P.W / 2, W = P.W;
    const long total = (long)P.N * OH * OW * C8;
    CHAP_GLOBAL char* const out = (CHAP_GLOBAL char*)P.out; CHAP_GLOBAL char* const idx = (CHAP_GLOBAL char*)P.idx;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    float sa[8], sb[8];
    if (FIXC) src_load_aff(S, src_make_lane<T>(S, (int)((u32)i % (u32)C8) * 8), sa, sb);
    for (; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; u32 r = ui / (u32)C8;
        const u32 ox = r % (u32)OW; r /= (u32)OW;      // r: n * OH + oy, and H = 2 * OH
        const src_lane L = src_make_lane<T>(S, c8);
        const u32 p0 = (2 * r) * (u32)W + 2 * ox;      // sample k = 0 of the window
        src_trip<T> w[4]; src_vec8 m, fa, fb;
        if (!FIXC) src_issue_aff<true>(S, L, p0, fa, fb);
#pragma unroll
        for (int k = 0; k < 4; ++k) src_issue<T, false, true>(S, L, p0 + (u32)((k >> 1) * W + (k & 1)), w[k]);
        if (!FIXC) { vec8_unpack(fa, sa); vec8_unpack(fb, sb); }
        float best[8]; uint32_t bi[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v[8];
            src_finish<T, false>(S, w[k], m, sa, sb, v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k == 0 || v[j] > best[j] || v[j] != v[j]) { best[j] = v[j]; bi[j] = k; }
        }
        const u32 op = r * (u32)OW + ox;
        st8g((CHAP_GLOBAL T*)(out + (u32)((op * C + c8) * ES)), best);
        if (idx) {
            u32x2n mm;
            mm.x = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
            mm.y = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
            *(CHAP_GLOBAL u32x2n*)(idx + (u32)(op * C + c8)) = mm;
        }
    }
}
template <typename T>
__device__ __forceinline__ void act_pool2_plain_kernel(const chap_pool_params& Pk) {
    const chap_pool_params P = chap_args_once(Pk);
    const src_plan S = src_make_plan<T>(P.r);
    if ((gridDim.x * 256u) % (u32)(P.r.C / 8) == 0) act_pool2_plain_body<T, true>(P, S);       // (wave-uniform)
    else act_pool2_plain_body<T, false>(P, S);
}
template <typename T>
static int act_pool2_launch(const chap_pool_params* p, bool plain, int blocks, hipStream_t s) {
    const dim3 g(blocks), b(256);
    if (plain) return chap_launch<chap_pool_params, act_pool2_plain_kernel<T>, 256, 6>(g, b, 0, s, *p, "chap_act_pool2");      // (6 waves per SIMD: as the general form)
    return chap_launch<chap_pool_params, act_pool2_kernel<T>, 256>(g, b, 0, s, *p, "chap_act_pool2");
}
extern "C" int chap_act_pool2(const chap_pool_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->r.ptr && p->out, "chap_act_pool2: null argument");
    CHAP_CHECK_ARG(p->r.C % 8 == 0 && p->H % 2 == 0 && p->W % 2 == 0 && (p->D <= 1 || p->D % 2 == 0), "chap_act_pool2: C%%8, even dims required");
    if (chap_lab_skip(KNOB_LAB_SKIP_POOL)) return CHAP_OK;      // lab builds only: timing bound (wrong numerics) of fusing this launch into its consumer
    const long total = (long)p->N * (p->D > 1 ? p->D / 2 : 1) * (p->H / 2) * (p->W / 2) * (p->r.C / 8);
    const int blocks = chap_blocks(total, 4096);
    const bool plain = p->D <= 1 && !src_has_km(p->r) && src_fits32((long)p->N * p->H * p->W, p->r.ld > p->r.C ? p->r.ld : p->r.C, p->dtype);      // (the pooled output is smaller)
    if (p->dtype == CHAP_BF16) return act_pool2_launch<bf16_t>(p, plain, blocks, (hipStream_t)stream);
    return act_pool2_launch<float>(p, plain, blocks, (hipStream_t)stream);
}

// =========================================================================================
// 2x upsample, align_corners=True: src = dst * (in-1)/(out-1)  (F.interpolate bilinear/trilinear).
__device__ __forceinline__ void ac_coord(int o, int in, int out, int& i0, int& i1, float& w1, bool half_pixel = false) {
    const float sc = half_pixel ? (float)in / (float)out : (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f);
    float f = half_pixel ? sc * ((float)o + 0.5f) - 0.5f : sc * (float)o;     // area_pixel_compute_source_index
    if (f < 0.f) f = 0.f;
    i0 = (int)f;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    w1 = f - (float)i0;
}

template <typename T>
__device__ __forceinline__ void upsample2x_kernel(const chap_upsample_params& P) {
    const int C8 = P.r.C / 8;
    const int OD = P.dims == 3 ? 2 * P.D : P.D, OH = 2 * P.H, OW = 2 * P.W;
    const long total = (long)P.N * OD * OH * OW * C8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; u32 r = ui / (u32)C8;
        const int ox = (int)(r % (u32)OW); r /= (u32)OW;
        const int oy = (int)(r % (u32)OH); r /= (u32)OH;
        const int oz = (int)(r % (u32)OD); const int n = (int)(r / (u32)OD);
        int x0, x1, y0, y1, z0, z1; float wx, wy, wz;
        const bool hp = P.half_pixel != 0;
        ac_coord(ox, P.W, OW, x0, x1, wx, hp);
        ac_coord(oy, P.H, OH, y0, y1, wy, hp);
        if (P.dims == 3) ac_coord(oz, P.D, OD, z0, z1, wz, hp); else { z0 = z1 = oz; wz = 0.f; }
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        const int nz = P.dims == 3 ? 2 : 1;
        for (int kz = 0; kz < nz; ++kz)
            for (int ky = 0; ky < 2; ++ky)
                for (int kx = 0; kx < 2; ++kx) {
                    const float w = (kz ? wz : 1.f - wz) * (ky ? wy : 1.f - wy) * (kx ? wx : 1.f - wx);
                    const long pix = (((long)n * P.D + (kz ? z1 : z0)) * P.H + (ky ? y1 : y0)) * P.W + (kx ? x1 : x0);
                    float v[8];
                    src_load8<T>(P.r, n, pix, c8, v);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, v[j], acc[j]);
                }
        const long op = (((long)n * OD + oz) * OH + oy) * OW + ox;
        st8((T*)P.out + op * P.out_ld + P.out_coff + c8, acc);
    }
}
// Cell form (used whenever every interpolated axis has >= 2 input samples): one thread owns one input CELL
// (the interval [i, i+1] on each interpolated axis) and 8 channels, loads and transforms (lazy activation) its
// 4 / 8 corner samples ONCE and writes every output sample whose source coordinate falls into the cell (2 per
// axis on average for x2).  The per-output form above re-loads and re-transforms the corners for each output:
// 8x the loads and VALU work in 3D.  Same weights, same summation order as the per-output form.
__device__ __forceinline__ int up_axis_outputs(int i, int in, int out, bool hp, int o_[5], float w_[5]) {
    int n = 0;
    for (int o = max(0, 2 * i - 1); o <= min(out - 1, 2 * i + 3); ++o) {      // 2i+3: only the clamped last output of the last cell
        int i0, i1; float w1;
        ac_coord(o, in, out, i0, i1, w1, hp);
        if (i0 > in - 2) { i0 = in - 2; w1 = 1.f; }             // source clamped to the last sample: corner 1 with weight 1
        if (i0 == i) { o_[n] = o; w_[n] = w1; ++n; }
    }
    return n;
}
// The general form: any source, any size, the corners one after the other through src_load8.
template <typename T, bool D3>
__device__ __forceinline__ void upsample2x_cell_kernel(const chap_upsample_params& P) {
    const int C8 = P.r.C / 8;
    const int OD = D3 ? 2 * P.D : P.D, OH = 2 * P.H, OW = 2 * P.W;
    const int CD = D3 ? P.D - 1 : P.D, CH = P.H - 1, CW = P.W - 1;       // cells per axis
    const long total = (long)P.N * CD * CH * CW * C8;
    const bool hp = P.half_pixel != 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; u32 r = ui / (u32)C8;
        const int cx = (int)(r % (u32)CW); r /= (u32)CW;
        const int cy = (int)(r % (u32)CH); r /= (u32)CH;
        const int cz = (int)(r % (u32)CD); const int n = (int)(r / (u32)CD);
        float v[D3 ? 2 : 1][2][2][8];
#pragma unroll
        for (int kz = 0; kz < (D3 ? 2 : 1); ++kz)
#pragma unroll
            for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                for (int kx = 0; kx < 2; ++kx)
                    src_load8<T>(P.r, n, (((long)n * P.D + cz + kz) * P.H + cy + ky) * P.W + cx + kx, c8, v[kz][ky][kx]);
        int oz_[5], oy_[5], ox_[5]; float wz_[5], wy_[5], wx_[5];
        int nz = 1; oz_[0] = cz; wz_[0] = 0.f;
        if (D3) nz = up_axis_outputs(cz, P.D, OD, hp, oz_, wz_);
        const int ny = up_axis_outputs(cy, P.H, OH, hp, oy_, wy_);
        const int nx = up_axis_outputs(cx, P.W, OW, hp, ox_, wx_);
        for (int a = 0; a < nz; ++a)
            for (int b = 0; b < ny; ++b)
                for (int c = 0; c < nx; ++c) {
                    const float wz = wz_[a], wy = wy_[b], wx = wx_[c];
                    float acc[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
                    for (int kz = 0; kz < (D3 ? 2 : 1); ++kz)
#pragma unroll
                        for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                            for (int kx = 0; kx < 2; ++kx) {
                                const float w = (kz ? wz : 1.f - wz) * (ky ? wy : 1.f - wy) * (kx ? wx : 1.f - wx);
#pragma unroll
                                for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, v[kz][ky][kx][j], acc[j]);
                            }
                    const long op = (((long)n * OD + oz_[a]) * OH + oy_[b]) * OW + ox_[c];
                    st8((T*)P.out + op * P.out_ld + P.out_coff + c8, acc);
                }
    }
}
// The plain source (neither keep mask nor channel multipliers) below 4 GB.
// The 4 / 8 corners are requested together (src_issue), then transformed (src_finish): one memory round trip per cell.
template <typename T, bool KM, bool A32, bool D3, bool FIXC>
__device__ __forceinline__ void upsample2x_cell_plain_body(const chap_upsample_params& P, const src_plan& S) {
    typedef typename src_off<A32>::t OFF;
    constexpr int NZ = D3 ? 2 : 1, ES = sizeof(T);
    const int C8 = P.r.C / 8, D = P.D, H = P.H, W = P.W;
    const int OD = D3 ? 2 * D : D, OH = 2 * H, OW = 2 * W;
    const int CD = D3 ? D - 1 : D, CH = H - 1, CW = W - 1;       // cells per axis
    const long total = (long)P.N * CD * CH * CW * C8;
    const bool hp = P.half_pixel != 0;
    CHAP_GLOBAL char* const out = (CHAP_GLOBAL char*)P.out + (long)P.out_coff * ES;
    const OFF out_ld = (OFF)P.out_ld;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    float sa[8], sb[8];
    if (FIXC) src_load_aff(S, src_make_lane<T>(S, (int)((u32)i % (u32)C8) * 8), sa, sb);
    for (; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; u32 r = ui / (u32)C8;
        const int cx = (int)(r % (u32)CW); r /= (u32)CW;
        const int cy = (int)(r % (u32)CH); r /= (u32)CH;
        const int cz = (int)(r % (u32)CD); const int n = (int)(r / (u32)CD);
        const src_lane L = src_make_lane<T>(S, c8);
        const OFF p0 = (((OFF)n * D + cz) * H + cy) * W + cx;             // corner (0, 0, 0) of the cell
        src_trip<T> t[NZ][2][2]; src_vec8 m, fa, fb;
        if (!FIXC) src_issue_aff<A32>(S, L, p0, fa, fb);
        src_issue_cm<KM, A32>(S, L, n, p0, m);
#pragma unroll
        for (int kz = 0; kz < NZ; ++kz)
#pragma unroll
            for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                for (int kx = 0; kx < 2; ++kx) src_issue<T, KM, A32>(S, L, p0 + (OFF)((kz * H + ky) * W + kx), t[kz][ky][kx]);
        if (!FIXC) { vec8_unpack(fa, sa); vec8_unpack(fb, sb); }
        float v[NZ][2][2][8];
#pragma unroll
        for (int kz = 0; kz < NZ; ++kz)
#pragma unroll
            for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                for (int kx = 0; kx < 2; ++kx) src_finish<T, KM>(S, t[kz][ky][kx], m, sa, sb, v[kz][ky][kx]);
        int oz_[5], oy_[5], ox_[5]; float wz_[5], wy_[5], wx_[5];
        int nz = 1; oz_[0] = cz; wz_[0] = 0.f;
        if (D3) nz = up_axis_outputs(cz, D, OD, hp, oz_, wz_);
        const int ny = up_axis_outputs(cy, H, OH, hp, oy_, wy_);
        const int nx = up_axis_outputs(cx, W, OW, hp, ox_, wx_);
        for (int a = 0; a < nz; ++a)
            for (int b = 0; b < ny; ++b)
                for (int c = 0; c < nx; ++c) {
                    const float wz = wz_[a], wy = wy_[b], wx = wx_[c];
                    float acc[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
                    for (int kz = 0; kz < NZ; ++kz)
#pragma unroll
                        for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                            for (int kx = 0; kx < 2; ++kx) {
                                const float w = (kz ? wz : 1.f - wz) * (ky ? wy : 1.f - wy) * (kx ? wx : 1.f - wx);
#pragma unroll
                                for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, v[kz][ky][kx][j], acc[j]);
                            }
                    const OFF op = (((OFF)n * OD + oz_[a]) * OH + oy_[b]) * OW + ox_[c];
                    st8g((CHAP_GLOBAL T*)(out + (OFF)((op * out_ld + c8) * ES)), acc);
                }
    }
}
template <typename T, bool KM, bool A32, bool D3>
__device__ __forceinline__ void upsample2x_cell_plain_kernel(const chap_upsample_params& Pk) {
    const chap_upsample_params P = chap_args_once(Pk);
    const src_plan S = src_make_plan<T>(P.r);
    if ((gridDim.x * 256u) % (u32)(P.r.C / 8) == 0) upsample2x_cell_plain_body<T, KM, A32, D3, true>(P, S);      // (wave-uniform)
    else upsample2x_cell_plain_body<T, KM, A32, D3, false>(P, S);
}
// (5 waves per SIMD in 2D, 3 in 3D: what the kernel ran at before the corners were in flight together)
template <typename T, bool D3>
static int upsample2x_cell_launch(const chap_upsample_params* p, bool a32, int blocks, hipStream_t s) {
    const dim3 g(blocks), b(256);
    // (with a keep mask or multipliers in flight per corner: 100 to 108 registers in 2D, 4 waves per SIMD, or scratch: the general form)
    if (!a32 || src_has_km(p->r)) return chap_launch<chap_upsample_params, upsample2x_cell_kernel<T, D3>, 256>(g, b, 0, s, *p, "chap_upsample2x");
    return chap_launch<chap_upsample_params, upsample2x_cell_plain_kernel<T, false, true, D3>, 256, D3 ? 3 : 5>(g, b, 0, s, *p, "chap_upsample2x");
}
extern "C" int chap_upsample2x(const chap_upsample_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->r.ptr && p->out && p->r.C % 8 == 0, "chap_upsample2x: bad argument");
    CHAP_CHECK_ARG(p->out_ld % 8 == 0 && p->out_coff % 8 == 0, "chap_upsample2x: out_ld/out_coff must be multiples of 8");
    if (chap_lab_skip(KNOB_LAB_SKIP_UPSAMPLE)) return CHAP_OK;      // lab builds only: timing bound (wrong numerics) of fusing this launch into its consumer
    const bool d3 = p->dims == 3;
    if (p->H >= 2 && p->W >= 2 && (!d3 || p->D >= 2)) {
        const long cells = (long)p->N * (d3 ? p->D - 1 : p->D) * (p->H - 1) * (p->W - 1) * (p->r.C / 8);
        const int blocks = chap_blocks(cells, 16384);
        hipStream_t s = (hipStream_t)stream;
        const long ipix = (long)p->N * p->D * p->H * p->W;
        const bool a32 = src_fits32(ipix, p->r.ld > p->r.C ? p->r.ld : p->r.C, p->dtype) && src_fits32(ipix * (d3 ? 8 : 4), p->out_ld, p->dtype);
        if (p->dtype == CHAP_BF16) return d3 ? upsample2x_cell_launch<bf16_t, true>(p, a32, blocks, s) : upsample2x_cell_launch<bf16_t, false>(p, a32, blocks, s);
        return d3 ? upsample2x_cell_launch<float, true>(p, a32, blocks, s) : upsample2x_cell_launch<float, false>(p, a32, blocks, s);
    }
    const long total = (long)p->N * (p->dims == 3 ? 2 * p->D : p->D) * 2 * p->H * 2 * p->W * (p->r.C / 8);
    const int blocks = chap_blocks(total, 8192);
    if (p->dtype == CHAP_BF16) return chap_launch<chap_upsample_params, upsample2x_kernel<bf16_t>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_upsample2x");
    return chap_launch<chap_upsample_params, upsample2x_kernel<float>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_upsample2x");
}


// Adjoint: each coarse pixel gathers from the fine pixels whose stencil touches it (no atomics).
// Along one axis, fine index o touches coarse i iff i0(o) == i or i1(o) == i; with scale
// (in-1)/(out-1) < 1/2 only o in [2i-2, 2i+2] can qualify, so a 5-wide window per axis suffices.
// weight with which fine sample o feeds coarse sample i along one axis (0 when its stencil does not touch i)
__device__ __forceinline__ int up_axis_adjoint(int i, int in, int out, int o_[5], float w_[5]) {
    int n = 0;
    for (int o = max(0, 2 * i - 2); o <= min(out - 1, 2 * i + 2); ++o) {
        int a0, a1; float w1;
        ac_coord(o, in, out, a0, a1, w1);
        const float w = (a0 == i ? 1.f - w1 : 0.f) + (a1 == i ? w1 : 0.f);
        if (w != 0.f) { o_[n] = o; w_[n] = w; ++n; }
    }
    return n;
}
template <typename T>
__device__ __forceinline__ void upsample2x_bwd_kernel(const chap_upsample_bwd_params& P) {
    const int C8 = P.C / 8;
    const int OD = P.dims == 3 ? 2 * P.D : P.D, OH = 2 * P.H, OW = 2 * P.W;
    const long total = (long)P.N * P.D * P.H * P.W * C8;
    const T* g = (const T*)P.g;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; u32 r = ui / (u32)C8;
        const int x = (int)(r % (u32)P.W); r /= (u32)P.W;
        const int y = (int)(r % (u32)P.H); r /= (u32)P.H;
        const int z = (int)(r % (u32)P.D); const int n = (int)(r / (u32)P.D);
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        // per-axis contributor lists first (the nested form evaluated the source coordinate 5*5*5 times per thread)
        int oz_[5], oy_[5]; float wz_[5], wy_[5];
        int nz = 1; oz_[0] = z; wz_[0] = 1.f;
        if (P.dims == 3) nz = up_axis_adjoint(z, P.D, OD, oz_, wz_);
        const int ny = up_axis_adjoint(y, P.H, OH, oy_, wy_);
        // x: the FIXED window 2x-2 .. 2x+2, clamped, weight 0 where a sample does not touch x (or lies outside): the five loads of a
        // (z, y) row are issued together instead of one dependent load per trip of a runtime-bounded loop (the kernel was load-latency
        // bound: ~70 serial 16-byte loads per thread).  Contributions are added in the same ascending order as before, zero-weight
        // ones skipped: bit-identical results.
        int ox_[5]; float wx_[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int o = 2 * x - 2 + k, oc = min(max(o, 0), OW - 1);
            int a0, a1; float w1;
            ac_coord(oc, P.W, OW, a0, a1, w1);
            const float w = (a0 == x ? 1.f - w1 : 0.f) + (a1 == x ? w1 : 0.f);
            ox_[k] = oc; wx_[k] = (o == oc) ? w : 0.f;
        }
        for (int a = 0; a < nz; ++a)
            for (int b = 0; b < ny; ++b) {
                const long row = (((long)n * OD + oz_[a]) * OH + oy_[b]) * OW;
                const float wzy = wz_[a] * wy_[b];
                float v[5][8];
#pragma unroll
                for (int c = 0; c < 5; ++c) ld8(g + (row + ox_[c]) * P.g_ld + P.g_coff + c8, v[c]);
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const float w = wzy * wx_[c];
                    if (wx_[c] != 0.f) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, v[c][j], acc[j]);
                    }
                }
            }
        const long cp = (((long)n * P.D + z) * P.H + y) * P.W + x;
        st8((T*)P.out + cp * P.C + c8, acc);
    }
}
extern "C" int chap_upsample2x_bwd(const chap_upsample_bwd_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->g && p->out && p->C % 8 == 0 && p->g_ld % 8 == 0 && p->g_coff % 8 == 0, "chap_upsample2x_bwd: bad argument");
    if (chap_lab_skip(KNOB_LAB_SKIP_UPSAMPLE_BWD)) return CHAP_OK;      // lab builds only: timing bound (wrong numerics) of fusing this launch into its consumer
    const long total = (long)p->N * p->D * p->H * p->W * (p->C / 8);
    const int blocks = chap_blocks(total, 8192);
    if (p->dtype == CHAP_BF16) return chap_launch<chap_upsample_bwd_params, upsample2x_bwd_kernel<bf16_t>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_upsample2x_bwd");
    return chap_launch<chap_upsample_bwd_params, upsample2x_bwd_kernel<float>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_upsample2x_bwd");
}

// =========================================================================================
// Backward through the lazy activation (+ pooled consumer) and training-mode BatchNorm.
// Thread = (pixel, 8 channels); a block covers 256/C8 pixels per step, grid-stride; per-channel
// partial sums are reduced over the block in a fixed order and stored as this block's partial row
// (sums layout: [1 + CHAP_ACT_BWD_SLOTS][2][C], row 0 = totals written by act_bwd_sum_kernel).
//
// How a thread asks for its data (the arithmetic and the order of every sum are those of actbwd_math.h and never depend on it):
//  * the kernel arguments are copied into an act_plan ONCE, in front of everything: byte base, byte stride and presence of every source;
//  * all loads of a trip are requested together, with no branch between them (the rule noted in halo_commit_impl, conv_kernel.h): a source
//    the layer does not have (gradients 1 and 2, pooled gradient and index, keep mask, channel multipliers) points at the 16 bytes of the raw
//    load of the same trip -- a valid address that is in the cache already -- and its value is never used.  The raw load goes LAST: loads
//    return in order, so the wait in front of the first use of a trip covers the whole trip;
//  * the next trip is requested as soon as the current one is consumed.  The pixel of the request is clamped to the last one, so a lane past
//    the end (the ragged last trip) asks for an address inside the tensors;
//  * GEN = false is the layer with exactly one incoming gradient and neither pooled gradient nor channel multipliers (21 of the 26
//    BatchNorm layers of the 2D step): it requests raw, that gradient and the keep mask only.  GEN = true takes every layer;
//  * reduce: the per-channel constants and the first trip go out together, one memory round trip in front of the loop (the general fp32
//    instance: two).  apply: two (see the prologue of act_bwd_kernel for both).
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct act_src1 { chap_gptr base; u32 stride; };         // bytes; element i of the source sits at base + i * stride + (the lane's channel offset), all of it below 2^32
// wave-uniform: lives in scalar registers
struct act_plan {
    act_src1 raw, g[3], gp, idx, keep, cm;
    bool has_g[3], has_pool, has_keep, has_cm, need_coords, act;
    int cm_hi;                                              // byte offset of channels 4..7 of the multipliers (0 when they alias the raw load)
    int W, H, D;
    float slope, keep_scale;
};
template <typename T>
__device__ __forceinline__ act_plan act_make_plan(const chap_act_bwd_params& P) {
    constexpr u32 ES = sizeof(T);
    act_plan S;
    const u32 C = (u32)P.r.C;
    S.raw = {chap_global(P.r.ptr) + (long)P.r.coff * ES, (u32)P.r.ld * ES};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        S.has_g[k] = k < P.ng;
        S.g[k] = S.has_g[k] ? act_src1{chap_global(P.g[k]) + (long)P.g_coff[k] * ES, (u32)P.g_ld[k] * ES} : S.raw;
    }
    S.has_pool = P.g_pool != nullptr; S.has_keep = P.r.keep != nullptr; S.has_cm = P.r.chan_mul != nullptr;
    S.gp = S.has_pool ? act_src1{chap_global(P.g_pool), C * ES} : S.raw;
    S.idx = S.has_pool ? act_src1{chap_global(P.pool_idx), C} : S.raw;
    S.keep = S.has_keep ? act_src1{chap_global(P.r.keep), C} : S.raw;
    S.cm = S.has_cm ? act_src1{chap_global(P.r.chan_mul), C * 4} : S.raw;
    S.cm_hi = S.has_cm ? 16 : 0;
    S.need_coords = S.has_pool || S.has_cm;
    S.act = P.r.act != 0;
    S.W = P.W; S.H = P.H; S.D = P.D;
    S.slope = P.r.slope; S.keep_scale = P.r.keep_scale;
    return S;
}
// the lane's channel offset in bytes: of the element type (raw, gradients), of the byte masks (an absent mask reads the first 8 bytes
// of the lane's own raw unit or of an earlier one: c8 <= c8 * sizeof(T)), of the multipliers
struct act_lane { int t, b, cm; };

template <typename T> struct act_trip { act_pk<T> raw, g0, g1, g2, gp; u32x2n idx, keep; f32x4n cm0, cm1; uint32_t me; };

__device__ __forceinline__ chap_gptr act_addr(const act_src1& s, u32 i, int lane) { return s.base + (u32)(i * s.stride + (u32)lane); }      // scalar base + 32-bit lane offset: no 64-bit address kept or computed per lane (the entry points check the 4 GB this assumes)
template <typename T, bool GEN>
__device__ __forceinline__ void act_issue(const act_plan& S, const act_lane& L, u32 pix, act_trip<T>& t) {
    if (GEN) {
        u32 pidx = pix, nidx = pix;
        t.me = 0;
        if (S.need_coords) {                       // wave-uniform, no load inside: only the pooled gradient / Dropout3d path needs (n, y, x)
            const u32 up = pix;
            const int x = (int)(up % (u32)S.W); u32 r = up / (u32)S.W;
            const int y = (int)(r % (u32)S.H); r /= (u32)S.H;
            const int n = (int)(r / (u32)S.D);
            const int OH = S.H / 2, OW = S.W / 2;
            const u32 pp = ((u32)n * OH + (y >> 1)) * OW + (x >> 1);
            t.me = ((y & 1) << 1) | (x & 1);
            pidx = S.has_pool ? pp : pix; nidx = S.has_cm ? (u32)n : pix;
        }
        pk_ld(act_addr(S.g[0], pix, L.t), t.g0);
        pk_ld(act_addr(S.g[1], pix, L.t), t.g1);
        pk_ld(act_addr(S.g[2], pix, L.t), t.g2);
        pk_ld(act_addr(S.gp, pidx, L.t), t.gp);
        t.idx = ldg<u32x2n>(act_addr(S.idx, pidx, L.b));
        const chap_gptr cp = act_addr(S.cm, nidx, L.cm);
        t.cm0 = ldg<f32x4n>(cp); t.cm1 = ldg<f32x4n>(cp + S.cm_hi);
    } else {
        pk_ld(act_addr(S.g[0], pix, L.t), t.g0);
    }
    t.keep = ldg<u32x2n>(act_addr(S.keep, pix, L.b));
    pk_ld(act_addr(S.raw, pix, L.t), t.raw);
}

// the incoming gradient of one trip: ((0 + g0) + g1) + g2, then the routed pooled gradient
template <typename T, bool GEN>
__device__ __forceinline__ void act_gsum(const act_plan& S, const act_trip<T>& t, float gsum[8]) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gsum[j] = 0.f;
    if (!GEN || S.has_g[0]) {
        pk_unpack(t.g0, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) gsum[j] += v[j];
    }
    if (GEN) {
        if (S.has_g[1]) {
            pk_unpack(t.g1, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) gsum[j] += v[j];
        }
        if (S.has_g[2]) {
            pk_unpack(t.g2, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) gsum[j] += v[j];
        }
        if (S.has_pool) {
            pk_unpack(t.gp, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t w = j < 4 ? t.idx.x : t.idx.y;
                if (((w >> (8 * (j & 3))) & 0xff) == t.me) gsum[j] += v[j];
            }
        }
    }
}
// ... and dz from it: a = keep*ks*cm*leaky(z), z = scale*raw+shift  ->  da/dz = keep*ks*cm*(z>0 ? 1 : slope)      (actbwd_math.h)
template <typename T, bool GEN>
__device__ __forceinline__ void act_bwd_dz(const act_plan& S, const act_trip<T>& t, const float gsum[8], const float sa[8], const float sb[8], float raw[8], float dz[8]) {
    pk_unpack(t.raw, raw);
    actbwd_deriv8(raw, gsum, sa, sb, S.act, S.slope, dz);
    if (S.has_keep) actbwd_keep8(dz, make_uint2(t.keep.x, t.keep.y), S.keep_scale);
    if (GEN && S.has_cm) {
        const float cm[8] = {t.cm0.x, t.cm0.y, t.cm0.z, t.cm0.w, t.cm1.x, t.cm1.y, t.cm1.z, t.cm1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) dz[j] *= cm[j];
    }
}

template <typename T, bool APPLY, bool GEN>
__device__ __forceinline__ void act_bwd_kernel(const chap_act_bwd_params& Pk) {
    extern __shared__ float red[];            // reduce phase: [4 waves][2][C] partials
    // ---- the kernel arguments, once ----
    const chap_act_bwd_params P = chap_args_once(Pk);
    const act_plan S = act_make_plan<T>(P);
    const int C = P.r.C, C8 = C / 8, bn = P.bn;
    const long npix = (long)P.N * P.D * P.H * P.W;
    const chap_gptr scale = chap_global(P.r.scale), shift = chap_global(P.r.shift);
    const chap_gptr meanp = chap_global(P.mean), istdp = chap_global(P.invstd), gammap = chap_global(P.gamma);
    CHAP_GLOBAL float* const sums = (CHAP_GLOBAL float*)P.sums; CHAP_GLOBAL T* const gout = (CHAP_GLOBAL T*)P.gout;
    const float count = P.count;
    const int c8 = (threadIdx.x % C8) * 8;
    float s0[8], s1[8], istd[8], k0[8], sa[8], sb[8], cB[8], cC[8], cM[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; sa[j] = 1.f; sb[j] = 0.f; k0[j] = 1.f; istd[j] = 1.f; cB[j] = 0.f; cC[j] = 0.f; cM[j] = 0.f; }
    // (first of all: while these loads and divisions are in flight nothing else of the thread is in registers yet)
    if (APPLY && bn == 1) {                            // training-mode BatchNorm backward
        float mean[8], gm[8], a0[8], a1[8];
        ld8g(meanp + c8 * 4, mean); ld8g(istdp + c8 * 4, istd); ld8g(gammap + c8 * 4, gm);
        ld8g((chap_gptr)(sums + c8), a0); ld8g((chap_gptr)(sums + C + c8), a1);
        // g = k0*(dz - k1 - xhat*k2), xhat = raw*istd - mean*istd  ==  dz*k0 + raw*cB + cC  (two FMAs per element; actbwd_math.h)
        // one channel at a time: the scheduler interleaves all 16 divisions otherwise, and their temporaries are the kernel's register peak
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            actbwd_consts1(a0[j], a1[j], gm[j], mean[j], istd[j], count, k0[j], cB[j], cC[j]);
            __builtin_amdgcn_sched_barrier(0);                 // (the last one also keeps the loads below from being hoisted over this)
        }
    }
    const int prow = threadIdx.x / C8, PPB = 256 / C8;      // C8 in {1,2,4,...,32} divides 256: every thread has a pixel row
    const act_lane L = {c8 * (int)sizeof(T), c8, S.has_cm ? c8 * 4 : c8 * (int)sizeof(T)};
    long pix = (long)blockIdx.x * PPB + prow;
    const long step = (long)gridDim.x * PPB, last = npix - 1;
    // ---- the per-channel constants and the first trip ----
    // reduce: scale, shift, mean, invstd and the first trip together: one round trip (see cM below).  apply with bn == 1: mean, invstd, gamma and the 16 totals of the
    // thread's channels (straight from row 0, written by act_bwd_sum_kernel together with dgamma / dbeta: no copy through LDS, no barrier) become
    // k0, cB, cC first; scale, shift and the first trip follow together: two round trips -- all seven vectors and a trip in flight at once need
    // more registers than the phase may use.  apply without it: scale, shift and the first trip, one round trip.
    if (scale) { ld8g(scale + c8 * 4, sa); ld8g(shift + c8 * 4, sb); }
    // reduce forms cM BEHIND the first trip's requests and a scheduling barrier: in front of them its wait for mean and invstd stood between the
    // constants and the first trip (and the compiler then folded that request into the loop's: two round trips).  Except the general fp32 instance:
    // mean, invstd and its 53-register trip in flight together take 130 VGPRs, 3 waves per SIMD; cM first keeps it at 121 and at two round trips.
    constexpr bool CM_FIRST = GEN && sizeof(T) == 4;
    float mean[8];
    if (!APPLY) { ld8g(meanp + c8 * 4, mean); ld8g(istdp + c8 * 4, istd); }      // (the entry point checks bn != 0)
    if (!APPLY && CM_FIRST) {
#pragma unroll
        for (int j = 0; j < 8; ++j) cM[j] = -mean[j] * istd[j];      // xhat = raw*istd + cM
    }
    act_trip<T> cur;
    act_issue<T, GEN>(S, L, (u32)(pix < last ? pix : last), cur);
    if (!APPLY && !CM_FIRST) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; ++j) cM[j] = -mean[j] * istd[j];
    }
    if (APPLY && bn != 1 && scale) {                   // fixed affine (eval-mode BN): dz/draw = scale
#pragma unroll
        for (int j = 0; j < 8; ++j) k0[j] = sa[j];
    }
    for (; pix < npix; pix += step) {
        float raw[8], dz[8], gsum[8];
        act_gsum<T, GEN>(S, cur, gsum);
        act_bwd_dz<T, GEN>(S, cur, gsum, sa, sb, raw, dz);
        if (!APPLY) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 d = {dz[2 * j], dz[2 * j + 1]}, r2 = {raw[2 * j], raw[2 * j + 1]};
                const f32x2 i2 = {istd[2 * j], istd[2 * j + 1]}, m2 = {cM[2 * j], cM[2 * j + 1]};
                const f32x2 xh = r2 * i2 + m2;
                f32x2 a = {s0[2 * j], s0[2 * j + 1]}, b = {s1[2 * j], s1[2 * j + 1]};
                a = a + d; b = d * xh + b;
                s0[2 * j] = a.x; s0[2 * j + 1] = a.y; s1[2 * j] = b.x; s1[2 * j + 1] = b.y;
            }
        } else {
            float o[8];
            actbwd_apply8(dz, raw, k0, cB, cC, o);         // bn != 1: cB = cC = 0 -> dz*k0
            st8g(gout + pix * C + c8, o);
        }
        // the next trip as soon as this one is consumed, into the same registers; past the end the last pixel again (in bounds, never used: one
        // trip of cache-resident loads per thread.  A wave-uniform branch that skips it when no lane goes on costs 8 to 13 VGPRs in every
        // instance -- one-gradient apply 80 -> 88, general reduce fp32 121 -> 134, 3 waves per SIMD -- and was not kept).
        // (A second register set, requested one trip ahead, won 6 % stand-alone at 256^2 and nothing on the whole iteration: DESIGN.md section 5.)
        const long pn = pix + step < last ? pix + step : last;
        act_issue<T, GEN>(S, L, (u32)pn, cur);
    }
    if (!APPLY) {
        for (int i = threadIdx.x; i < 4 * 2 * C; i += 256) red[i] = 0.f;
        __syncthreads();
        // lanes l, l+C8, l+2*C8, ... of a wave hold the same 8 channels: shuffle-reduce them (fixed pairing), one row of
        // partials per wave in LDS, the four rows summed in a fixed order -> this block's partial row.  No atomics.
        const int wave = threadIdx.x >> 6;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = s0[j], b = s1[j];
            // inside a 16-lane row: DPP rotations (C8 is wave-uniform); across rows: two shuffles.  C8 == 1 (C = 8): all 16 lanes of a row hold the
            // same channels -- the whole row
            if (C8 == 1) { a = row16_sum(a); b = row16_sum(b); }
            else if (C8 == 2) { a = row16_stride_sum<2>(a); b = row16_stride_sum<2>(b); }
            else if (C8 == 4) { a = row16_stride_sum<4>(a); b = row16_stride_sum<4>(b); }
            else if (C8 == 8) { a = row16_stride_sum<8>(a); b = row16_stride_sum<8>(b); }
            for (int o = (C8 > 16 ? C8 : 16); o < 64; o <<= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
            if ((threadIdx.x & 63) < C8) { red[(wave * 2 + 0) * C + c8 + j] = a; red[(wave * 2 + 1) * C + c8 + j] = b; }
        }
        __syncthreads();
        CHAP_GLOBAL float* dst = sums + (long)(1 + blockIdx.x) * 2 * C;
        for (int i = threadIdx.x; i < 2 * C; i += 256) {
            const int which = i / C, c = i % C;
            dst[i] = (red[(0 * 2 + which) * C + c] + red[(1 * 2 + which) * C + c]) + (red[(2 * 2 + which) * C + c] + red[(3 * 2 + which) * C + c]);
        }
    }
}

// Fixed-order total of the per-block partial rows (one wave per value, fp64) into row 0, read by the apply phase;
// accumulates the BatchNorm parameter gradients.
struct act_bwd_sum_args { float* sums; int nblocks; float* dgamma; float* dbeta; int C; };
__device__ __forceinline__ void act_bwd_sum_kernel(const act_bwd_sum_args& Ak) {
    const act_bwd_sum_args A = chap_args_once(Ak);          // one scalar load and wait instead of three
    CHAP_GLOBAL float* const sums = (CHAP_GLOBAL float*)A.sums; const int nblocks = A.nblocks, C = A.C;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= 2 * C) return;
    // the parameter gradient this total is added to is requested NOW, next to the partial rows: behind the reduction it was one more
    // dependent memory round trip of a kernel that is nothing but latency
    CHAP_GLOBAL float* const acc = (CHAP_GLOBAL float*)(i < C ? A.dbeta : A.dgamma);
    const int ai = i < C ? i : i - C;
    float prior = 0.f;
    if (acc) prior = acc[ai];
    double t = 0.0;
    constexpr int NB = CHAP_ACT_BWD_SLOTS / 64;                  // all of a lane's loads in flight at once, adds in the fixed order
    float vv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int b = lane + 64 * k;
        vv[k] = sums[(long)(1 + (b < nblocks ? b : 0)) * 2 * C + i];
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) t += (lane + 64 * k < nblocks) ? (double)vv[k] : 0.0;
    t = wave_sum_f64(t);
    if (lane != 0) return;
    const float v = (float)t;
    sums[i] = v;
    if (acc) acc[ai] = prior + v;
}

static int act_bwd_check(const chap_act_bwd_params* p) {
    CHAP_CHECK_ARG(p && p->r.ptr, "chap_act_bwd: null argument");
    CHAP_CHECK_ARG(p->r.C % 8 == 0 && 256 % (p->r.C / 8) == 0 && p->r.C <= 1024, "chap_act_bwd: C=%d unsupported", p->r.C);
    CHAP_CHECK_ARG(p->ng >= 0 && p->ng <= 3, "chap_act_bwd: ng=%d", p->ng);
    {   // the kernels address every tensor with a 32-bit byte offset from its base
        long ld = p->r.ld > p->r.C ? p->r.ld : p->r.C;
        for (int k = 0; k < p->ng; ++k) ld = p->g_ld[k] > ld ? p->g_ld[k] : ld;
        const long bytes = (long)p->N * p->D * p->H * p->W * ld * (p->dtype == CHAP_BF16 ? 2 : 4);
        CHAP_CHECK_ARG(bytes < (1l << 32), "chap_act_bwd: a tensor of %ld bytes (4 GB at most)", bytes);
    }
    CHAP_CHECK_ARG(p->bn >= 0 && p->bn <= 2, "chap_act_bwd: bn=%d", p->bn);
    CHAP_CHECK_ARG(p->bn != 1 || (p->mean && p->invstd && p->gamma && p->sums), "chap_act_bwd: bn=1 needs mean/invstd/gamma/sums");
    CHAP_CHECK_ARG(!p->g_pool || (p->pool_idx && p->D == 1 && p->H % 2 == 0 && p->W % 2 == 0), "chap_act_bwd: pooled gradient needs idx and even 2D dims");
    return CHAP_OK;
}
// (Round 3 measured the totals folded into the apply phase -- every apply block re-reading the partial rows instead of the totals kernel:
// 2D 6.77 -> 6.95 ms, 3D 14.91 -> 15.04 ms per step, slower; removed in round 4, the record is in DESIGN.md section 5.)
static int act_bwd_blocks(const chap_act_bwd_params* p) {
    const long npix = (long)p->N * p->D * p->H * p->W;
    const int ppb = 256 / (p->r.C / 8);
    long b = (npix + ppb - 1) / ppb;
    // 2 blocks per CU, swept on the whole iteration (round 2, final tree: 256 / 384 / 512 / 640 / 768 / 1024 blocks -> 7.36 / 7.28 / 7.28 / 7.31 /
    // 7.38 / 7.41 ms per 2D step, 3D 16.80-16.87 for all): more blocks add partial rows to total and take CUs from the kernels of the
    // other streams
    long cap = chap_knob(KNOB_ACTBWD_BLOCKS);      // lab knob
    if (cap > CHAP_ACT_BWD_SLOTS) cap = 512;
    return (int)(b < cap ? b : cap);          // one partial row per block
}
// The instance of a layer: GEN = false for exactly one incoming gradient, no pooled gradient, no channel multipliers.
template <typename T, bool APPLY>
static int act_bwd_launch_t(const chap_act_bwd_params* p, int nb, size_t lds, hipStream_t s, const char* name) {
    if (p->ng == 1 && !p->g_pool && !p->r.chan_mul) return chap_launch<chap_act_bwd_params, act_bwd_kernel<T, APPLY, false>, 256>(dim3(nb), dim3(256), lds, s, *p, name);
    return chap_launch<chap_act_bwd_params, act_bwd_kernel<T, APPLY, true>, 256>(dim3(nb), dim3(256), lds, s, *p, name);
}
template <bool APPLY>
static int act_bwd_launch(const chap_act_bwd_params* p, int nb, size_t lds, hipStream_t s, const char* name) {
    return p->dtype == CHAP_BF16 ? act_bwd_launch_t<bf16_t, APPLY>(p, nb, lds, s, name) : act_bwd_launch_t<float, APPLY>(p, nb, lds, s, name);
}
extern "C" int chap_act_bwd_reduce(const chap_act_bwd_params* p, void* stream) {
    int r = act_bwd_check(p); if (r) return r;
    CHAP_CHECK_ARG(p->bn && p->mean && p->invstd && p->sums, "chap_act_bwd_reduce: needs bn, mean, invstd, sums");
    const size_t lds = 4 * 2 * p->r.C * sizeof(float);
    const int nb = act_bwd_blocks(p);              // one partial row per block
    r = act_bwd_launch<false>(p, nb, lds, (hipStream_t)stream, "chap_act_bwd_reduce");
    if (r) return r;
    if (chap_lab_skip(KNOB_LAB_SKIP_ACTSUM)) return CHAP_OK;      // lab builds only: timing bound, wrong numerics
    const act_bwd_sum_args sa = {p->sums, nb, p->dgamma, p->dbeta, p->r.C};
    return chap_launch<act_bwd_sum_args, act_bwd_sum_kernel, 256>(dim3(cdiv(2 * p->r.C, 4)), dim3(256), 0, (hipStream_t)stream, sa, "chap_act_bwd_reduce(sum)");
}
extern "C" int chap_act_bwd_apply(const chap_act_bwd_params* p, void* stream) {
    int r = act_bwd_check(p); if (r) return r;
    CHAP_CHECK_ARG(p->gout, "chap_act_bwd_apply: null gout");
    if (chap_lab_skip(KNOB_LAB_SKIP_ACTAPPLY) && p->bn == 1) return CHAP_OK;      // lab builds only: timing bound (wrong numerics) for folding this pass into the loads of its consumers
    return act_bwd_launch<true>(p, act_bwd_blocks(p), 0, (hipStream_t)stream, "chap_act_bwd_apply");      // (no LDS: the totals come straight from row 0)
}

// =========================================================================================
// Layout converters at the module boundary.
template <typename T>
__device__ __forceinline__ void planar_to_cl_kernel(const chap_planar_to_cl_params& P) {
    const int Cp = P.Cpad > P.C ? P.Cpad : P.C;       // channels [C, Cpad) are written as zeros
    const long total = (long)P.N * P.P * Cp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const u32 ui = (u32)i;
        const int c = (int)(ui % (u32)Cp); const u32 r = ui / (u32)Cp;
        const long pp = r % (u32)P.P; const int n = (int)(r / (u32)P.P);
        const float v = c < P.C ? P.in[((long)n * P.C + c) * P.P + pp] : 0.f;
        ((T*)P.out)[(n * (long)P.P + pp) * P.out_ld + P.out_coff + c] = elem<T>::put(v);
    }
}
// vector form: thread = (pixel, 8 channels), one 16-/32-byte store (the scalar form above writes 2 bytes per thread)
template <typename T>
__device__ __forceinline__ void planar_to_cl8_kernel(const chap_planar_to_cl_params& P) {
    const int Cp = P.Cpad > P.C ? P.Cpad : P.C, C8 = Cp / 8;
    const long total = (long)P.N * P.P * C8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const int c8 = (int)(ui % (u32)C8) * 8; const u32 r = ui / (u32)C8;
        const long pp = r % (u32)P.P; const int n = (int)(r / (u32)P.P);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c8 + j < P.C ? P.in[((long)n * P.C + c8 + j) * P.P + pp] : 0.f;
        st8((T*)P.out + (n * (long)P.P + pp) * P.out_ld + P.out_coff + c8, v);
    }
}
extern "C" int chap_planar_to_cl(const chap_planar_to_cl_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->in && p->out, "chap_planar_to_cl: null argument");
    const int Cp = p->Cpad > p->C ? p->Cpad : p->C;
    if (Cp % 8 == 0 && p->out_ld % 8 == 0 && p->out_coff % 8 == 0) {
        const long total = (long)p->N * p->P * (Cp / 8);
        const int blocks = chap_blocks(total, 16384);
        if (p->dtype == CHAP_BF16) return chap_launch<chap_planar_to_cl_params, planar_to_cl8_kernel<bf16_t>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_planar_to_cl");
        return chap_launch<chap_planar_to_cl_params, planar_to_cl8_kernel<float>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_planar_to_cl");
    }
    const long total = (long)p->N * p->P * Cp;
    const int blocks = chap_blocks(total, 4096);
    if (p->dtype == CHAP_BF16) return chap_launch<chap_planar_to_cl_params, planar_to_cl_kernel<bf16_t>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_planar_to_cl");
    return chap_launch<chap_planar_to_cl_params, planar_to_cl_kernel<float>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_planar_to_cl");
}

template <typename T>
__device__ __forceinline__ void cl_to_planar_kernel(const chap_cl_to_planar_params& P) {
    const int C = P.r.C;
    const long total = (long)P.N * P.P * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const u32 ui = (u32)i;
        const long pp = ui % (u32)P.P; const u32 r = ui / (u32)P.P;
        const int c = (int)(r % (u32)C); const int n = (int)(r / (u32)C);
        P.out[i] = src_load1<T>(P.r, n, (long)n * P.P + pp, c);
    }
}
extern "C" int chap_cl_to_planar(const chap_cl_to_planar_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->r.ptr && p->out, "chap_cl_to_planar: null argument");
    const long total = (long)p->N * p->P * p->r.C;
    const int blocks = chap_blocks(total, 4096);
    if (p->dtype == CHAP_BF16) return chap_launch<chap_cl_to_planar_params, cl_to_planar_kernel<bf16_t>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_cl_to_planar");
    return chap_launch<chap_cl_to_planar_params, cl_to_planar_kernel<float>, 256>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, "chap_cl_to_planar");
}

// =========================================================================================
// out[c] += sum over pixels of a (lazy) channel-last tensor: bias gradient of layers whose output
// gradient is not the B operand of chap_wgrad (transposed conv).
// A thread's channel group never changes: scale and shift once, in front of the loop; a trip's loads through src_issue / src_issue_cm, the
// next trip requested as soon as the current one is consumed (past the end: the last pixel again, in bounds, never used), as act_bwd_kernel.
template <typename T, bool KM, bool A32>
__device__ __forceinline__ void channel_sum_kernel(const chap_chansum_params& Pk) {
    typedef typename src_off<A32>::t OFF;
    extern __shared__ float red[];             // [4 waves][C]
    const chap_chansum_params P = chap_args_once(Pk);
    const src_plan S = src_make_plan<T>(P.r);
    const int C = P.r.C, C8 = C / 8;
    const int c8 = (threadIdx.x % C8) * 8, prow = threadIdx.x / C8, PPB = 256 / C8;
    const long npix = P.npix, last = npix > 0 ? npix - 1 : 0, step = (long)gridDim.x * PPB;
    const u32 pps = (u32)P.pix_per_sample;
    CHAP_GLOBAL float* const ws = (CHAP_GLOBAL float*)P.ws;
    const src_lane L = src_make_lane<T>(S, c8);
    float s[8], sa[8], sb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    src_load_aff(S, L, sa, sb);
    long pix = (long)blockIdx.x * PPB + prow;
    src_trip<T> cur; src_vec8 m;
    {
        const long pc = pix < last ? pix : last;
        src_issue_cm<KM, A32>(S, L, (int)((u32)pc / pps), (OFF)pc, m);
        src_issue<T, KM, A32>(S, L, (OFF)pc, cur);
    }
    for (; pix < npix; pix += step) {
        float v[8];
        src_finish<T, KM>(S, cur, m, sa, sb, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += v[j];
        const long pn = pix + step < last ? pix + step : last;
        src_issue_cm<KM, A32>(S, L, (int)((u32)pn / pps), (OFF)pn, m);
        src_issue<T, KM, A32>(S, L, (OFF)pn, cur);
    }
    for (int i = threadIdx.x; i < 4 * C; i += 256) red[i] = 0.f;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float a = s[j];
        for (int o = C8; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
        if ((threadIdx.x & 63) < C8) red[wave * C + c8 + j] = a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) ws[(long)blockIdx.x * C + i] = (red[i] + red[C + i]) + (red[2 * C + i] + red[3 * C + i]);
}
// out[c] += fixed-order total of the block partials (one wave per channel, fp64).  As act_bwd_sum_kernel: the arguments once, all of a lane's
// partial rows in flight at once, the prior out[c] requested next to them; the adds in the fixed ascending order.
struct chansum_final_args { const float* ws; int nblocks, C; float* out; };
__device__ __forceinline__ void channel_sum_final_kernel(const chansum_final_args& Ak) {
    const chansum_final_args A = chap_args_once(Ak);
    const CHAP_GLOBAL float* const ws = (const CHAP_GLOBAL float*)A.ws; CHAP_GLOBAL float* const out = (CHAP_GLOBAL float*)A.out;
    const int nblocks = A.nblocks, C = A.C;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    const float prior = out[c];
    constexpr int NB = CHAP_CHANSUM_SLOTS / 64;                  // (the entry point launches CHAP_CHANSUM_SLOTS blocks at most)
    float vv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int b = lane + 64 * k;
        vv[k] = ws[(long)(b < nblocks ? b : 0) * C + c];
    }
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) if (lane + 64 * k < nblocks) t += (double)vv[k];
    t = wave_sum_f64(t);
    if (lane == 0) out[c] = prior + (float)t;
}
template <typename T>
static int channel_sum_launch(const chap_chansum_params* p, bool a32, int nb, size_t lds, hipStream_t s) {
    const dim3 g(nb), b(256);
    if (!a32) return chap_launch<chap_chansum_params, channel_sum_kernel<T, true, false>, 256>(g, b, lds, s, *p, "chap_channel_sum");
    if (src_has_km(p->r)) return chap_launch<chap_chansum_params, channel_sum_kernel<T, true, true>, 256>(g, b, lds, s, *p, "chap_channel_sum");
    return chap_launch<chap_chansum_params, channel_sum_kernel<T, false, true>, 256>(g, b, lds, s, *p, "chap_channel_sum");
}
extern "C" int chap_channel_sum(const chap_chansum_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->r.ptr && p->out && p->ws && p->r.C % 8 == 0 && 256 % (p->r.C / 8) == 0 && p->r.C <= 512, "chap_channel_sum: bad argument");
    const int ppb = 256 / (p->r.C / 8);
    long b = (p->npix + ppb - 1) / ppb;
    const int nb = (int)(b < CHAP_CHANSUM_SLOTS ? b : CHAP_CHANSUM_SLOTS);
    const size_t lds = 4 * p->r.C * sizeof(float);
    const bool a32 = src_fits32(p->npix, p->r.ld > p->r.C ? p->r.ld : p->r.C, p->dtype);
    int r;
    if (p->dtype == CHAP_BF16) r = channel_sum_launch<bf16_t>(p, a32, nb, lds, (hipStream_t)stream);
    else r = channel_sum_launch<float>(p, a32, nb, lds, (hipStream_t)stream);
    if (r) return r;
    const chansum_final_args fa = {(const float*)p->ws, nb, p->r.C, p->out};
    return chap_launch<chansum_final_args, channel_sum_final_kernel, 256>(dim3(cdiv(p->r.C, 4)), dim3(256), 0, (hipStream_t)stream, fa, "chap_channel_sum(final)");
}
