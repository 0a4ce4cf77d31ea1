// Residual V-Net block (ResidualConvBlock, vnet.py:37-67): the add + ReLU behind a block's last Conv3d -> BatchNorm, its backward, and
// the fold of more than three gradient contributions.  Streaming, HBM-bound: one lane = 8 channels of one voxel (16-byte accesses for
// bf16, two for fp32), grid-stride, fp32 arithmetic, plain stores, no LDS, no atomics.  Launched through launch.h's trampoline: the
// two decoders' blocks are the lanes of one grouped launch.
#include "common.h"
#include "launch.h"

typedef unsigned int u32;      // 32-bit index decoding (pointwise.hip): the entry points reject >= 2^32 lanes

// out = max(0, (scale * r + shift) + t), t = the block input summed first: a(src0) [+ a(src1)], or the one-channel image
template <typename T>
__device__ __forceinline__ void residual_fwd_kernel(const chap_residual_params& P) {
    const int C = P.r.C, C8 = C / 8;
    const u32 pps = (u32)P.D * (u32)P.H * (u32)P.W;
    const long total = (long)P.N * pps * C8;
    const bool need_n = P.r.chan_mul != nullptr || (P.nsrc > 0 && P.src[0].chan_mul != nullptr) || (P.nsrc > 1 && P.src[1].chan_mul != nullptr);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const u32 upix = ui / (u32)C8;
        const int c8 = (int)(ui - upix * (u32)C8) * 8;
        const long pix = (long)upix;
        const int n = need_n ? (int)(upix / pps) : 0;      // wave-uniform: only a Dropout3d multiplier needs the sample
        float v[8], t[8];
        src_load8<T>(P.r, n, pix, c8, v);
        if (P.nsrc > 0) {
            src_load8<T>(P.src[0], n, pix, c8, t);
            if (P.nsrc > 1) {
                float u[8];
                src_load8<T>(P.src[1], n, pix, c8, u);
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] += u[j];
            }
        } else {
            const float xv = P.xin[pix];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = xv;
        }
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float s = v[j] + t[j]; o[j] = s <= 0.f ? 0.f : s; }      // (a NaN stays a NaN, as torch's ReLU keeps it)
        st8((T*)P.out + pix * C + c8, o);
    }
}

static int residual_src_check(const chap_src_t& s, int C, const char* what) {
    CHAP_CHECK_ARG(s.ptr != nullptr, "chap_residual_fwd: %s: null tensor", what);
    CHAP_CHECK_ARG(s.C == C, "chap_residual_fwd: %s: C=%d, the block has %d channels", what, s.C, C);
    CHAP_CHECK_ARG(s.ld >= s.coff + s.C && s.ld % 8 == 0 && s.coff % 8 == 0 && s.coff >= 0, "chap_residual_fwd: %s: ld=%d coff=%d C=%d not 8-aligned / too small", what, s.ld, s.coff, s.C);
    CHAP_CHECK_ARG((s.scale == nullptr) == (s.shift == nullptr), "chap_residual_fwd: %s: scale and shift must come together", what);
    return CHAP_OK;
}

// lanes of a launch: voxels * C / 8, which must fit the kernels' 32-bit index
static int residual_lanes(const char* who, int N, int D, int H, int W, int C, long* lanes) {
    CHAP_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, "%s: empty grid N=%d D=%d H=%d W=%d", who, N, D, H, W);
    CHAP_CHECK_ARG(C > 0 && C % 8 == 0, "%s: C=%d must be a positive multiple of 8", who, C);
    const long npix = (long)N * D * H * W;
    CHAP_CHECK_ARG(npix < (1L << 31) && npix * (C / 8) < (1L << 32), "%s: %ld voxels x %d channels exceed the 32-bit voxel index", who, npix, C);
    *lanes = npix * (C / 8);
    return CHAP_OK;
}

extern "C" int chap_residual_fwd(const chap_residual_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->r.ptr && p->out, "chap_residual_fwd: null argument");
    CHAP_CHECK_ARG(p->dtype == CHAP_F32 || p->dtype == CHAP_BF16, "chap_residual_fwd: dtype=%d", p->dtype);
    long lanes = 0;
    int r = residual_lanes("chap_residual_fwd", p->N, p->D, p->H, p->W, p->r.C, &lanes); if (r) return r;
    CHAP_CHECK_ARG(p->r.act == 0, "chap_residual_fwd: r.act=%d (the block's last stage has no activation: must be 0)", p->r.act);
    r = residual_src_check(p->r, p->r.C, "r"); if (r) return r;
    CHAP_CHECK_ARG(p->nsrc >= 0 && p->nsrc <= 2, "chap_residual_fwd: nsrc=%d (0..2)", p->nsrc);
    CHAP_CHECK_ARG((p->nsrc > 0) != (p->xin != nullptr), "chap_residual_fwd: exactly one of nsrc > 0 and xin (nsrc=%d, xin %s)", p->nsrc, p->xin ? "given" : "NULL");
    for (int k = 0; k < p->nsrc; ++k) { r = residual_src_check(p->src[k], p->r.C, k ? "src[1]" : "src[0]"); if (r) return r; }
    const int nb = chap_blocks(lanes, 2048);
    hipStream_t s = (hipStream_t)stream;
    if (p->dtype == CHAP_BF16) return chap_launch<chap_residual_params, residual_fwd_kernel<bf16_t>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_residual_fwd");
    return chap_launch<chap_residual_params, residual_fwd_kernel<float>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_residual_fwd");
}

// gout = ((g0 + g1) + g2) * chan_mul * [out > 0];  DXIN: dxin[voxel] = sum_c of the unrounded value -- a lane's 8 channels in ascending
// order, then an xor butterfly over the C/8 lanes of the voxel (consecutive lanes of one wave: C/8 is a power of two dividing 64, and
// 256 % (C/8) == 0 keeps a voxel's lanes together in every grid-stride trip).  Every lane of a wave runs every trip of the DXIN loop
// (the shuffles need the partner lanes); lanes past the end compute on voxel 0 and store nothing.
template <typename T, bool DXIN>
__device__ __forceinline__ void residual_bwd_kernel(const chap_residual_bwd_params& P) {
    const int C = P.C, C8 = C / 8;
    const u32 pps = (u32)P.D * (u32)P.H * (u32)P.W;
    const long total = (long)P.N * pps * C8;
    for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {
        const long i = base + threadIdx.x;
        const bool live = i < total;
        if (!DXIN && !live) break;
        const u32 ui = live ? (u32)i : 0u;
        const u32 upix = ui / (u32)C8;
        const int c8 = (int)(ui - upix * (u32)C8) * 8;
        const long pix = (long)upix;
        float gs[8], o[8];
        ld8((const T*)P.g[0] + pix * P.g_ld[0] + P.g_coff[0] + c8, gs);
        for (int k = 1; k < P.ng; ++k) {
            float v[8];
            ld8((const T*)P.g[k] + pix * P.g_ld[k] + P.g_coff[k] + c8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) gs[j] += v[j];
        }
        ld8((const T*)P.out + pix * C + c8, o);
        if (P.chan_mul) {
            float cm[8];
            ld8(P.chan_mul + (long)(upix / pps) * C + c8, cm);
#pragma unroll
            for (int j = 0; j < 8; ++j) gs[j] *= cm[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) gs[j] = o[j] > 0.f ? gs[j] : 0.f;
        if (live) st8((T*)P.gout + pix * C + c8, gs);
        if (DXIN) {
            float s = gs[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) s += gs[j];
            for (int m = 1; m < C8; m <<= 1) s += __shfl_xor(s, m, 64);
            if (live && c8 == 0) P.dxin[pix] = s;
        }
    }
}

extern "C" int chap_residual_bwd(const chap_residual_bwd_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->out && p->gout, "chap_residual_bwd: null argument");
    CHAP_CHECK_ARG(p->dtype == CHAP_F32 || p->dtype == CHAP_BF16, "chap_residual_bwd: dtype=%d", p->dtype);
    long lanes = 0;
    int r = residual_lanes("chap_residual_bwd", p->N, p->D, p->H, p->W, p->C, &lanes); if (r) return r;
    CHAP_CHECK_ARG(p->ng >= 1 && p->ng <= 3, "chap_residual_bwd: ng=%d (1..3)", p->ng);
    for (int k = 0; k < p->ng; ++k) {
        CHAP_CHECK_ARG(p->g[k] != nullptr, "chap_residual_bwd: g[%d] is null", k);
        CHAP_CHECK_ARG(p->g_coff[k] >= 0 && p->g_ld[k] >= p->g_coff[k] + p->C && p->g_ld[k] % 8 == 0 && p->g_coff[k] % 8 == 0,
                       "chap_residual_bwd: g[%d]: ld=%d coff=%d C=%d not 8-aligned / too small", k, p->g_ld[k], p->g_coff[k], p->C);
    }
    const int c8 = p->C / 8;
    if (p->dxin) CHAP_CHECK_ARG(c8 <= 64 && (c8 & (c8 - 1)) == 0, "chap_residual_bwd: dxin needs C/8 a power of two <= 64 (C=%d)", p->C);
    const int nb = chap_blocks(lanes, 2048);
    hipStream_t s = (hipStream_t)stream;
    const bool bf = p->dtype == CHAP_BF16;
    if (p->dxin) {
        if (bf) return chap_launch<chap_residual_bwd_params, residual_bwd_kernel<bf16_t, true>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_residual_bwd(dxin)");
        return chap_launch<chap_residual_bwd_params, residual_bwd_kernel<float, true>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_residual_bwd(dxin)");
    }
    if (bf) return chap_launch<chap_residual_bwd_params, residual_bwd_kernel<bf16_t, false>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_residual_bwd");
    return chap_launch<chap_residual_bwd_params, residual_bwd_kernel<float, false>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_residual_bwd");
}

// out = ((g0 + g1) + g2) + g3
template <typename T>
__device__ __forceinline__ void grad_sum_kernel(const chap_grad_sum_params& P) {
    const int C = P.C, C8 = C / 8;
    const long total = (long)P.npix * C8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const u32 ui = (u32)i;
        const u32 upix = ui / (u32)C8;
        const int c8 = (int)(ui - upix * (u32)C8) * 8;
        const long pix = (long)upix;
        float a[8];
        ld8((const T*)P.g[0] + pix * P.g_ld[0] + P.g_coff[0] + c8, a);
        for (int k = 1; k < P.ng; ++k) {
            float v[8];
            ld8((const T*)P.g[k] + pix * P.g_ld[k] + P.g_coff[k] + c8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] += v[j];
        }
        st8((T*)P.out + pix * C + c8, a);
    }
}

extern "C" int chap_grad_sum(const chap_grad_sum_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->out, "chap_grad_sum: null argument");
    CHAP_CHECK_ARG(p->dtype == CHAP_F32 || p->dtype == CHAP_BF16, "chap_grad_sum: dtype=%d", p->dtype);
    CHAP_CHECK_ARG(p->C > 0 && p->C % 8 == 0, "chap_grad_sum: C=%d must be a positive multiple of 8", p->C);
    CHAP_CHECK_ARG(p->npix > 0 && p->npix < (1L << 31) && p->npix * (p->C / 8) < (1L << 32), "chap_grad_sum: %ld pixels x %d channels exceed the 32-bit pixel index",
                   (long)p->npix, p->C);
    CHAP_CHECK_ARG(p->ng >= 2 && p->ng <= 4, "chap_grad_sum: ng=%d (2..4)", p->ng);
    for (int k = 0; k < p->ng; ++k) {
        CHAP_CHECK_ARG(p->g[k] != nullptr, "chap_grad_sum: g[%d] is null", k);
        CHAP_CHECK_ARG(p->g_coff[k] >= 0 && p->g_ld[k] >= p->g_coff[k] + p->C && p->g_ld[k] % 8 == 0 && p->g_coff[k] % 8 == 0,
                       "chap_grad_sum: g[%d]: ld=%d coff=%d C=%d not 8-aligned / too small", k, p->g_ld[k], p->g_coff[k], p->C);
    }
    const int nb = chap_blocks(p->npix * (p->C / 8), 2048);
    hipStream_t s = (hipStream_t)stream;
    if (p->dtype == CHAP_BF16) return chap_launch<chap_grad_sum_params, grad_sum_kernel<bf16_t>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_grad_sum");
    return chap_launch<chap_grad_sum_params, grad_sum_kernel<float>, 256>(dim3(nb), dim3(256), 0, s, *p, "chap_grad_sum");
}
