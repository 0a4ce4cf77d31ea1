// The uncertainty-aware form of the mean teacher's consistency term (include/chap_hip_uncertainty.h).  Two streaming kernels with
// teacher_consistency_kernel's structure (teacher.hip): the first turns the 2T logit tensors of T noisy teacher passes into the entropy of
// their mean softmax, the mask "entropy under the threshold" and its exact count; the second is the softmax-MSE term counted over the masked
// pixels only.  Both HBM-bound: 2T N C P floats read and N P bytes written; 4 N C P floats + N P bytes read, 2 N C P read-modify-written
// where the mask is set.  Per-block partials and a one-block fixed-order finalize each (integers for the count, fp64 for the loss): no atomics.
#include "common.h"
#include "chap_hip_uncertainty.h"

namespace {

constexpr int UC_MINC = 2, UC_MAXC = 8;

__device__ __forceinline__ double wave_sum_f64(double v) {      // xor butterfly: the same pairing on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// softmax of one pixel's C values, in place (max-subtracted, expf: the training kernels' form)
template <int C>
__device__ __forceinline__ void softmax_inplace(float z[C]) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { z[c] = expf(z[c] - m); s += z[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] *= inv;
}

// the sum of the 2T softmax outputs of one pixel -> its entropy H = -sum_c pbar_c logf(pbar_c + 1e-6), pbar = sum * 1 / (2T)
template <int C>
__device__ __forceinline__ float entropy_px(const float sum[C], float inv2t) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { const float pb = sum[c] * inv2t; s += pb * logf(pb + 1e-6f); }
    return -s;
}

// the paths' common decision, from the same values on host and device
__host__ __device__ inline bool uncertainty_quads(const chap_teacher_uncertainty_params& p) {
    uintptr_t a = (uintptr_t)p.entropy;
    for (int k = 0; k < p.T; ++k) a |= (uintptr_t)p.teacher[k][0] | (uintptr_t)p.teacher[k][1];
    return (p.P & 3) == 0 && (a & 15) == 0 && ((uintptr_t)p.mask & 3) == 0;
}

__host__ __device__ inline bool masked_quads(const chap_teacher_consistency_masked_params& p) {
    return (p.P & 3) == 0 && (((uintptr_t)p.logits[0] | (uintptr_t)p.logits[1] | (uintptr_t)p.teacher[0] | (uintptr_t)p.teacher[1] |
                               (uintptr_t)p.dlogits[0] | (uintptr_t)p.dlogits[1]) & 15) == 0 && ((uintptr_t)p.mask & 3) == 0;
}

// ws rows: [1 + CHAP_LOSS_SLOTS] int64; block b leaves the number of pixels it found certain in row 1 + b.
template <int C>
__global__ __launch_bounds__(256) void teacher_uncertainty_kernel(const chap_teacher_uncertainty_params P_) {
    __shared__ int red[4];
    const long P = P_.P, total = (long)P_.N * P;
    const int T = P_.T;
    const float thr = P_.threshold_dev ? *P_.threshold_dev : P_.threshold;
    const float inv2t = 1.f / (float)(2 * T);
    int cnt = 0;
    if (uncertainty_quads(P_)) {
        // four consecutive pixels per thread, 16-byte loads of every class plane: the running sum [C][4] and one head's [C][4] are live
        const long totalq = total >> 2;
        for (long qi = (long)blockIdx.x * 256 + threadIdx.x; qi < totalq; qi += (long)gridDim.x * 256) {
            const long i = qi << 2;
            const long n = (unsigned)i / (unsigned)P, pp = (unsigned)i % (unsigned)P, base = n * C * P + pp;
            float sum[C][4];
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c][0] = sum[c][1] = sum[c][2] = sum[c][3] = 0.f;
            for (int k = 0; k < T; ++k) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float* src = P_.teacher[k][h] + base;
                    float z[C][4];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float4 a = *(const float4*)(src + c * P);
                        z[c][0] = a.x; z[c][1] = a.y; z[c][2] = a.z; z[c][3] = a.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float u[C];
#pragma unroll
                        for (int c = 0; c < C; ++c) u[c] = z[c][e];
                        softmax_inplace<C>(u);
#pragma unroll
                        for (int c = 0; c < C; ++c) sum[c][e] += u[c];
                    }
                }
            }
            float H[4];
            unsigned mw = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float u[C];
#pragma unroll
                for (int c = 0; c < C; ++c) u[c] = sum[c][e];
                H[e] = entropy_px<C>(u, inv2t);
                const unsigned m = H[e] < thr ? 1u : 0u;
                mw |= m << (8 * e);
                cnt += (int)m;
            }
            *(unsigned*)(P_.mask + i) = mw;
            if (P_.entropy) *(float4*)(P_.entropy + i) = make_float4(H[0], H[1], H[2], H[3]);
        }
    } else
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = (unsigned)i / (unsigned)P, pp = (unsigned)i % (unsigned)P, base = n * C * P + pp;
        float sum[C];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = 0.f;
        for (int k = 0; k < T; ++k) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float* src = P_.teacher[k][h] + base;
                float u[C];
#pragma unroll
                for (int c = 0; c < C; ++c) u[c] = src[c * P];
                softmax_inplace<C>(u);
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += u[c];
            }
        }
        const float H = entropy_px<C>(sum, inv2t);
        const int m = H < thr ? 1 : 0;
        P_.mask[i] = (uint8_t)m;
        if (P_.entropy) P_.entropy[i] = H;
        cnt += m;
    }
    cnt = wave_sum_i32(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) P_.ws[1 + blockIdx.x] = (int64_t)red[0] + red[1] + red[2] + red[3];
}

// row 0 and *count <- the sum of rows 1..nblocks (integers: exact, whatever the order)
__global__ __launch_bounds__(64) void teacher_uncertainty_final_kernel(int64_t* ws, int nblocks, int64_t* count) {
    long long t = 0;
    for (int b = threadIdx.x; b < nblocks; b += 64) t += ws[1 + b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (threadIdx.x == 0) { ws[0] = t; *count = t; }
}

// p (softmax of a student head) and q -> the pixel's sum of e^2 is returned, p is overwritten with gs * p * (e - sum_c p_c e_c)
template <int C>
__device__ __forceinline__ float mse_grad_px(float p[C], const float q[C], float gs) {
    float e[C], sq = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { e[c] = p[c] - q[c]; sq += e[c] * e[c]; dot += p[c] * e[c]; }
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = gs * p[c] * (e[c] - dot);
    return sq;
}

__device__ __forceinline__ float masked_den(const chap_teacher_consistency_masked_params& p) { return (float)p.C * (float)*p.count + 1e-16f; }

// ws rows: [1 + CHAP_LOSS_SLOTS][2 heads]; block b leaves its partial sums of m e^2 in row 1 + b.  A pixel with m = 0 is never loaded: it
// adds nothing to the sums, and its gradient is not touched (`accumulate`) or written as +0.
template <int C>
__global__ __launch_bounds__(256) void teacher_consistency_masked_kernel(const chap_teacher_consistency_masked_params P_) {
    __shared__ float red[4][2];
    const long P = P_.P, total = (long)P_.N * P;
    const float gs = P_.gscale * (P_.gscale_dev ? *P_.gscale_dev : 1.f) * (2.f / masked_den(P_));
    const bool acc_grad = P_.accumulate != 0;
    float acc[2] = {0.f, 0.f};
    if (masked_quads(P_)) {
        const long totalq = total >> 2;
        for (long qi = (long)blockIdx.x * 256 + threadIdx.x; qi < totalq; qi += (long)gridDim.x * 256) {
            const long i = qi << 2;
            const long n = (unsigned)i / (unsigned)P, pp = (unsigned)i % (unsigned)P, base = n * C * P + pp;
            const unsigned mw = *(const unsigned*)(P_.mask + i);
            if (mw == 0) {                      // the whole quad is uncertain
                if (!acc_grad) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (P_.dlogits[h]) {
#pragma unroll
                            for (int c = 0; c < C; ++c) *(float4*)(P_.dlogits[h] + base + c * P) = make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                }
                continue;
            }
            bool on[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) on[e] = ((mw >> (8 * e)) & 0xffu) != 0;
            float q[C][4];
            {
                float t[C][4];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float4 a = *(const float4*)(P_.teacher[0] + base + c * P), b = *(const float4*)(P_.teacher[1] + base + c * P);
                    q[c][0] = a.x; q[c][1] = a.y; q[c][2] = a.z; q[c][3] = a.w; t[c][0] = b.x; t[c][1] = b.y; t[c][2] = b.z; t[c][3] = b.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float u[C], v[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) { u[c] = q[c][e]; v[c] = t[c][e]; }
                    softmax_inplace<C>(u);
                    softmax_inplace<C>(v);
#pragma unroll
                    for (int c = 0; c < C; ++c) q[c][e] = 0.5f * (u[c] + v[c]);
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float z[C][4];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float4 a = *(const float4*)(P_.logits[h] + base + c * P);
                    z[c][0] = a.x; z[c][1] = a.y; z[c][2] = a.z; z[c][3] = a.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float p[C], qq[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) { p[c] = z[c][e]; qq[c] = q[c][e]; }
                    softmax_inplace<C>(p);
                    const float sq = mse_grad_px<C>(p, qq, gs);
                    if (on[e]) acc[h] += sq;
#pragma unroll
                    for (int c = 0; c < C; ++c) z[c][e] = p[c];
                }
                if (P_.dlogits[h]) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        float4* d = (float4*)(P_.dlogits[h] + base + c * P);
                        float4 g;
                        if (acc_grad) {
                            const float4 o = *d;
                            g.x = on[0] ? o.x + z[c][0] : o.x; g.y = on[1] ? o.y + z[c][1] : o.y;
                            g.z = on[2] ? o.z + z[c][2] : o.z; g.w = on[3] ? o.w + z[c][3] : o.w;
                        } else
                            g = make_float4(on[0] ? z[c][0] : 0.f, on[1] ? z[c][1] : 0.f, on[2] ? z[c][2] : 0.f, on[3] ? z[c][3] : 0.f);
                        *d = g;
                    }
                }
            }
        }
    } else
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = (unsigned)i / (unsigned)P, pp = (unsigned)i % (unsigned)P, base = n * C * P + pp;
        if (P_.mask[i] == 0) {
            if (!acc_grad) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (P_.dlogits[h]) {
#pragma unroll
                        for (int c = 0; c < C; ++c) P_.dlogits[h][base + c * P] = 0.f;
                    }
            }
            continue;
        }
        float q[C], t[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { q[c] = P_.teacher[0][base + c * P]; t[c] = P_.teacher[1][base + c * P]; }
        softmax_inplace<C>(q);
        softmax_inplace<C>(t);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = 0.5f * (q[c] + t[c]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float p[C];
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = P_.logits[h][base + c * P];
            softmax_inplace<C>(p);
            acc[h] += mse_grad_px<C>(p, q, gs);
            if (P_.dlogits[h]) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float* d = P_.dlogits[h] + base + c * P;
                    *d = acc_grad ? *d + p[c] : p[c];
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float v = wave_sum(acc[h]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][h] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) P_.ws[(long)(1 + blockIdx.x) * 2 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// row 0 <- the fixed-order fp64 column sums of rows 1..nblocks (wave h: head h); loss = (sum of both) / den
__global__ __launch_bounds__(256) void teacher_consistency_masked_final_kernel(float* ws, int nblocks, int C, const int64_t* count, float* loss) {
    __shared__ float tot[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2) {
        double t = 0.0;
        for (int b = lane; b < nblocks; b += 64) t += (double)ws[(long)(1 + b) * 2 + wave];
        t = wave_sum_f64(t);
        if (lane == 0) { tot[wave] = (float)t; ws[wave] = (float)t; }
    }
    __syncthreads();
    if (threadIdx.x == 0) *loss = (tot[0] + tot[1]) / ((float)C * (float)*count + 1e-16f);
}

int grid_for(long units) {
    const long blocks = (units + 255) / 256;
    return (int)(blocks < CHAP_LOSS_SLOTS ? blocks : CHAP_LOSS_SLOTS);
}

}  // namespace

#define UC_CASE(C_) case C_: hipLaunchKernelGGL(teacher_uncertainty_kernel<C_>, dim3(nb), dim3(256), 0, s, *p); break;
#define MC_CASE(C_) case C_: hipLaunchKernelGGL(teacher_consistency_masked_kernel<C_>, dim3(nb), dim3(256), 0, s, *p); break;

extern "C" int chap_teacher_uncertainty(const chap_teacher_uncertainty_params* p, void* stream) {
    CHAP_CHECK_ARG(p, "chap_teacher_uncertainty: null argument");
    CHAP_CHECK_ARG(p->T >= 1 && p->T <= CHAP_UNCERTAINTY_MAX_T, "chap_teacher_uncertainty: T=%d (1..%d built)", p->T, CHAP_UNCERTAINTY_MAX_T);
    CHAP_CHECK_ARG(p->C >= UC_MINC && p->C <= UC_MAXC, "chap_teacher_uncertainty: C=%d (2..8 built)", p->C);
    CHAP_CHECK_ARG(p->N > 0 && p->P > 0, "chap_teacher_uncertainty: N=%d, P=%d", p->N, p->P);
    const long total = (long)p->N * p->P;
    CHAP_CHECK_ARG(total < (1L << 32), "chap_teacher_uncertainty: N*P=%ld exceeds the 32-bit pixel index", total);
    uintptr_t a = 0;
    for (int k = 0; k < p->T; ++k) {
        CHAP_CHECK_ARG(p->teacher[k][0] && p->teacher[k][1], "chap_teacher_uncertainty: null teacher logits in pass %d of T=%d", k, p->T);
        a |= (uintptr_t)p->teacher[k][0] | (uintptr_t)p->teacher[k][1];
    }
    CHAP_CHECK_ARG(p->mask && p->count && p->ws, "chap_teacher_uncertainty: null mask, count or ws");
    CHAP_CHECK_ARG(((a | (uintptr_t)p->entropy | (uintptr_t)p->threshold_dev) & 3) == 0, "chap_teacher_uncertainty: float pointers must be 4-byte aligned");
    CHAP_CHECK_ARG((((uintptr_t)p->count | (uintptr_t)p->ws) & 7) == 0, "chap_teacher_uncertainty: count and ws must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the grid the kernel's path needs, capped so the partial rows suffice (the kernel takes the same decision from the same values)
    const int nb = grid_for(uncertainty_quads(*p) ? total >> 2 : total);
    switch (p->C) { UC_CASE(2) UC_CASE(3) UC_CASE(4) UC_CASE(5) UC_CASE(6) UC_CASE(7) UC_CASE(8) default: break; }
    CHAP_LAUNCH_CHECK("chap_teacher_uncertainty");
    hipLaunchKernelGGL(teacher_uncertainty_final_kernel, dim3(1), dim3(64), 0, s, p->ws, nb, p->count);
    CHAP_LAUNCH_CHECK("chap_teacher_uncertainty(final)");
    return CHAP_OK;
}

extern "C" int chap_teacher_consistency_masked(const chap_teacher_consistency_masked_params* p, void* stream) {
    CHAP_CHECK_ARG(p, "chap_teacher_consistency_masked: null argument");
    CHAP_CHECK_ARG(p->logits[0] && p->logits[1] && p->teacher[0] && p->teacher[1] && p->mask && p->count && p->loss && p->ws,
                   "chap_teacher_consistency_masked: null logits, teacher, mask, count, loss or ws");
    CHAP_CHECK_ARG(p->C >= UC_MINC && p->C <= UC_MAXC, "chap_teacher_consistency_masked: C=%d (2..8 built)", p->C);
    CHAP_CHECK_ARG(p->N > 0 && p->P > 0, "chap_teacher_consistency_masked: N=%d, P=%d", p->N, p->P);
    const long total = (long)p->N * p->P;
    CHAP_CHECK_ARG(total < (1L << 32), "chap_teacher_consistency_masked: N*P=%ld exceeds the 32-bit pixel index", total);
    CHAP_CHECK_ARG((((uintptr_t)p->logits[0] | (uintptr_t)p->logits[1] | (uintptr_t)p->teacher[0] | (uintptr_t)p->teacher[1] | (uintptr_t)p->dlogits[0] |
                     (uintptr_t)p->dlogits[1] | (uintptr_t)p->loss | (uintptr_t)p->ws | (uintptr_t)p->gscale_dev) & 3) == 0,
                   "chap_teacher_consistency_masked: float pointers must be 4-byte aligned");
    CHAP_CHECK_ARG(((uintptr_t)p->count & 7) == 0, "chap_teacher_consistency_masked: count must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nb = grid_for(masked_quads(*p) ? total >> 2 : total);
    switch (p->C) { MC_CASE(2) MC_CASE(3) MC_CASE(4) MC_CASE(5) MC_CASE(6) MC_CASE(7) MC_CASE(8) default: break; }
    CHAP_LAUNCH_CHECK("chap_teacher_consistency_masked");
    hipLaunchKernelGGL(teacher_consistency_masked_final_kernel, dim3(1), dim3(256), 0, s, p->ws, nb, p->C, p->count, p->loss);
    CHAP_LAUNCH_CHECK("chap_teacher_consistency_masked(final)");
    return CHAP_OK;
}
