// The mean teacher's consistency term (include/chap_hip_teacher.h): softmax-MSE between each student head and the ensemble of the teacher's
// two heads, loss and gradient in ONE streaming kernel with kl_kernel's structure (loss.hip) -- the gradient is local to the pixel -- and a
// one-block fixed-order fp64 finalize.  HBM-bound: 4 N C P floats read, 2 N C P written (and read, when it accumulates).  No atomics.
#include "common.h"
#include "chap_hip_teacher.h"

namespace {

constexpr int TC_MINC = 2, TC_MAXC = 8;

__device__ __forceinline__ double wave_sum_f64(double v) {      // xor butterfly: the same pairing on every run
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

// ws rows: [1 + CHAP_LOSS_SLOTS][2 heads]; block b leaves its partial sums of e^2 in row 1 + b.
template <int C>
__global__ __launch_bounds__(256) void teacher_consistency_kernel(const chap_teacher_consistency_params P_) {
    __shared__ float red[4][2];
    const long P = P_.P, total = (long)P_.N * P;
    const float gs = P_.gscale * (P_.gscale_dev ? *P_.gscale_dev : 1.f) * (2.f / ((float)total * (float)C));
    const bool acc_grad = P_.accumulate != 0;
    float acc[2] = {0.f, 0.f};
    const bool quads = (P & 3) == 0 && (((uintptr_t)P_.logits[0] | (uintptr_t)P_.logits[1] | (uintptr_t)P_.teacher[0] | (uintptr_t)P_.teacher[1] |
                                         (uintptr_t)P_.dlogits[0] | (uintptr_t)P_.dlogits[1]) & 15) == 0;
    if (quads) {
        // four consecutive pixels per thread, 16-byte loads / stores of every class plane (as kl_kernel).  q[C][4] first, then one student
        // head at a time: q, one head's values and the prior gradient are about 100 live floats at C = 8
        const long totalq = total >> 2;
        for (long qi = (long)blockIdx.x * 256 + threadIdx.x; qi < totalq; qi += (long)gridDim.x * 256) {
            const long i = qi << 2;
            const long n = (unsigned)i / (unsigned)P, pp = (unsigned)i % (unsigned)P, base = n * C * P + pp;
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
                    acc[h] += mse_grad_px<C>(p, qq, gs);
#pragma unroll
                    for (int c = 0; c < C; ++c) z[c][e] = p[c];
                }
                if (P_.dlogits[h]) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        float4* d = (float4*)(P_.dlogits[h] + base + c * P);
                        float4 g = make_float4(z[c][0], z[c][1], z[c][2], z[c][3]);
                        if (acc_grad) { const float4 o = *d; g.x += o.x; g.y += o.y; g.z += o.z; g.w += o.w; }
                        *d = g;
                    }
                }
            }
        }
    } else
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = (unsigned)i / (unsigned)P, pp = (unsigned)i % (unsigned)P, base = n * C * P + pp;
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

// row 0 <- the fixed-order fp64 column sums of rows 1..nblocks (wave h: head h); loss = (sum of both) / (N C P)
__global__ __launch_bounds__(256) void teacher_consistency_final_kernel(float* ws, int nblocks, float inv_count, float* loss) {
    __shared__ float tot[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2) {
        double t = 0.0;
        for (int b = lane; b < nblocks; b += 64) t += (double)ws[(long)(1 + b) * 2 + wave];
        t = wave_sum_f64(t);
        if (lane == 0) { tot[wave] = (float)t; ws[wave] = (float)t; }
    }
    __syncthreads();
    if (threadIdx.x == 0) *loss = (tot[0] + tot[1]) * inv_count;
}

}  // namespace

#define TC_CASE(C_) case C_: hipLaunchKernelGGL(teacher_consistency_kernel<C_>, dim3(nb), dim3(256), 0, s, *p); break;

extern "C" int chap_teacher_consistency(const chap_teacher_consistency_params* p, void* stream) {
    CHAP_CHECK_ARG(p, "chap_teacher_consistency: null argument");
    CHAP_CHECK_ARG(p->logits[0] && p->logits[1] && p->teacher[0] && p->teacher[1] && p->loss && p->ws, "chap_teacher_consistency: null logits, teacher, loss or ws");
    CHAP_CHECK_ARG(p->C >= TC_MINC && p->C <= TC_MAXC, "chap_teacher_consistency: C=%d (2..8 built)", p->C);
    CHAP_CHECK_ARG(p->N > 0 && p->P > 0, "chap_teacher_consistency: N=%d, P=%d", p->N, p->P);
    const long total = (long)p->N * p->P;
    CHAP_CHECK_ARG(total < (1L << 32), "chap_teacher_consistency: N*P=%ld exceeds the 32-bit pixel index", total);
    CHAP_CHECK_ARG((((uintptr_t)p->logits[0] | (uintptr_t)p->logits[1] | (uintptr_t)p->teacher[0] | (uintptr_t)p->teacher[1] | (uintptr_t)p->dlogits[0] |
                     (uintptr_t)p->dlogits[1] | (uintptr_t)p->loss | (uintptr_t)p->ws | (uintptr_t)p->gscale_dev) & 3) == 0, "chap_teacher_consistency: pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the grid the kernel's path needs, capped so the partial rows suffice (the kernel takes the same decision from the same values)
    const bool quads = (p->P & 3) == 0 && (((uintptr_t)p->logits[0] | (uintptr_t)p->logits[1] | (uintptr_t)p->teacher[0] | (uintptr_t)p->teacher[1] |
                                            (uintptr_t)p->dlogits[0] | (uintptr_t)p->dlogits[1]) & 15) == 0;
    const long units = quads ? total >> 2 : total;
    const long blocks = (units + 255) / 256;
    const int nb = (int)(blocks < CHAP_LOSS_SLOTS ? blocks : CHAP_LOSS_SLOTS);
    switch (p->C) { TC_CASE(2) TC_CASE(3) TC_CASE(4) TC_CASE(5) TC_CASE(6) TC_CASE(7) TC_CASE(8) default: break; }
    CHAP_LAUNCH_CHECK("chap_teacher_consistency");
    hipLaunchKernelGGL(teacher_consistency_final_kernel, dim3(1), dim3(256), 0, s, p->ws, nb, 1.f / ((float)total * (float)p->C), p->loss);
    CHAP_LAUNCH_CHECK("chap_teacher_consistency(final)");
    return CHAP_OK;
}
