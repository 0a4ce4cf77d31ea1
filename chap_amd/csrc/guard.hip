// Gradient guard (include/chap_hip_guard.h): the global L2 norm of the gradient the optimizer is about to apply, in a fixed order and
// without atomics, and the optimizer kernel that reads the clip coefficient and the skip flag that norm gives from device memory.
// chap_grad_norm is HBM-bound (both buckets read once, 16 bytes per load; the fp64 accumulation is four v_fma_f64 per load, far below the
// load rate); chap_sgd_guard_step is sgd_kernel / sgd_ema_kernel of aux.hip with one more word read per thread.
#include "common.h"
#include "chap_hip_guard.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {      // xor butterfly: the same pairing on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One fp64 partial per block.  Thread t of the fixed grid owns the vectors t, t + T, t + 2T, ... (T = CHAP_GRADNORM_SLOTS * 256) and adds their
// squares in that order; block 0 adds the scalar tail n % 4 as sgd_kernel applies it.  h = g + g2 is the fp32 sum sgd_kernel forms; the
// square of an fp32 value is exact in fp64, so the only rounding is the additions'.
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const chap_grad_norm_params P) {
    __shared__ double sm[4];
    const long n4 = P.n / 4;
    const long T = (long)CHAP_GRADNORM_SLOTS * 256;
    const float4* __restrict__ g1 = (const float4*)P.grad;
    const float4* __restrict__ g2 = (const float4*)P.grad2;
    double acc = 0.0;
#pragma unroll 4
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += T) {
        float4 g = g1[i];
        if (g2) { const float4 h = g2[i]; g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w; }
        acc += (double)g.x * (double)g.x; acc += (double)g.y * (double)g.y; acc += (double)g.z * (double)g.z; acc += (double)g.w * (double)g.w;
    }
    if (blockIdx.x == 0) {
        for (long i = n4 * 4 + threadIdx.x; i < P.n; i += 256) {
            const float gr = P.grad[i] + (P.grad2 ? P.grad2[i] : 0.f);
            acc += (double)gr * (double)gr;
        }
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) P.ws[blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// One wave: lane l adds the partials l, l + 64, ..., l + 448 in that order, the butterfly adds the lanes, lane 0 writes the state block.
__global__ __launch_bounds__(64) void grad_norm_total_kernel(const chap_grad_norm_params P) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < CHAP_GRADNORM_SLOTS / 64; ++k) v += P.ws[k * 64 + threadIdx.x];
    const double total = wave_sum_f64(v);
    if (threadIdx.x != 0) return;
    chap_guard_state* st = P.state;
    const double norm = sqrt(total) * (double)P.grad_scale;
    const bool nonfinite = !isfinite(total);
    const int skip = (nonfinite && P.skip_nonfinite) ? 1 : 0;
    const double c = skip ? 0.0 : (P.max_norm > 0.f ? fmin(1.0, (double)P.max_norm / (norm + 1e-6)) : 1.0);
    const float coef = (float)c, normf = (float)norm;
    const int steps = st->steps, skipped = st->skipped_total + skip, clipped = st->clipped_total + ((!skip && coef < 1.f) ? 1 : 0);
    chap_guard_row* row = (chap_guard_row*)(st + 1) + (unsigned)steps % (unsigned)P.ring;       // (unsigned: inside the ring whatever the counter holds)
    *(int4*)st = make_int4(__float_as_int(coef), skip, __float_as_int(normf), steps + 1);
    *((int4*)st + 1) = make_int4(skipped, clipped, 0, 0);
    *(int4*)row = make_int4(steps + 1, __float_as_int(normf), __float_as_int(coef), skip);
}

// sgd_kernel / sgd_ema_kernel (aux.hip) with s = grad_scale * state->scale in place of grad_scale: the expressions are theirs token for token,
// so the compiler contracts them the same way and scale == 1 gives their bits.  (g * grad_scale * scale as a third factor would not: another
// product would be the fused one.)  skip: nothing but the zeroing of the buckets, which the engine accumulates into.
#define CHAP_GUARD_SGD1(f) { const float gg = g.f * s + P.weight_decay * p.f; m.f = P.momentum * m.f + gg; p.f -= lr * m.f; }
template <bool EMA>
__global__ void sgd_guard_kernel(const chap_sgd_guard_params G) {
    const chap_sgd_params& P = G.se.sgd;
    const float lr = *P.lr;
    const float s = P.grad_scale * G.state->scale;
    const int skip = G.state->skip;
    float ca = 0.f, cb = 0.f;
    if (EMA) { ca = G.se.coef[0]; cb = G.se.coef[1]; }
    const long n4 = P.n / 4;
    if (skip) {
        if (!P.zero_grad) return;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
            ((float4*)P.grad)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (P.grad2) ((float4*)P.grad2)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (blockIdx.x == 0)
            for (long i = n4 * 4 + threadIdx.x; i < P.n; i += blockDim.x) { P.grad[i] = 0.f; if (P.grad2) P.grad2[i] = 0.f; }
        return;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 p = ((float4*)P.param)[i], g = ((float4*)P.grad)[i], m = ((float4*)P.mom)[i];
        if (P.grad2) { const float4 h = ((float4*)P.grad2)[i]; g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w; }
        CHAP_GUARD_SGD1(x) CHAP_GUARD_SGD1(y) CHAP_GUARD_SGD1(z) CHAP_GUARD_SGD1(w)
        if (EMA) {
            float4 e = ((float4*)G.se.ema)[i];
            e.x = ca * e.x + cb * p.x; e.y = ca * e.y + cb * p.y; e.z = ca * e.z + cb * p.z; e.w = ca * e.w + cb * p.w;
            ((float4*)G.se.ema)[i] = e;
        }
        ((float4*)P.param)[i] = p; ((float4*)P.mom)[i] = m;
        if (P.zero_grad) {
            ((float4*)P.grad)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (P.grad2) ((float4*)P.grad2)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if (blockIdx.x == 0) {
        for (long i = n4 * 4 + threadIdx.x; i < P.n; i += blockDim.x) {
            const float gr = P.grad[i] + (P.grad2 ? P.grad2[i] : 0.f);
            const float gg = gr * s + P.weight_decay * P.param[i];
            const float mm = P.momentum * P.mom[i] + gg;
            const float pn = P.param[i] - lr * mm;
            P.mom[i] = mm; P.param[i] = pn;
            if (EMA) G.se.ema[i] = ca * G.se.ema[i] + cb * pn;
            if (P.zero_grad) { P.grad[i] = 0.f; if (P.grad2) P.grad2[i] = 0.f; }
        }
    }
}

}  // namespace

extern "C" int chap_grad_norm(const chap_grad_norm_params* p, void* stream) {
    CHAP_CHECK_ARG(p, "chap_grad_norm: null argument");
    CHAP_CHECK_ARG(p->grad && p->ws && p->state && p->n > 0, "chap_grad_norm: bad argument");
    CHAP_CHECK_ARG(p->ring >= 1, "chap_grad_norm: ring=%d", p->ring);
    CHAP_CHECK_ARG(((uintptr_t)p->grad | (uintptr_t)p->grad2 | (uintptr_t)p->state) % 16 == 0 && (uintptr_t)p->ws % 8 == 0,
                   "chap_grad_norm: grad, grad2 and state must be 16-byte, ws 8-byte aligned");
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(CHAP_GRADNORM_SLOTS), dim3(256), 0, (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_grad_norm(partials)");
    hipLaunchKernelGGL(grad_norm_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_grad_norm(totals)");
    return CHAP_OK;
}

extern "C" int chap_sgd_guard_step(const chap_sgd_guard_params* q, void* stream) {
    CHAP_CHECK_ARG(q, "chap_sgd_guard_step: null argument");
    const chap_sgd_params* p = &q->se.sgd;
    CHAP_CHECK_ARG(p->param && p->grad && p->mom && p->lr && p->n > 0, "chap_sgd_guard_step: bad argument");
    CHAP_CHECK_ARG(q->state, "chap_sgd_guard_step: null state");
    CHAP_CHECK_ARG(!q->se.ema || q->se.coef, "chap_sgd_guard_step: null coef");
    CHAP_CHECK_ARG(((uintptr_t)p->param | (uintptr_t)p->grad | (uintptr_t)p->grad2 | (uintptr_t)p->mom | (uintptr_t)q->se.ema | (uintptr_t)q->state) % 16 == 0,
                   "chap_sgd_guard_step: buffers must be 16-byte aligned");
    const long n4 = p->n / 4;
    const int nb = chap_blocks(n4, 2048);
    if (q->se.ema) hipLaunchKernelGGL(sgd_guard_kernel<true>, dim3(nb > 0 ? nb : 1), dim3(256), 0, (hipStream_t)stream, *q);
    else hipLaunchKernelGGL(sgd_guard_kernel<false>, dim3(nb > 0 ? nb : 1), dim3(256), 0, (hipStream_t)stream, *q);
    CHAP_LAUNCH_CHECK("chap_sgd_guard_step");
    return CHAP_OK;
}
