// Adam / AdamW (include/chap_hip_optim.h): the step counter and bias corrections in device memory (chap_adam_tick, one wave) and one streaming
// kernel over the flat buffers (chap_adam_step) with sgd_kernel's structure -- float4 body, scalar tail on block 0, grid-stride, no atomics.
// HBM-bound like sgd_kernel: 32 bytes per parameter (40 with the mean teacher's average), one correctly rounded sqrt and two divisions per
// element beside them.  The guard's scale and skip words are read as sgd_guard_kernel (guard.hip) reads them.
#include "common.h"
#include "chap_hip_optim.h"

namespace {

// What the kernel gets: the caller's struct and the two host-formed complements fl32(1 - (double)beta).
struct adam_args { chap_adam_params P; float omb1, omb2; };

__global__ __launch_bounds__(64) void adam_tick_kernel(const chap_adam_tick_params T) {
    if (threadIdx.x != 0) return;
    if (T.guard && T.guard->skip) return;           // a skipped step does not count
    const int t = T.state->step + 1;
    const double lr = (double)*T.lr;
    const double bc1 = 1.0 - pow((double)T.beta1, (double)t);
    const double bc2 = 1.0 - pow((double)T.beta2, (double)t);
    const float step_size = (float)(lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    const float decay = T.decoupled ? (float)(1.0 - lr * (double)T.weight_decay) : 1.f;
    *(int4*)T.state = make_int4(t, __float_as_int(step_size), __float_as_int(bc2_sqrt), __float_as_int(decay));
}

// The order of the header, one element.  `dec` is uniform over the launch.
#define CHAP_ADAM1(f) { float x = g.f * s; \
    if (!dec) x = x + P.weight_decay * p.f; else p.f = p.f * decay; \
    m.f = P.beta1 * m.f + A.omb1 * x; \
    v.f = P.beta2 * v.f + (A.omb2 * x) * x; \
    const float den = sqrtf(v.f) / bc2_sqrt + P.eps; \
    p.f = p.f - step_size * (m.f / den); }

template <bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(const adam_args A) {
    const chap_adam_params& P = A.P;
    // the words every thread needs, once, in front of the loop
    const int4 st = *(const int4*)P.state;
    const float step_size = __int_as_float(st.y), bc2_sqrt = __int_as_float(st.z), decay = __int_as_float(st.w);
    float s = P.grad_scale;
    int skip = 0;
    if (P.guard) { s = P.grad_scale * P.guard->scale; skip = P.guard->skip; }
    float ca = 0.f, cb = 0.f;
    if (EMA) { ca = P.coef[0]; cb = P.coef[1]; }
    const bool dec = P.decoupled != 0;
    const long n4 = P.n / 4;
    const long stride = (long)gridDim.x * blockDim.x;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (skip) {
        if (!P.zero_grad) return;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            ((float4*)P.grad)[i] = zero;
            if (P.grad2) ((float4*)P.grad2)[i] = zero;
        }
        if (blockIdx.x == 0)
            for (long i = n4 * 4 + threadIdx.x; i < P.n; i += blockDim.x) { P.grad[i] = 0.f; if (P.grad2) P.grad2[i] = 0.f; }
        return;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        // every load of the trip before the first use
        float4 p = ((const float4*)P.param)[i], g = ((const float4*)P.grad)[i], m = ((const float4*)P.exp_avg)[i], v = ((const float4*)P.exp_avg_sq)[i];
        float4 h = zero, e = zero;
        if (EMA) e = ((const float4*)P.ema)[i];
        if (P.grad2) h = ((const float4*)P.grad2)[i];
        if (P.grad2) { g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w; }
        CHAP_ADAM1(x) CHAP_ADAM1(y) CHAP_ADAM1(z) CHAP_ADAM1(w)
        if (EMA) {
            e.x = ca * e.x + cb * p.x; e.y = ca * e.y + cb * p.y; e.z = ca * e.z + cb * p.z; e.w = ca * e.w + cb * p.w;
            ((float4*)P.ema)[i] = e;
        }
        ((float4*)P.param)[i] = p; ((float4*)P.exp_avg)[i] = m; ((float4*)P.exp_avg_sq)[i] = v;
        if (P.zero_grad) {
            ((float4*)P.grad)[i] = zero;
            if (P.grad2) ((float4*)P.grad2)[i] = zero;
        }
    }
    if (blockIdx.x == 0) {
        for (long i = n4 * 4 + threadIdx.x; i < P.n; i += blockDim.x) {
            struct { float x; } p = {P.param[i]}, g = {P.grad[i]}, m = {P.exp_avg[i]}, v = {P.exp_avg_sq[i]};
            if (P.grad2) g.x += P.grad2[i];
            CHAP_ADAM1(x)
            P.param[i] = p.x; P.exp_avg[i] = m.x; P.exp_avg_sq[i] = v.x;
            if (EMA) P.ema[i] = ca * P.ema[i] + cb * p.x;
            if (P.zero_grad) { P.grad[i] = 0.f; if (P.grad2) P.grad2[i] = 0.f; }
        }
    }
}

}  // namespace

extern "C" int chap_adam_tick(const chap_adam_tick_params* p, void* stream) {
    CHAP_CHECK_ARG(p, "chap_adam_tick: null argument");
    CHAP_CHECK_ARG(p->state && p->lr, "chap_adam_tick: null state or lr");
    CHAP_CHECK_ARG((uintptr_t)p->state % 16 == 0, "chap_adam_tick: state must be 16-byte aligned");
    CHAP_CHECK_ARG((uintptr_t)p->lr % 4 == 0 && (uintptr_t)p->guard % 16 == 0, "chap_adam_tick: lr must be 4-byte, guard 16-byte aligned");
    CHAP_CHECK_ARG(p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f, "chap_adam_tick: betas=(%g, %g), need 0 <= beta < 1",
                   (double)p->beta1, (double)p->beta2);
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_adam_tick");
    return CHAP_OK;
}

extern "C" int chap_adam_step(const chap_adam_params* p, void* stream) {
    CHAP_CHECK_ARG(p, "chap_adam_step: null argument");
    CHAP_CHECK_ARG(p->param && p->grad && p->exp_avg && p->exp_avg_sq, "chap_adam_step: null param, grad, exp_avg or exp_avg_sq");
    CHAP_CHECK_ARG(p->state, "chap_adam_step: null state");
    CHAP_CHECK_ARG(p->n > 0, "chap_adam_step: n=%lld", (long long)p->n);
    CHAP_CHECK_ARG(!p->ema || p->coef, "chap_adam_step: null coef");
    CHAP_CHECK_ARG(((uintptr_t)p->param | (uintptr_t)p->grad | (uintptr_t)p->grad2 | (uintptr_t)p->exp_avg | (uintptr_t)p->exp_avg_sq | (uintptr_t)p->ema |
                    (uintptr_t)p->state | (uintptr_t)p->guard) % 16 == 0, "chap_adam_step: buffers, state and guard must be 16-byte aligned");
    CHAP_CHECK_ARG((uintptr_t)p->coef % 4 == 0, "chap_adam_step: coef must be 4-byte aligned");
    CHAP_CHECK_ARG(p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f, "chap_adam_step: betas=(%g, %g), need 0 <= beta < 1",
                   (double)p->beta1, (double)p->beta2);
    CHAP_CHECK_ARG(p->eps > 0.f, "chap_adam_step: eps=%g, need eps > 0", (double)p->eps);
    adam_args a;
    a.P = *p;
    a.omb1 = (float)(1.0 - (double)p->beta1);
    a.omb2 = (float)(1.0 - (double)p->beta2);
    const long n4 = p->n / 4;
    const int nb = chap_blocks(n4, 2048);
    if (p->ema) hipLaunchKernelGGL(adam_kernel<true>, dim3(nb > 0 ? nb : 1), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(adam_kernel<false>, dim3(nb > 0 ? nb : 1), dim3(256), 0, (hipStream_t)stream, a);
    CHAP_LAUNCH_CHECK("chap_adam_step");
    return CHAP_OK;
}
