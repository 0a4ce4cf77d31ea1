/*
 * chap_hip_optim.h -- the second optimizer of libchap_hip.so (Adam / AdamW), additive to ABI 9 of chap_hip.h.
 *
 * An opt-in like chap_hip_guard.h, in a header of its own: include this file (it includes chap_hip_guard.h, which includes chap_hip.h).  No
 * launch of chap_amd.train.ChapStep issues these entry points unless the caller builds the step with a chap_amd.train.FusedAdamW, and the
 * ctypes binding keeps them in a table of their own (chap_amd/_lib.py: _OPTIM_SIGS).
 *
 * Definitions.  beta1, beta2, eps, weight_decay and grad_scale are the fp32 values of the structs below; lr is the fp32 word `lr` points to.
 *
 * chap_adam_tick, once per optimizer step and before chap_adam_step, in fp64 (every fp32 input widened exactly), t = state->step + 1:
 *     bc1       = 1 - beta1^t
 *     bc2       = 1 - beta2^t
 *     step_size = lr / bc1
 *     bc2_sqrt  = sqrt(bc2)
 *     decay     = decoupled ? 1 - lr * weight_decay : 1
 * each of the three rounded once to fp32; state = {t, step_size, bc2_sqrt, decay}.  With a guard whose skip != 0 nothing is written: a
 * skipped step does not advance t (torch.optim.Adam when step() is not called).
 *
 * chap_adam_step, per element and in fp32, every operation rounded on its own unless the compiler fuses a product into the sum that
 * consumes it (an fma: one rounding fewer), in exactly this order:
 *     s   = grad_scale * guard->scale                 (one product formed once per thread; guard == NULL: s = grad_scale)
 *     h   = g + g2                                    (grad2 == NULL: h = g)
 *     x   = h * s
 *     decoupled == 0:   x = x + weight_decay * p      (L2: torch.optim.Adam's weight_decay)
 *     decoupled != 0:   p = p * decay                 (torch.optim.AdamW)
 *     m   = beta1 * m + omb1 * x                      (omb1 = fl32(1 - (double)beta1), formed on the host)
 *     v   = beta2 * v + (omb2 * x) * x                (omb2 = fl32(1 - (double)beta2))
 *     den = sqrt(v) / bc2_sqrt + eps                  (sqrt and both divisions correctly rounded)
 *     p   = p - step_size * (m / den)
 *     ema = a * ema + b * p                           (ema != NULL; a, b = coef[0], coef[1], as chap_sgd_ema_step; p is the new parameter)
 * guard != NULL and guard->skip != 0: param, exp_avg, exp_avg_sq and ema are not written.  The buckets are zeroed whenever zero_grad is
 * set, on the skip path too.  With guard->scale == 1 the bits are those of guard == NULL; with scale == c those of guard == NULL called
 * with grad_scale = fl32(grad_scale * c).  param, exp_avg and exp_avg_sq do not depend on whether ema is given.  No atomics.
 */
#ifndef CHAP_HIP_OPTIM_H
#define CHAP_HIP_OPTIM_H
#include "chap_hip_guard.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The optimizer's state block in device memory, 16 bytes, 16-byte aligned.  chap_adam_tick writes all of it in one store (and advances
 * `step` itself: a replayed graph needs no host upload); chap_adam_step reads the three floats. */
typedef struct {
    int32_t step;               /* t of the last applied step; 0 before the first                                 */
    float step_size;            /* lr / (1 - beta1^t)                                                              */
    float bc2_sqrt;             /* sqrt(1 - beta2^t)                                                               */
    float decay;                /* 1 - lr * weight_decay (decoupled) or 1                                          */
} chap_adam_state;

/* One wave on `stream`. */
typedef struct {
    chap_adam_state* state;             /* 16-byte aligned                                                         */
    const float* lr;                    /* device word                                                             */
    const chap_guard_state* guard;      /* or NULL; skip is read                                                   */
    float beta1, beta2;                 /* 0 <= beta < 1                                                           */
    float weight_decay;
    int32_t decoupled;
} chap_adam_tick_params;
int chap_adam_tick(const chap_adam_tick_params* p, void* stream);

/* One streaming launch over the flat buffers: 32 bytes of traffic per parameter (40 with ema), plus 8 for a second bucket. */
typedef struct {
    float* param;                       /* [n]; every buffer 16-byte aligned                                       */
    float* grad;                        /* [n]                                                                     */
    float* grad2;                       /* second bucket or NULL                                                   */
    float* exp_avg;                     /* [n] m                                                                   */
    float* exp_avg_sq;                  /* [n] v                                                                   */
    const chap_adam_state* state;       /* as chap_adam_tick left it                                               */
    const chap_guard_state* guard;      /* or NULL; scale and skip are read                                        */
    float* ema;                         /* [n] or NULL                                                             */
    const float* coef;                  /* two device words (a, b); required with ema                              */
    float beta1, beta2, eps, weight_decay;
    int32_t decoupled;
    float grad_scale;
    int32_t zero_grad;
    int64_t n;
} chap_adam_params;
int chap_adam_step(const chap_adam_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
