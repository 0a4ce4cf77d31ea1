/*
 * chap_hip_guard.h -- the gradient guard of libchap_hip.so, additive to ABI 9 of chap_hip.h.
 *
 * An opt-in like chap_hip_ext.h and chap_hip_monitor.h, in a header of its own: include this file (it includes chap_hip.h).  No launch of
 * chap_amd.train.ChapStep issues these entry points unless the caller attaches a chap_amd.guard.StepGuard, and the ctypes binding keeps them
 * in a table of their own (chap_amd/_lib.py: _SIGS_GUARD).
 *
 * Definitions.  The gradient the optimizer applies is h * grad_scale with h = grad + grad2 formed in fp32 (sgd_kernel's sum).
 *     norm  = sqrt(sum h^2) * grad_scale                      (fp64; the global L2 norm of torch.nn.utils.clip_grad_norm_)
 *     nonfinite = !isfinite(sum h^2)                          (exact: at most 2^31 squares of finite fp32 values cannot overflow fp64, and
 *                                                              one inf or NaN among the h makes the sum non-finite)
 *     skip  = nonfinite && skip_nonfinite
 *     coef  = skip ? 0 : (max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1)      (clip_grad_norm_'s clip_coef, in fp64, rounded once to fp32;
 *                                                              min is C's fmin: a NaN quotient -- reachable only with skip_nonfinite == 0 -- gives 1)
 * The sum runs in a fixed order that depends on n alone: no atomics, the same bits on every device, every launch and every rank.
 */
#ifndef CHAP_HIP_GUARD_H
#define CHAP_HIP_GUARD_H
#include "chap_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHAP_GRADNORM_SLOTS 512         /* blocks of the partials kernel = fp64 words of its workspace, whatever the device or n */

/* The state block in device memory: this header, then `ring` rows.  chap_grad_norm writes all of it (and advances the three counters itself:
 * a replayed graph needs no host upload); chap_sgd_guard_step reads scale and skip. */
typedef struct {
    float scale;                /* coef of the step in flight                                                      */
    int32_t skip;               /* 1: the optimizer leaves param / mom / ema alone                                 */
    float norm;                 /* before clipping; inf / NaN when non-finite                                      */
    int32_t steps;              /* chap_grad_norm launches so far                                                  */
    int32_t skipped_total;      /* ... of which skip == 1                                                          */
    int32_t clipped_total;      /* ... of which skip == 0 and coef < 1                                             */
    int32_t reserved[2];        /* written as 0 (keeps the rows 16-byte aligned)                                   */
} chap_guard_state;
typedef struct { int32_t step; float norm; float coef; int32_t skip; } chap_guard_row;      /* step: 1-based, `steps` after the launch */
#define CHAP_GUARD_STATE_BYTES(ring) (sizeof(chap_guard_state) + (size_t)(ring) * sizeof(chap_guard_row))

/* Two launches on `stream`: CHAP_GRADNORM_SLOTS blocks of 256 threads leave one fp64 partial each in `ws` (nothing to zero), one block adds them
 * in a fixed order and writes the state header and the row (steps % ring), steps the counter before this launch. */
typedef struct {
    const float* grad;          /* [n], 16-byte aligned                                                            */
    const float* grad2;         /* second bucket or NULL                                                           */
    int64_t n;
    float grad_scale;
    float max_norm;             /* <= 0: no clipping                                                               */
    int32_t skip_nonfinite;
    int32_t ring;               /* rows behind the header of `state`, >= 1                                         */
    double* ws;                 /* CHAP_GRADNORM_SLOTS doubles                                                     */
    chap_guard_state* state;    /* CHAP_GUARD_STATE_BYTES(ring) bytes, 16-byte aligned                             */
} chap_grad_norm_params;
int chap_grad_norm(const chap_grad_norm_params* p, void* stream);

/* chap_sgd_step (se.ema == NULL) or chap_sgd_ema_step with the gradient scaled by s = grad_scale * state->scale, one fp32 product formed once:
 * with scale == 1 the bits of the plain entries, with scale == c the bits of the plain entries called with grad_scale = fl32(grad_scale * c).
 * state->skip != 0: param, mom and ema are not written.  The buckets are zeroed whenever zero_grad is set, on the skip path too. */
typedef struct { chap_sgd_ema_params se; const chap_guard_state* state; } chap_sgd_guard_params;
int chap_sgd_guard_step(const chap_sgd_guard_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
