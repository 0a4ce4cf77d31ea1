/*
 * chap_hip_ext.h -- opt-in entry points of libchap_hip.so, additive to ABI 9 of chap_hip.h.
 *
 * A fragment of chap_hip.h: that header includes it last, inside its extern "C" block and after the types used here.  Include
 * chap_hip.h, never this file on its own.  What is declared here is not part of the default training iteration: no launch of
 * chap_amd.train.ChapStep issues it unless the caller asks for the feature, and the ctypes binding keeps these entries in a table
 * of their own (chap_amd/_lib.py: _SIGS_EXT), apart from the table of the iteration's entry points (_SIGS).
 */
#ifndef CHAP_HIP_EXT_H
#define CHAP_HIP_EXT_H

/* chap_sgd_step and, in the same pass, the mean-teacher average of the weights (update_ema_variables, train_ours_2D.py:50-54):
 * ema = a * ema + b * p', p' the parameter just written; param / mom / the gradient buckets get bit for bit what chap_sgd_step writes.
 * coef[0] = a, coef[1] = b: fp32 words in device memory (a replayed graph reads new values).  The caller computes
 * alpha = min(1 - 1/(global_step + 1), ema_decay) (:52) in double and rounds a = alpha and b = 1 - alpha to fp32 separately. */
typedef struct { chap_sgd_params sgd; float* ema; const float* coef; } chap_sgd_ema_params;
int chap_sgd_ema_step(const chap_sgd_ema_params* p, void* stream);

#endif
