/*
 * chap_hip_teacher.h -- the mean teacher's consistency term of libchap_hip.so, additive to ABI 9 of chap_hip.h.
 *
 * An opt-in like chap_hip_optim.h, in a header of its own: include this file (it includes chap_hip.h).  No launch of
 * chap_amd.train.ChapStep issues this entry point unless the step is built with args['teacher_consistency'] > 0, and the ctypes binding
 * keeps it in a table of its own (chap_amd/_lib.py: _TEACHER_SIGS).
 *
 * Definitions (Tarvainen and Valpola's softmax-MSE consistency, softmax_mse_loss of the public mean-teacher code, against the ensemble of
 * the teacher's two heads).  All tensors are planar fp32 [N][C][P]; per pixel (n, p) and with softmax over the C classes:
 *     q_c     = 0.5 * (softmax(teacher[0])_c + softmax(teacher[1])_c)
 *     p_h     = softmax(logits[h]),  e_h = p_h - q                                   (h = 0, 1: the student's heads)
 *     loss    = sum_h  1 / (N C P) * sum_{n,c,p} e_{h,c}^2
 *     G       = gscale * (gscale_dev ? *gscale_dev : 1) * 2 / (N C P)
 *     d loss / d logits[h]_k = G * p_k * (e_k - sum_c p_c e_c)
 * `loss` is written (not added to).  dlogits[h] receives the gradient, or -- `accumulate` != 0 -- prior + gradient in one rounding; a NULL
 * dlogits[h] is skipped.  Every softmax subtracts the pixel's maximum and uses expf.  The kernel leaves one partial sum per block and head
 * in ws, a one-block kernel adds them in fixed order in fp64: no atomics, two launches give identical bits.
 */
#ifndef CHAP_HIP_TEACHER_H
#define CHAP_HIP_TEACHER_H
#include "chap_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One streaming launch (forward and gradient together) and a one-block finalize: 4 N C P floats read, and per given dlogits N C P written
 * (with `accumulate` also read).  C = 2..8, N * P < 2^32.  Four pixels per thread with 16-byte accesses when P % 4 == 0 and all six tensor
 * pointers are 16-byte aligned, one pixel per thread otherwise. */
typedef struct {
    const float* logits[2];     /* the student's heads                                                             */
    const float* teacher[2];    /* the teacher's heads                                                             */
    float* dlogits[2];          /* either may be NULL                                                              */
    float* loss;                /* [1], written                                                                    */
    float* ws;                  /* [1 + CHAP_LOSS_SLOTS][2]: row 0 <- the heads' sums, rows 1.. per-block partials; nothing needs zeroing */
    const float* gscale_dev;    /* optional device scalar                                                          */
    float gscale;
    int32_t accumulate;
    int32_t N, C, P;
} chap_teacher_consistency_params;
int chap_teacher_consistency(const chap_teacher_consistency_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
