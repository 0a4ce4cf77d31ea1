/*
 * chap_hip_uncertainty.h -- the uncertainty-aware form of the mean teacher's consistency term of libchap_hip.so, additive to ABI 9 of chap_hip.h.
 *
 * An opt-in like chap_hip_teacher.h, in a header of its own: include this file (it includes chap_hip.h).  No launch of
 * chap_amd.train.ChapStep issues these entry points unless the step is built with args['teacher_uncertainty'] > 0, and the ctypes binding
 * keeps them in a table of its own (chap_amd/_lib.py: _UNCERTAINTY_SIGS).
 *
 * Definitions (the uncertainty-aware mean teacher, Yu et al. 2019: T noisy teacher predictions, the entropy of their mean as a per-pixel
 * uncertainty, the consistency term counted only where it lies under a threshold).  All logits are planar fp32 [N][C][P]; per pixel (n, p),
 * with softmax over the C classes (max-subtracted, expf):
 *     pbar_c  = 1 / (2T) * sum_{k<T} sum_{h<2} softmax(teacher[k][h])_c          (summed in the order k outer, h inner)
 *     H       = - sum_c pbar_c * logf(pbar_c + 1e-6)
 *     m       = H < thr,   thr = threshold_dev ? *threshold_dev : threshold
 *     count   = sum_{n,p} m
 * and, with q = 0.5 * (softmax(teacher[0]) + softmax(teacher[1])) of the TARGET pass, p_h = softmax(logits[h]), e_h = p_h - q as in
 * chap_hip_teacher.h:
 *     den     = (float)C * (float)count + 1e-16f
 *     loss    = sum_h sum_{n,c,p} m * e_{h,c}^2 / den
 *     G       = gscale * (gscale_dev ? *gscale_dev : 1) * 2 / den
 *     d loss / d logits[h]_k = m * G * p_k * (e_k - sum_c p_c e_c)
 * Where m = 0 the gradient is exactly 0: with `accumulate` such an element is not touched, without it +0 is written.  count = 0 gives loss 0
 * and all-zero gradients.  Both kernels leave per-block partials in their workspace and a one-block kernel adds them in fixed order (the
 * count in integers, the loss in fp64): no atomics, two launches give identical bits.
 */
#ifndef CHAP_HIP_UNCERTAINTY_H
#define CHAP_HIP_UNCERTAINTY_H
#include "chap_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHAP_UNCERTAINTY_MAX_T 8

/* One streaming launch and a one-block finalize: 2T N C P floats read, N P bytes written (and N P floats with `entropy`).  C = 2..8,
 * T = 1..8, N * P < 2^32.  Four pixels per thread with 16-byte loads when P % 4 == 0, the first T passes' pointers and `entropy` are 16-byte
 * aligned and `mask` is 4-byte aligned (it is then written as one 32-bit word); one pixel per thread otherwise. */
typedef struct {
    const float* teacher[CHAP_UNCERTAINTY_MAX_T][2];  /* the first T passes' two heads; the rest is ignored                 */
    uint8_t* mask;              /* [N][P], 0 / 1                                                                   */
    float* entropy;             /* [N][P], optional: NULL is skipped                                               */
    int64_t* count;             /* [1], written                                                                    */
    int64_t* ws;                /* [1 + CHAP_LOSS_SLOTS]: row 0 <- the count, rows 1.. per-block partials; nothing needs zeroing */
    const float* threshold_dev; /* optional device scalar: replaces `threshold`                                    */
    float threshold;
    int32_t T;
    int32_t N, C, P;
} chap_teacher_uncertainty_params;
int chap_teacher_uncertainty(const chap_teacher_uncertainty_params* p, void* stream);

/* chap_teacher_consistency with the mask: 4 N C P floats and N P bytes read, and per given dlogits N C P written (with `accumulate`
 * read, and only where m = 1 written).  The four-pixel path needs P % 4 == 0, the six tensor pointers 16-byte and `mask` 4-byte aligned. */
typedef struct {
    const float* logits[2];     /* the student's heads                                                             */
    const float* teacher[2];    /* the target pass's heads                                                         */
    const uint8_t* mask;        /* [N][P], 0 / 1                                                                   */
    const int64_t* count;       /* [1], device: the number of ones in `mask`                                       */
    float* dlogits[2];          /* either may be NULL                                                              */
    float* loss;                /* [1], written                                                                    */
    float* ws;                  /* [1 + CHAP_LOSS_SLOTS][2]: row 0 <- the heads' sums, rows 1.. per-block partials; nothing needs zeroing */
    const float* gscale_dev;    /* optional device scalar                                                          */
    float gscale;
    int32_t accumulate;
    int32_t N, C, P;
} chap_teacher_consistency_masked_params;
int chap_teacher_consistency_masked(const chap_teacher_consistency_masked_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
