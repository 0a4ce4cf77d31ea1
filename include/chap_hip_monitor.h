/*
 * chap_hip_monitor.h -- the device-side training monitor of libchap_hip.so, additive to ABI 9 of chap_hip.h.
 *
 * An opt-in like chap_hip_ext.h, in a header of its own: include this file (it includes chap_hip.h).  No launch of chap_amd.train.ChapStep
 * issues these entry points unless the caller attaches a chap_amd.monitor.StepMonitor, and the ctypes binding keeps them in a table of their
 * own (chap_amd/_lib.py: _SIGS_MONITOR).
 *
 * What is counted is pinned to the reference where the reference has it: acc_conf_analysis (train_ours_2D.py:152-193: arg-max, the error mask
 * pred != gt, the confidence sums, the Dice terms), the per-iteration loss line (train_ours_2D.py:404-405) and the head-disagreement ratio
 * (train_ablation_2D.py:180-190).  The split into two groups at a sample index, C classes instead of four, and the Dice terms of the maps
 * behind the largest-component filter are this project's own.
 *
 * All words of the workspace and of the ring are 8 bytes.  Per group (samples [0, n_first) are group 0, [n_first, N) group 1) a row holds, in
 * this order, CHAP_MONITOR_GROUP_WORDS(C) words:
 *     n | n_disagree | gt[C] | n_correct[2 heads] | conf_correct[2] | conf_err[2] | inter[2][C] | pred[2][C]
 * and for the label-map form CHAP_MONITOR_LABEL_WORDS(C) words:  inter_f[2][C] | pred_f[2][C].
 * In the workspace the counts are int64 and the confidence sums fp64 (one partial row per block, nothing to zero); in the ring every word is
 * fp64 (counts are exact up to 2^53).  A ring row, CHAP_MONITOR_ROW_WORDS(C) words:
 *     iteration | group 0 | group 1 | label-map group 0 | label-map group 1 | scalars[CHAP_MONITOR_MAX_SCALARS]
 */
#ifndef CHAP_HIP_MONITOR_H
#define CHAP_HIP_MONITOR_H
#include "chap_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHAP_MONITOR_SLOTS 512          /* per-block partial rows of a group, as CHAP_LOSS_SLOTS */
#define CHAP_MONITOR_MAX_SCALARS 16
#define CHAP_MONITOR_HDR 2              /* words in front of a region's rows: the row counts of group 0 and group 1, written by the launch */
#define CHAP_MONITOR_GROUP_WORDS(C) (8 + 5 * (C))
#define CHAP_MONITOR_LABEL_WORDS(C) (4 * (C))
#define CHAP_MONITOR_ROW_WORDS(C) (1 + 2 * CHAP_MONITOR_GROUP_WORDS(C) + 2 * CHAP_MONITOR_LABEL_WORDS(C) + CHAP_MONITOR_MAX_SCALARS)
/* the workspace: [logits region: HDR + 2 * SLOTS rows of GROUP_WORDS][label-map region: HDR + 2 * SLOTS rows of LABEL_WORDS] */
#define CHAP_MONITOR_LABEL_REGION(C) (CHAP_MONITOR_HDR + 2 * CHAP_MONITOR_SLOTS * CHAP_MONITOR_GROUP_WORDS(C))
#define CHAP_MONITOR_WS_WORDS(C) (CHAP_MONITOR_LABEL_REGION(C) + CHAP_MONITOR_HDR + 2 * CHAP_MONITOR_SLOTS * CHAP_MONITOR_LABEL_WORDS(C))

/* One streaming pass over two heads' fp32 planar logits and the ground-truth label map: what acc_conf_analysis (train_ours_2D.py:152-193)
 * computes from softmax outputs on the host, as counts.  The arg-max is chap_pseudo_block's (first maximum of the soft-max), the confidence
 * max soft-max = 1 / sum exp(z - zmax) in fp32, added in fp64.  A label outside [0, C) counts in n, is never correct (pred != gt, :164-165),
 * its confidence goes to conf_err, and it is in no gt[c].  n_disagree is the count behind the ratio of train_ablation_2D.py:180-190.
 * Writes the logits region of `ws` only.  C in 2..8; P % 4 == 0 and 16-byte aligned tensors take 16-byte loads. */
typedef struct {
    const float* logits[2];     /* [N][C][P] */
    const int64_t* labels;      /* [N][P] */
    void* ws;                   /* CHAP_MONITOR_WS_WORDS(C) 8-byte words */
    int32_t N, C, P, n_first;
} chap_monitor_params;
int chap_monitor_accumulate(const chap_monitor_params* p, void* stream);

/* The same for two integer label maps (the pseudo labels behind the largest-component filter): inter_f / pred_f against `labels`, the Dice
 * terms of calculate_avg_dice as acc_conf_analysis calls it (train_ours_2D.py:168-169).  Writes the label-map region of `ws` only, so it may
 * run on another stream than chap_monitor_accumulate. */
typedef struct {
    const int64_t* maps[2];     /* [N][P] */
    const int64_t* labels;      /* [N][P] */
    void* ws;
    int32_t N, C, P, n_first;
} chap_monitor_labels_params;
int chap_monitor_accumulate_labels(const chap_monitor_labels_params* p, void* stream);

/* One block: fixed-order totals of the partial rows (int64 for counts, fp64 for the confidence sums) and ONE ring row, slot_iter[0] % ring_rows.
 * slot_iter = {slot, iteration}: int32 words in device memory, so that a replayed graph advances them.  scalars[k], k < nscalars: device
 * addresses of fp32 words copied into the row widened exactly (the loss words of the iteration: loss_l / loss_u of the line
 * 'iteration %d : l loss : %f unl loss : %f', train_ours_2D.py:404-405, are sums of them); the remaining scalar words are written as 0.
 * has_labels == 0: no chap_monitor_accumulate_labels launch preceded, the label-map words are written as 0. */
typedef struct {
    const void* ws;
    double* ring;               /* [ring_rows][CHAP_MONITOR_ROW_WORDS(C)] */
    const int32_t* slot_iter;
    const float* scalars[CHAP_MONITOR_MAX_SCALARS];
    int32_t C, ring_rows, nscalars, has_labels;
} chap_monitor_finalize_params;
int chap_monitor_finalize(const chap_monitor_finalize_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
