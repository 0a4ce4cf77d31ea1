// The soft-max of the inference callers (loss.hip: chap_ensemble_argmax, chap_window_accumulate; window3d.hip:
// chap_window_accumulate_heads).  One definition: the two window kernels must round alike, bit for bit.
#pragma once
#include "common.h"

constexpr int INFER_MAXC = 8;

__device__ __forceinline__ void softmax_c(float* v, int C) {
    float m = v[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) { v[c] = __expf(v[c] - m); s += v[c]; }
    const float inv = 1.f / s;
    for (int c = 0; c < C; ++c) v[c] *= inv;
}
