// Training input on the device: RandomGenerator (rot90 + flip | rotate, then zoom, all order 0) as one gather per output pixel from a
// slice store in HBM, and the 3D crop + rot90 + flip (chap_augment3d_padded: from a zero-padded volume).  Contract: include/chap_hip.h
// (chap_augment2d / chap_augment3d / chap_augment3d_padded); exactness
// argument: DESIGN.md "Data layer".  Bandwidth-trivial (one batch is a few MB): one thread per four output pixels along W, image and
// label from the same index, 16-byte stores, no LDS.
#include "common.h"

namespace {

constexpr int AUG_TB = 256;

struct AugIdx { long src; bool inside; };

// Source element of output pixel (o0, o1) of one record.  Everything that decides a pixel is fp64 with the operation order of scipy's
// compiled loops; contraction is OFF here: a fused multiply-add rounds once where scipy rounds twice, which moves floor(c + 0.5) and the
// inside test on ties.
__device__ __forceinline__ AugIdx aug_index2d(const chap_augment2d_record& r, int xi, int yi, double c0, bool in0, int o1) {
#pragma clang fp contract(off)
    AugIdx a;
    const double c1 = (double)o1 * r.zoom[1];
    a.inside = in0 && c1 >= 0.0 && c1 <= (double)(yi - 1);
    int i = (int)floor(c0 + 0.5), j = (int)floor(c1 + 0.5);
    const int x = r.x, y = r.y;
    if (r.mode == CHAP_AUG_ROTFLIP) {
        if (r.axis & 1) j = yi - 1 - j; else i = xi - 1 - i;
        int si, sj;
        switch (r.k & 3) {
            case 0: si = i; sj = j; break;
            case 1: si = j; sj = y - 1 - i; break;
            case 2: si = x - 1 - i; sj = y - 1 - j; break;
            default: si = x - 1 - j; sj = i; break;
        }
        i = si; j = sj;
    } else if (r.mode == CHAP_AUG_ROTATE) {
        const double fi = (double)i, fj = (double)j;
        double ch = r.off[0] + fi * r.m[0];
        ch = ch + fj * r.m[1];
        double cw = r.off[1] + fi * r.m[2];
        cw = cw + fj * r.m[3];
        a.inside = a.inside && ch >= 0.0 && ch <= (double)(x - 1) && cw >= 0.0 && cw <= (double)(y - 1);
        i = (int)floor(ch + 0.5); j = (int)floor(cw + 0.5);
    }
    a.inside = a.inside && i >= 0 && i < x && j >= 0 && j < y;      // implied by the tests above; keeps every read inside the slice
    a.src = r.offset + (long)i * y + j;
    return a;
}

__device__ __forceinline__ void aug_store4(float* img, void* lab, int i64, long o, const float v[4], const uint8_t l[4], int n, bool vec) {
    if (vec) {
        *(float4*)(img + o) = make_float4(v[0], v[1], v[2], v[3]);
        if (i64) {
            long long* q = (long long*)lab + o;
            *(longlong2*)q = make_longlong2(l[0], l[1]);
            *(longlong2*)(q + 2) = make_longlong2(l[2], l[3]);
        } else {
            *(uchar4*)((uint8_t*)lab + o) = make_uchar4(l[0], l[1], l[2], l[3]);
        }
    } else {
        for (int e = 0; e < n; ++e) {
            img[o + e] = v[e];
            if (i64) ((long long*)lab)[o + e] = l[e]; else ((uint8_t*)lab)[o + e] = l[e];
        }
    }
}

// grid (quads of a sample, B); vec: W % 4 == 0 and 16-byte aligned outputs
__global__ __launch_bounds__(AUG_TB) void aug2d_kernel(const chap_augment2d_params P, int vec) {
#pragma clang fp contract(off)
    const int H = P.H, W = P.W, WQ = (W + 3) >> 2;
    const int q = blockIdx.x * AUG_TB + threadIdx.x;
    if (q >= H * WQ) return;
    const int b = blockIdx.y;
    const chap_augment2d_record r = P.records[b];
    const bool ok = r.offset >= 0 && r.x >= 1 && r.y >= 1 && r.offset + (long)r.x * r.y <= P.store_elems;
    const bool swap = r.mode == CHAP_AUG_ROTFLIP && (r.k & 1);
    const int xi = swap ? r.y : r.x, yi = swap ? r.x : r.y;         // the shape the zoom sees
    const int o0 = q / WQ, w0 = (q - o0 * WQ) << 2;
    const double c0 = (double)o0 * r.zoom[0];
    const bool in0 = ok && c0 >= 0.0 && c0 <= (double)(xi - 1);
    float v[4]; uint8_t l[4];
    const int n = min(4, W - w0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = 0.f; l[e] = 0;
        if (e < n) {
            const AugIdx a = aug_index2d(r, xi, yi, c0, in0, w0 + e);
            if (a.inside) { v[e] = P.images[a.src]; l[e] = P.labels[a.src]; }
        }
    }
    aug_store4(P.image_out, P.label_out, P.label_i64, ((long)b * H + o0) * W + w0, v, l, n, vec != 0);
}

// rot90(k) in the first two axes, then flip(axis): output voxel (i, j) of a [P0][P1] plane -> (si, sj) in the [n0][n1] crop
__device__ __forceinline__ void aug3d_rotflip(int k, int axis, int P0, int P1, int n0, int n1, int i, int j, int& si, int& sj) {
    if (axis & 1) j = P1 - 1 - j; else i = P0 - 1 - i;
    switch (k & 3) {
        case 0: si = i; sj = j; break;
        case 1: si = j; sj = n1 - 1 - i; break;
        case 2: si = n0 - 1 - i; sj = n1 - 1 - j; break;
        default: si = n0 - 1 - j; sj = i; break;
    }
}

// grid (quads of a sample, B)
__global__ __launch_bounds__(AUG_TB) void aug3d_kernel(const chap_augment3d_params P, int vec) {
    const int P0 = P.P0, P1 = P.P1, P2 = P.P2, WQ = (P2 + 3) >> 2;
    const long q = (long)blockIdx.x * AUG_TB + threadIdx.x;
    if (q >= (long)P0 * P1 * WQ) return;
    const int b = blockIdx.y;
    const chap_augment3d_record r = P.records[b];
    const int n0 = (r.k & 1) ? P1 : P0, n1 = (r.k & 1) ? P0 : P1;  // the crop
    bool ok = r.offset >= 0 && r.offset + (long)r.shape[0] * r.shape[1] * r.shape[2] <= P.store_elems;
    ok = ok && r.corner[0] >= 0 && r.corner[1] >= 0 && r.corner[2] >= 0
            && r.corner[0] + n0 <= r.shape[0] && r.corner[1] + n1 <= r.shape[1] && r.corner[2] + P2 <= r.shape[2];
    const int w0 = (int)(q % WQ) << 2;
    const int j = (int)((q / WQ) % P1), i = (int)(q / ((long)WQ * P1));
    const long o = (((long)b * P0 + i) * P1 + j) * P2 + w0;
    int si, sj;
    aug3d_rotflip(r.k, r.axis, P0, P1, n0, n1, i, j, si, sj);
    const long src = r.offset + ((long)(r.corner[0] + si) * r.shape[1] + (r.corner[1] + sj)) * r.shape[2] + r.corner[2] + w0;
    float v[4]; uint8_t l[4];
    const int n = min(4, P2 - w0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = 0.f; l[e] = 0;
        if (ok && e < n) { v[e] = P.images[src + e]; l[e] = P.labels[src + e]; }
    }
    aug_store4(P.image_out, P.label_out, P.label_i64, o, v, l, n, vec != 0);
}

// aug3d_kernel on a volume surrounded by r.pad zero voxels per axis: the same index maps, then the shift by pad and one inside test per voxel
__global__ __launch_bounds__(AUG_TB) void aug3d_pad_kernel(const chap_augment3d_pad_params P, int vec) {
    const int P0 = P.P0, P1 = P.P1, P2 = P.P2, WQ = (P2 + 3) >> 2;
    const long q = (long)blockIdx.x * AUG_TB + threadIdx.x;
    if (q >= (long)P0 * P1 * WQ) return;
    const int b = blockIdx.y;
    const chap_augment3d_pad_record r = P.records[b];
    const int n0 = (r.k & 1) ? P1 : P0, n1 = (r.k & 1) ? P0 : P1;  // the crop
    bool ok = r.offset >= 0 && r.shape[0] >= 1 && r.shape[1] >= 1 && r.shape[2] >= 1
              && r.offset + (long)r.shape[0] * r.shape[1] * r.shape[2] <= P.store_elems;
    ok = ok && r.pad[0] >= 0 && r.pad[1] >= 0 && r.pad[2] >= 0 && r.corner[0] >= 0 && r.corner[1] >= 0 && r.corner[2] >= 0
            && (long)r.corner[0] + n0 <= (long)r.shape[0] + 2L * r.pad[0] && (long)r.corner[1] + n1 <= (long)r.shape[1] + 2L * r.pad[1]
            && (long)r.corner[2] + P2 <= (long)r.shape[2] + 2L * r.pad[2];
    const int w0 = (int)(q % WQ) << 2;
    const int j = (int)((q / WQ) % P1), i = (int)(q / ((long)WQ * P1));
    const long o = (((long)b * P0 + i) * P1 + j) * P2 + w0;
    int si, sj;
    aug3d_rotflip(r.k, r.axis, P0, P1, n0, n1, i, j, si, sj);
    const long t0 = (long)r.corner[0] + si - r.pad[0], t1 = (long)r.corner[1] + sj - r.pad[1], t2 = (long)r.corner[2] + w0 - r.pad[2];
    const bool in01 = ok && t0 >= 0 && t0 < r.shape[0] && t1 >= 0 && t1 < r.shape[1];
    const long src = r.offset + (t0 * r.shape[1] + t1) * r.shape[2] + t2;
    float v[4]; uint8_t l[4];
    const int n = min(4, P2 - w0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = 0.f; l[e] = 0;
        if (in01 && e < n && t2 + e >= 0 && t2 + e < r.shape[2]) { v[e] = P.images[src + e]; l[e] = P.labels[src + e]; }
    }
    aug_store4(P.image_out, P.label_out, P.label_i64, o, v, l, n, vec != 0);
}

bool aug_vec_ok(const void* img, const void* lab, int W) {
    return W % 4 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)lab & 15) == 0;
}

}  // namespace

extern "C" int chap_augment2d(const chap_augment2d_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->images && p->labels && p->records && p->image_out && p->label_out, "chap_augment2d: null argument");
    CHAP_CHECK_ARG(p->B >= 1 && p->B <= 65535, "chap_augment2d: B must be in [1, 65535] (got %d)", p->B);
    CHAP_CHECK_ARG(p->H >= 2 && p->W >= 2 && (long)p->H * p->W < (1L << 30), "chap_augment2d: output must be at least 2 x 2 and below 2^30 pixels (got %d x %d)", p->H, p->W);
    CHAP_CHECK_ARG(p->label_i64 == 0 || p->label_i64 == 1, "chap_augment2d: label_i64 must be 0 or 1");
    CHAP_CHECK_ARG(p->store_elems >= 1, "chap_augment2d: empty store");
    const long quads = (long)p->H * ((p->W + 3) / 4);
    hipLaunchKernelGGL(aug2d_kernel, dim3((unsigned)((quads + AUG_TB - 1) / AUG_TB), (unsigned)p->B), dim3(AUG_TB), 0, (hipStream_t)stream,
                       *p, (int)aug_vec_ok(p->image_out, p->label_out, p->W));
    CHAP_LAUNCH_CHECK("chap_augment2d");
    return CHAP_OK;
}

extern "C" int chap_augment3d(const chap_augment3d_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->images && p->labels && p->records && p->image_out && p->label_out, "chap_augment3d: null argument");
    CHAP_CHECK_ARG(p->B >= 1 && p->B <= 65535, "chap_augment3d: B must be in [1, 65535] (got %d)", p->B);
    CHAP_CHECK_ARG(p->P0 >= 1 && p->P1 >= 1 && p->P2 >= 1 && (long)p->P0 * p->P1 * p->P2 < (1L << 31),
                   "chap_augment3d: patch must be non-empty and below 2^31 voxels (got %d x %d x %d)", p->P0, p->P1, p->P2);
    CHAP_CHECK_ARG(p->label_i64 == 0 || p->label_i64 == 1, "chap_augment3d: label_i64 must be 0 or 1");
    CHAP_CHECK_ARG(p->store_elems >= 1, "chap_augment3d: empty store");
    const long quads = (long)p->P0 * p->P1 * ((p->P2 + 3) / 4);
    hipLaunchKernelGGL(aug3d_kernel, dim3((unsigned)((quads + AUG_TB - 1) / AUG_TB), (unsigned)p->B), dim3(AUG_TB), 0, (hipStream_t)stream,
                       *p, (int)aug_vec_ok(p->image_out, p->label_out, p->P2));
    CHAP_LAUNCH_CHECK("chap_augment3d");
    return CHAP_OK;
}

extern "C" int chap_augment3d_padded(const chap_augment3d_pad_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->images && p->labels && p->records && p->image_out && p->label_out, "chap_augment3d_padded: null argument");
    CHAP_CHECK_ARG(p->B >= 1 && p->B <= 65535, "chap_augment3d_padded: B must be in [1, 65535] (got %d)", p->B);
    CHAP_CHECK_ARG(p->P0 >= 1 && p->P1 >= 1 && p->P2 >= 1 && (long)p->P0 * p->P1 * p->P2 < (1L << 31),
                   "chap_augment3d_padded: patch must be non-empty and below 2^31 voxels (got %d x %d x %d)", p->P0, p->P1, p->P2);
    CHAP_CHECK_ARG(p->label_i64 == 0 || p->label_i64 == 1, "chap_augment3d_padded: label_i64 must be 0 or 1");
    CHAP_CHECK_ARG(p->store_elems >= 1, "chap_augment3d_padded: empty store");
    const long quads = (long)p->P0 * p->P1 * ((p->P2 + 3) / 4);
    hipLaunchKernelGGL(aug3d_pad_kernel, dim3((unsigned)((quads + AUG_TB - 1) / AUG_TB), (unsigned)p->B), dim3(AUG_TB), 0, (hipStream_t)stream,
                       *p, (int)aug_vec_ok(p->image_out, p->label_out, p->P2));
    CHAP_LAUNCH_CHECK("chap_augment3d_padded");
    return CHAP_OK;
}
