// The sliding window of the 3D evaluation on the device (contract: include/chap_hip.h, chap_window_gather /
// chap_window_accumulate_heads; callers: chap_amd/test_3d_patch.py).  chap_window_gather cuts a batch of patches out of the UNPADDED
// volume, the zero padding being an index test (test_3D_util.py:33-34, 59-61 on the host); chap_window_accumulate_heads is
// chap_window_accumulate (loss.hip) for one or two heads.  Both are bandwidth-trivial beside the network they feed: one thread per
// four voxels along the last axis / one thread per voxel of the volume, plain loads and stores, no LDS, no atomics.
#include "infer_math.h"

namespace {

constexpr int WIN_TB = 256;
constexpr int WIN_MAX_BLOCKS = 2048;

inline int win_blocks(long total) { long b = (total + WIN_TB - 1) / WIN_TB; return (int)(b < WIN_MAX_BLOCKS ? b : WIN_MAX_BLOCKS); }

// grid (blocks over the quads of a patch, npatch); vec: pd % 4 == 0 and a 16-byte aligned output
__global__ __launch_bounds__(WIN_TB) void window_gather_kernel(const chap_window_gather_params P, int vec) {
    const int DQ = (P.pd + 3) >> 2;
    const long quads = (long)P.pw * P.ph * DQ;
    const long pvox = (long)P.pw * P.ph * P.pd;
    const int k = blockIdx.y;
    const int ox = P.origins[3 * k] - P.pad_lo[0], oy = P.origins[3 * k + 1] - P.pad_lo[1], oz = P.origins[3 * k + 2] - P.pad_lo[2];
    float* out = P.patches + (long)k * pvox;
    for (long q = (long)blockIdx.x * WIN_TB + threadIdx.x; q < quads; q += (long)gridDim.x * WIN_TB) {
        const int l0 = (int)(q % DQ) << 2;
        const long r = q / DQ;
        const int j = (int)(r % P.ph), i = (int)(r / P.ph);
        const long x = (long)ox + i, y = (long)oy + j;           // 64-bit: any int32 origin is legal
        const bool in_xy = x >= 0 && x < P.W && y >= 0 && y < P.H;
        const int n = min(4, P.pd - l0);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long z = (long)oz + l0 + e;
            v[e] = (e < n && in_xy && z >= 0 && z < P.D) ? P.volume[(x * P.H + y) * P.D + z] : 0.f;
        }
        const long o = ((long)i * P.ph + j) * P.pd + l0;
        if (vec) {
            *(float4*)(out + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int e = 0; e < n; ++e) out[o + e] = v[e];
        }
    }
}

// window_accumulate_kernel (loss.hip) with the value of a patch taken from NH heads.  NH == 1 is that kernel statement for statement.
template <int NH>
__global__ __launch_bounds__(256) void window_accumulate_heads_kernel(const chap_window_acc_heads_params P) {
    const long pvox = (long)P.pw * P.ph * P.pd;
    const long vol = (long)P.W * P.H * P.D;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < vol; i += (long)gridDim.x * 256) {
        const int z = (int)(i % P.D); const long r = i / P.D;
        const int y = (int)(r % P.H); const int x = (int)(r / P.H);
        float acc[INFER_MAXC], cn = 0.f;
        bool touched = false;
        for (int k = 0; k < P.npatch; ++k) {
            const int lx = x - P.origins[3 * k], ly = y - P.origins[3 * k + 1], lz = z - P.origins[3 * k + 2];
            if ((unsigned)lx >= (unsigned)P.pw || (unsigned)ly >= (unsigned)P.ph || (unsigned)lz >= (unsigned)P.pd) continue;
            if (!touched) {
                for (int c = 0; c < P.C; ++c) acc[c] = P.score[c * vol + i];
                cn = P.cnt[i];
                touched = true;
            }
            const long off = (long)k * P.C * pvox + ((long)lx * P.ph + ly) * P.pd + lz;
            const float* lg = P.logits[0] + off;
            float v[INFER_MAXC];
            for (int c = 0; c < P.C; ++c) v[c] = lg[c * pvox];
            softmax_c(v, P.C);
            if (NH == 2) {
                const float* lg2 = P.logits[1] + off;
                float b[INFER_MAXC];
                for (int c = 0; c < P.C; ++c) b[c] = lg2[c * pvox];
                softmax_c(b, P.C);
                for (int c = 0; c < P.C; ++c) v[c] = (v[c] + b[c]) / 2.0f;
            }
            for (int c = 0; c < P.C; ++c) acc[c] += v[c];
            cn += 1.f;
        }
        if (touched) {
            for (int c = 0; c < P.C; ++c) P.score[c * vol + i] = acc[c];
            P.cnt[i] = cn;
        }
    }
}

}  // namespace

extern "C" int chap_window_gather(const chap_window_gather_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->volume && p->origins && p->patches, "chap_window_gather: null argument");
    CHAP_CHECK_ARG(p->npatch >= 1 && p->npatch <= 65535, "chap_window_gather: npatch must be in [1, 65535] (got %d)", p->npatch);
    CHAP_CHECK_ARG(p->W >= 1 && p->H >= 1 && p->D >= 1 && p->pw >= 1 && p->ph >= 1 && p->pd >= 1,
                   "chap_window_gather: empty volume or patch (%d x %d x %d, %d x %d x %d)", p->W, p->H, p->D, p->pw, p->ph, p->pd);
    CHAP_CHECK_ARG(p->pad_lo[0] >= 0 && p->pad_lo[1] >= 0 && p->pad_lo[2] >= 0, "chap_window_gather: negative padding");
    const long quads = (long)p->pw * p->ph * ((p->pd + 3) / 4);
    const int vec = p->pd % 4 == 0 && ((uintptr_t)p->patches & 15) == 0;
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)win_blocks(quads), (unsigned)p->npatch), dim3(WIN_TB), 0, (hipStream_t)stream, *p, vec);
    CHAP_LAUNCH_CHECK("chap_window_gather");
    return CHAP_OK;
}

extern "C" int chap_window_accumulate_heads(const chap_window_acc_heads_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->logits[0] && p->origins && p->score && p->cnt && p->npatch > 0 && p->C >= 1 && p->C <= INFER_MAXC,
                   "chap_window_accumulate_heads: bad argument");
    CHAP_CHECK_ARG(p->nheads == 1 || (p->nheads == 2 && p->logits[1]), "chap_window_accumulate_heads: nheads must be 1 or 2, with as many logits tensors (got %d)", p->nheads);
    CHAP_CHECK_ARG(p->pw > 0 && p->ph > 0 && p->pd > 0 && p->pw <= p->W && p->ph <= p->H && p->pd <= p->D, "chap_window_accumulate_heads: patch larger than the volume");
    const int nb = win_blocks((long)p->W * p->H * p->D);
    if (p->nheads == 1) hipLaunchKernelGGL(window_accumulate_heads_kernel<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(window_accumulate_heads_kernel<2>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_window_accumulate_heads");
    return CHAP_OK;
}
