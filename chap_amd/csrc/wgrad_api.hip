// chap_wgrad: make the plan (wgrad_plan.h: split selection, workspace sizing), launch, deterministic slab reduction.
#include "launchers.h"
#include "launch.h"

extern "C" size_t chap_wgrad_ws(const chap_wgrad_params* p) {
    wg_plan q;
    if (!p || wg_make_plan(p, &q)) return 0;
    return q.bytes;
}

// Deterministic slab reduction.  A block owns E4*4 consecutive elements (one float4 per thread column) and
// splits the slabs over G = 256/E4 thread groups: group g sums slabs g, g+G, ... with 4 loads in flight, the G
// partials are combined in a fixed order through LDS.  E4 = 64 (1 KB contiguous per wave-load, G = 4) for the
// few-slab / large-weight layers, E4 = 8 (G = 32) when there are many slabs of a small weight.
// Fixed summation order -> bitwise reproducible.  total % 4 == 0 (Cb is a multiple of 16).
// Blocks [0, nb_dw) reduce dW, blocks [nb_dw, ...) reduce the bias-gradient partials the same way.
struct wgrad_reduce_args { const float* ws; const float* ws_db; int nsplit, taps, Ca, Cb; float* dw; long s_tap, s_kc, s_kn; int kc_valid, kn_valid; float* db; int nb_dw; };
template <int E4>
__device__ __forceinline__ void wgrad_reduce_kernel(const wgrad_reduce_args& A) {
    const int bid = (int)blockIdx.x;
    const float* __restrict__ ws = A.ws; const float* __restrict__ ws_db = A.ws_db;
    const int nsplit = A.nsplit, taps = A.taps, Ca = A.Ca, Cb = A.Cb, kc_valid = A.kc_valid, kn_valid = A.kn_valid, nb_dw = A.nb_dw;
    float* dw = A.dw; float* db = A.db;
    const long s_tap = A.s_tap, s_kc = A.s_kc, s_kn = A.s_kn;
    constexpr int G = 256 / E4;
    __shared__ float4 red[G][E4];
    const int col = threadIdx.x % E4, g = threadIdx.x / E4;
    const bool is_db = bid >= nb_dw;                             // bias gradient: Cb values x nsplit partials, same scheme
    const long total = is_db ? (long)Cb : (long)taps * Ca * Cb;
    const long i = ((long)(is_db ? bid - nb_dw : bid) * E4 + col) * 4;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
    if (i < total) {
        const float* src = (is_db ? ws_db : ws) + i;
        int k = g;
        for (; k + 3 * G < nsplit; k += 4 * G) {
            const float4 a = *(const float4*)(src + (long)k * total), b = *(const float4*)(src + (long)(k + G) * total);
            const float4 c = *(const float4*)(src + (long)(k + 2 * G) * total), d = *(const float4*)(src + (long)(k + 3 * G) * total);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;  s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
            s2.x += c.x; s2.y += c.y; s2.z += c.z; s2.w += c.w;  s3.x += d.x; s3.y += d.y; s3.z += d.z; s3.w += d.w;
        }
        for (; k < nsplit; k += G) { const float4 a = *(const float4*)(src + (long)k * total); s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w; }
    }
    red[g][col] = make_float4((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y), (s0.z + s1.z) + (s2.z + s3.z), (s0.w + s1.w) + (s2.w + s3.w));
    __syncthreads();
    if (g == 0 && i < total) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < G; ++k) { const float4 a = red[k][col]; t[0] += a.x; t[1] += a.y; t[2] += a.z; t[3] += a.w; }
        const int kn0 = (int)(i % Cb); const long r = i / Cb;            // 4 consecutive kn of one (tap, kc): Cb % 4 == 0
        const int kc = (int)(r % Ca); const int tap = (int)(r / Ca);
        if (is_db) {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (kn0 + j < kn_valid) db[kn0 + j] += t[j];
        } else if (kc < kc_valid) {
            float* o = dw + tap * s_tap + kc * s_kc;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (kn0 + j < kn_valid) o[(kn0 + j) * s_kn] += t[j];
        }
    }
}

extern "C" int chap_wgrad(const chap_wgrad_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->dw && p->ws && p->b.ptr && p->a[0].ptr, "chap_wgrad: null argument");
    wg_plan q;
    int r = wg_make_plan(p, &q);
    if (r) return r;
    CHAP_CHECK_ARG(p->ws_bytes >= q.bytes, "chap_wgrad: workspace %zu < %zu bytes", p->ws_bytes, q.bytes);
    const int sd = p->dims == 3 ? p->stride : 1;
    CHAP_CHECK_ARG(p->ID == (p->stride == 1 ? p->D : p->D * sd) && p->IH == p->H * p->stride && p->IW == p->W * p->stride,
                   "chap_wgrad: A dims (%d,%d,%d) do not match grid (%d,%d,%d) stride %d", p->ID, p->IH, p->IW, p->D, p->H, p->W, p->stride);
    if (p->dims == 3 && (p->a[0].keep || (p->na > 1 && p->a[1].keep))) { chap_set_error("chap_wgrad: element keep masks on the A operand are built for 2D only"); return CHAP_EUNSUPPORTED; }
    float* ws = (float*)p->ws;
    float* ws_db = p->db ? ws + (size_t)q.nsplit * (q.slab / sizeof(float)) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (p->dtype == CHAP_BF16) r = chap_wgrad_launch_bf16(p, q, ws, ws_db, s);
    else if (p->dtype == CHAP_F32) r = chap_wgrad_launch_f32(p, q, ws, ws_db, s);
    else { chap_set_error("chap_wgrad: dtype=%d", p->dtype); return CHAP_EINVAL; }
    if (r) return r;
    const long total = (long)q.taps * q.Ca * q.Cb;
    const int kcv = p->kc_valid > 0 ? p->kc_valid : q.Ca, knv = p->kn_valid > 0 ? p->kn_valid : q.Cb;
    wgrad_reduce_args ra = {(const float*)ws, (const float*)ws_db, q.nsplit, q.taps, q.Ca, q.Cb, p->dw, (long)p->s_tap, (long)p->s_kc, (long)p->s_kn, kcv, knv, p->db, 0};
    const int e4 = q.nsplit >= 64 ? 8 : 64;      // (8 elements per block / 128 slab groups for the 768-split layers measured 25 us against 7 us: too few loads in flight per thread)
    const int nb_db = p->db ? cdiv(q.Cb, 4 * e4) : 0;
    ra.nb_dw = cdiv(total, 4 * e4);
    if (e4 == 8) return chap_launch<wgrad_reduce_args, wgrad_reduce_kernel<8>, 256>(dim3(ra.nb_dw + nb_db), dim3(256), 0, s, ra, "chap_wgrad(reduce)");
    return chap_launch<wgrad_reduce_args, wgrad_reduce_kernel<64>, 256>(dim3(ra.nb_dw + nb_db), dim3(256), 0, s, ra, "chap_wgrad(reduce)");
}
