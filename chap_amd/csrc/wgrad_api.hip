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
// The kernel is nothing but latency, so (as act_bwd_sum_kernel, pointwise.hip): the arguments are read once; the element's (tap, kc, kn0) is
// decoded and the four prior dw / db values its g == 0 thread adds to are requested IN FRONT of the slab loop, next to the first slabs, not
// behind the barrier where they were one more dependent memory round trip.  A prior that is not to be written (kn >= kn_valid, kc >= kc_valid)
// is requested at the first valid one's address -- in bounds, never used.
struct wgrad_reduce_args { const float* ws; const float* ws_db; int nsplit, taps, Ca, Cb; float* dw; long s_tap, s_kc, s_kn; int kc_valid, kn_valid; float* db; int nb_dw; };
template <int E4>
__device__ __forceinline__ void wgrad_reduce_kernel(const wgrad_reduce_args& Ak) {
    const wgrad_reduce_args A = chap_args_once(Ak);
    const int bid = (int)blockIdx.x;
    const int nsplit = A.nsplit, Ca = A.Ca, Cb = A.Cb, kc_valid = A.kc_valid, kn_valid = A.kn_valid, nb_dw = A.nb_dw;
    constexpr int G = 256 / E4;
    __shared__ float4 red[G][E4];
    const int col = threadIdx.x % E4, g = threadIdx.x / E4;
    const bool is_db = bid >= nb_dw;                             // bias gradient: Cb values x nsplit partials, same scheme
    const long total = is_db ? (long)Cb : (long)A.taps * Ca * Cb;
    const long i = ((long)(is_db ? bid - nb_dw : bid) * E4 + col) * 4;
    // where the total goes: 4 consecutive kn of one (tap, kc) (Cb % 4 == 0); 32-bit division unless the weight has 2^32 elements (wave-uniform)
    int kn0, kc, tap;
    if (total < (1l << 32)) {
        const u32 ui = (u32)i, r = ui / (u32)Cb;
        kn0 = (int)(ui % (u32)Cb); kc = (int)(r % (u32)Ca); tap = (int)(r / (u32)Ca);
    } else {
        const long r = i / Cb;
        kn0 = (int)(i % Cb); kc = (int)(r % Ca); tap = (int)(r / Ca);
    }
    const bool writer = g == 0 && i < total && (is_db || kc < kc_valid) && kn0 < kn_valid;
    CHAP_GLOBAL float* const o = is_db ? (CHAP_GLOBAL float*)A.db + kn0 : (CHAP_GLOBAL float*)A.dw + tap * A.s_tap + kc * A.s_kc + kn0 * A.s_kn;
    const long s_o = is_db ? 1 : A.s_kn;
    float prior[4] = {0.f, 0.f, 0.f, 0.f};
    if (writer) {
#pragma unroll
        for (int j = 0; j < 4; ++j) prior[j] = o[(kn0 + j < kn_valid ? j : 0) * s_o];
    }
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
    if (i < total) {
        const CHAP_GLOBAL float* src = (const CHAP_GLOBAL float*)(is_db ? A.ws_db : A.ws) + i;
        typedef const CHAP_GLOBAL f32x4n* f4p;
        int k = g;
        for (; k + 3 * G < nsplit; k += 4 * G) {
            const f32x4n a = *(f4p)(src + (long)k * total), b = *(f4p)(src + (long)(k + G) * total);
            const f32x4n c = *(f4p)(src + (long)(k + 2 * G) * total), d = *(f4p)(src + (long)(k + 3 * G) * total);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;  s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
            s2.x += c.x; s2.y += c.y; s2.z += c.z; s2.w += c.w;  s3.x += d.x; s3.y += d.y; s3.z += d.z; s3.w += d.w;
        }
        for (; k < nsplit; k += G) { const f32x4n a = *(f4p)(src + (long)k * total); s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w; }
    }
    red[g][col] = make_float4((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y), (s0.z + s1.z) + (s2.z + s3.z), (s0.w + s1.w) + (s2.w + s3.w));
    __syncthreads();
    if (writer) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < G; ++k) { const float4 a = red[k][col]; t[0] += a.x; t[1] += a.y; t[2] += a.z; t[3] += a.w; }
#pragma unroll
        for (int j = 0; j < 4; ++j) if (kn0 + j < kn_valid) o[j * s_o] = prior[j] + t[j];
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
