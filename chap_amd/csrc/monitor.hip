// Training monitor (include/chap_hip_monitor.h): pseudo-label quality of an iteration as counts, from inside the iteration's streams.
// Two streaming passes (logits / label maps) leave one partial row per block -- int64 counts, fp64 confidence sums, no float atomics --
// and a one-block kernel sums the rows in a fixed order and writes one row of a ring the host reads whenever it likes.
// HBM-bound: every logit and label is read once, 16 bytes per load where the shape allows.
#include "common.h"
#include "chap_hip_monitor.h"

namespace {

typedef long long i64;
typedef unsigned long long u64;
typedef i64 i64x2n __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {      // xor butterfly: the same pairing on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rows a group of `units` work items (pixels, or groups of four) leaves: one per block, 0 for an empty group
__host__ __device__ inline int mon_slots(long units) { const long b = (units + 255) / 256; return (int)(b < CHAP_MONITOR_SLOTS ? b : CHAP_MONITOR_SLOTS); }

// chap_pseudo_block's arg-max (loss.hip: softmax_px, then the first maximum of p) and max soft-max.  p[a] = expf(z[a] - m) * inv with
// expf(z[a] - m) == 1 for the class that wins (or ties) the comparison of p, so the confidence is inv itself.
template <int C>
__device__ __forceinline__ void head_px(const float z[C], int& a, float& conf) {
    float m = -INFINITY, p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - m); s += p[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    a = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) if (p[c] > p[a]) a = c;
    conf = inv;
}

// a label as a class index, -1 outside [0, C): equal to no arg-max, member of no gt[c]
template <int C> __device__ __forceinline__ int class_of(i64 l) { return (l >= 0 && l < C) ? (int)l : -1; }

template <int C>
struct LogitsAcc {
    u32 n = 0, ndis = 0, gt[C], ncor[2] = {0, 0}, inter[2][C], pred[2][C];
    double cc[2] = {0.0, 0.0}, ce[2] = {0.0, 0.0};
    __device__ __forceinline__ LogitsAcc() {
#pragma unroll
        for (int c = 0; c < C; ++c) { gt[c] = 0; inter[0][c] = inter[1][c] = 0; pred[0][c] = pred[1][c] = 0; }
    }
    __device__ __forceinline__ void add(const int a[2], const float conf[2], int lab) {
        n += 1;
        ndis += (a[0] != a[1]);
#pragma unroll
        for (int c = 0; c < C; ++c) gt[c] += (lab == c);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool ok = a[h] == lab;
            ncor[h] += ok;
            const double v = (double)conf[h];
            cc[h] += ok ? v : 0.0;
            ce[h] += ok ? 0.0 : v;
#pragma unroll
            for (int c = 0; c < C; ++c) { pred[h][c] += (a[h] == c); inter[h][c] += (ok && a[h] == c); }
        }
    }
};

// this block's row: wave sums first, then the four waves' sums through LDS in a fixed order
template <int NW>
__device__ __forceinline__ void store_row(u64 (*red)[NW], i64* row, int conf_lo, int conf_hi) {
    __syncthreads();
    for (int i = threadIdx.x; i < NW; i += 256) {
        if (i >= conf_lo && i < conf_hi) {
            const double t = (__longlong_as_double((i64)red[0][i]) + __longlong_as_double((i64)red[1][i])) +
                             (__longlong_as_double((i64)red[2][i]) + __longlong_as_double((i64)red[3][i]));
            row[i] = __double_as_longlong(t);
        } else {
            row[i] = (i64)((red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void monitor_acc_kernel(const chap_monitor_params P_) {
    constexpr int GA = CHAP_MONITOR_GROUP_WORDS(C);
    __shared__ u64 red[4][GA];
    const int g = blockIdx.y;
    const long P = P_.P;
    const long s0 = g ? P_.n_first : 0, s1 = g ? P_.N : P_.n_first;
    const long total = (s1 - s0) * P;
    const bool quads = (P & 3) == 0 && (((uintptr_t)P_.logits[0] | (uintptr_t)P_.logits[1] | (uintptr_t)P_.labels) & 15) == 0;
    const int nb = mon_slots(quads ? total >> 2 : total);
    i64* ws = (i64*)P_.ws;
    if (blockIdx.x == 0 && threadIdx.x == 0) ws[g] = nb;
    if ((int)blockIdx.x >= nb) return;
    LogitsAcc<C> A;
    if (quads) {
        // four consecutive pixels of one sample per thread: one 16-byte load per class plane and head, two for the labels
        const long totalq = total >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < totalq; q += (long)nb * 256) {
            const long i = q << 2;
            const long n = s0 + (u32)i / (u32)P, pp = (u32)i % (u32)P, base = n * C * P + pp;
            const i64x2n l01 = *(const i64x2n*)(P_.labels + n * P + pp), l23 = *(const i64x2n*)(P_.labels + n * P + pp + 2);
            const int lab[4] = {class_of<C>(l01.x), class_of<C>(l01.y), class_of<C>(l23.x), class_of<C>(l23.y)};
            int a[4][2];
            float conf[4][2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float z[4][C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float4 v = *(const float4*)(P_.logits[h] + base + c * P);
                    z[0][c] = v.x; z[1][c] = v.y; z[2][c] = v.z; z[3][c] = v.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) head_px<C>(z[e], a[e][h], conf[e][h]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) A.add(a[e], conf[e], lab[e]);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)nb * 256) {
            const long n = s0 + (u32)i / (u32)P, pp = (u32)i % (u32)P, base = n * C * P + pp;
            int a[2];
            float conf[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float z[C];
#pragma unroll
                for (int c = 0; c < C; ++c) z[c] = P_.logits[h][base + c * P];
                head_px<C>(z, a[h], conf[h]);
            }
            A.add(a, conf, class_of<C>(P_.labels[n * P + pp]));
        }
    }
    // the row, in the order of chap_hip_monitor.h: n | n_disagree | gt[C] | n_correct[2] | conf_correct[2] | conf_err[2] | inter[2][C] | pred[2][C]
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
    u32 v;
    v = wave_sum_u32(A.n); if (lead) red[wave][0] = v;
    v = wave_sum_u32(A.ndis); if (lead) red[wave][1] = v;
#pragma unroll
    for (int c = 0; c < C; ++c) { v = wave_sum_u32(A.gt[c]); if (lead) red[wave][2 + c] = v; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        v = wave_sum_u32(A.ncor[h]); if (lead) red[wave][2 + C + h] = v;
        double d = wave_sum_f64(A.cc[h]); if (lead) red[wave][4 + C + h] = (u64)__double_as_longlong(d);
        d = wave_sum_f64(A.ce[h]); if (lead) red[wave][6 + C + h] = (u64)__double_as_longlong(d);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            v = wave_sum_u32(A.inter[h][c]); if (lead) red[wave][8 + C + h * C + c] = v;
            v = wave_sum_u32(A.pred[h][c]); if (lead) red[wave][8 + 3 * C + h * C + c] = v;
        }
    }
    store_row<GA>(red, ws + CHAP_MONITOR_HDR + ((long)g * CHAP_MONITOR_SLOTS + blockIdx.x) * GA, 4 + C, 8 + C);
}

template <int C>
__global__ __launch_bounds__(256) void monitor_labels_kernel(const chap_monitor_labels_params P_) {
    constexpr int GL = CHAP_MONITOR_LABEL_WORDS(C);
    __shared__ u64 red[4][GL];
    const int g = blockIdx.y;
    const long P = P_.P;
    const long s0 = g ? P_.n_first : 0, s1 = g ? P_.N : P_.n_first;
    const long total = (s1 - s0) * P, off = s0 * P;
    const bool pairs = (P & 1) == 0 && (((uintptr_t)P_.maps[0] | (uintptr_t)P_.maps[1] | (uintptr_t)P_.labels) & 15) == 0;
    const int nb = mon_slots(pairs ? total >> 1 : total);
    i64* ws = (i64*)P_.ws + CHAP_MONITOR_LABEL_REGION(C);
    if (blockIdx.x == 0 && threadIdx.x == 0) ws[g] = nb;
    if ((int)blockIdx.x >= nb) return;
    u32 inter[2][C], pred[2][C];
#pragma unroll
    for (int c = 0; c < C; ++c) { inter[0][c] = inter[1][c] = 0; pred[0][c] = pred[1][c] = 0; }
    auto add = [&](i64 m0, i64 m1, i64 l) {
        const int lab = class_of<C>(l), a[2] = {class_of<C>(m0), class_of<C>(m1)};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < C; ++c) { pred[h][c] += (a[h] == c); inter[h][c] += (a[h] == c && lab == c); }
    };
    if (pairs) {    // int64 maps: a 16-byte load is two pixels
        const long totalp = total >> 1;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < totalp; q += (long)nb * 256) {
            const long i = off + (q << 1);
            const i64x2n m0 = *(const i64x2n*)(P_.maps[0] + i), m1 = *(const i64x2n*)(P_.maps[1] + i), l = *(const i64x2n*)(P_.labels + i);
            add(m0.x, m1.x, l.x);
            add(m0.y, m1.y, l.y);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)nb * 256) add(P_.maps[0][off + i], P_.maps[1][off + i], P_.labels[off + i]);
    }
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            u32 v = wave_sum_u32(inter[h][c]); if (lead) red[wave][h * C + c] = v;
            v = wave_sum_u32(pred[h][c]); if (lead) red[wave][2 * C + h * C + c] = v;
        }
    store_row<GL>(red, ws + CHAP_MONITOR_HDR + ((long)g * CHAP_MONITOR_SLOTS + blockIdx.x) * GL, 0, 0);
}

// One block.  The summation discipline of mix_loss_final_kernel -- fixed order, fp64 -- for up to 160 columns of up to 512 rows: the block's
// 1024 threads are `np` parts per column; part q adds the rows q, q + np, ... of its column in that order (sixteen loads in flight at a
// time: one thread per column alone took 56 us, a chain of dependent round trips), and the column's parts are then added in the order
// 0 .. np - 1.  np depends on C alone, so the order is the same on every run.  Counts are summed as int64, exactly.
constexpr int FIN_THREADS = 1024, FIN_BATCH = 16;
__global__ __launch_bounds__(FIN_THREADS) void monitor_final_kernel(const chap_monitor_finalize_params P_) {
    __shared__ u64 part[FIN_THREADS];
    const int C = P_.C, GA = CHAP_MONITOR_GROUP_WORDS(C), GL = CHAP_MONITOR_LABEL_WORDS(C), W = CHAP_MONITOR_ROW_WORDS(C);
    const int ncol = 2 * GA + 2 * GL, np = FIN_THREADS / ncol;
    const i64* wsA = (const i64*)P_.ws;
    const i64* wsL = wsA + CHAP_MONITOR_LABEL_REGION(C);
    const int slot = P_.slot_iter[0], iter = P_.slot_iter[1];
    double* out = P_.ring + (long)((u32)slot % (u32)P_.ring_rows) * W;
    const int t = threadIdx.x, col_i = t % ncol, q = t / ncol;
    const bool lab = col_i >= 2 * GA;
    const int u = lab ? col_i - 2 * GA : col_i, gw = lab ? GL : GA;
    const int g = u / gw, j = u % gw;
    const bool conf = !lab && j >= 4 + C && j < 8 + C;
    if (q < np) {
        const i64* reg = lab ? wsL : wsA;
        int nrows = 0;
        if (!lab || P_.has_labels) {
            const i64 hdr = reg[g];
            nrows = hdr < 0 ? 0 : hdr > CHAP_MONITOR_SLOTS ? CHAP_MONITOR_SLOTS : (int)hdr;      // (a region no launch has written: stay inside it)
        }
        const i64* col = reg + CHAP_MONITOR_HDR + (long)g * CHAP_MONITOR_SLOTS * gw + j;
        double sd = 0.0;
        i64 si = 0;
        for (int r0 = q; r0 < nrows; r0 += np * FIN_BATCH) {
            i64 v[FIN_BATCH];
#pragma unroll
            for (int k = 0; k < FIN_BATCH; ++k) { const int r = r0 + k * np; v[k] = r < nrows ? col[(long)r * gw] : 0; }       // (+0.0 and 0 for the rows past the end)
#pragma unroll
            for (int k = 0; k < FIN_BATCH; ++k) { sd += __longlong_as_double(v[k]); si += v[k]; }
        }
        part[q * ncol + col_i] = conf ? (u64)__double_as_longlong(sd) : (u64)si;
    }
    __syncthreads();
    if (t == 0) out[0] = (double)iter;
    if (t < ncol) {         // (q == 0: this thread's own decoding of the column holds)
        double tot;
        if (conf) {
            tot = 0.0;
            for (int k = 0; k < np; ++k) tot += __longlong_as_double((i64)part[k * ncol + t]);
        } else {
            i64 s = 0;
            for (int k = 0; k < np; ++k) s += (i64)part[k * ncol + t];
            tot = (double)s;
        }
        out[1 + t] = tot;
    }
    if (t < CHAP_MONITOR_MAX_SCALARS) out[1 + ncol + t] = t < P_.nscalars ? (double)*P_.scalars[t] : 0.0;
}

constexpr int MON_MINC = 2, MON_MAXC = 8;
#define MON_LAUNCH(KERNEL, C_, GRID, STREAM, ...)                                                                       \
    switch (C_) {                                                                                                       \
        case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        case 5: hipLaunchKernelGGL(KERNEL<5>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        case 6: hipLaunchKernelGGL(KERNEL<6>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        case 7: hipLaunchKernelGGL(KERNEL<7>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        case 8: hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(256), 0, STREAM, __VA_ARGS__); break;                          \
        default: break; /* refused by the entry's argument check */                                                     \
    }
#define MON_CHECK_C(WHO, C_) CHAP_CHECK_ARG((C_) >= MON_MINC && (C_) <= MON_MAXC, WHO ": C=%d (2..8 built)", C_)

// grid.x: the larger group's row count, `per_thread` pixels to a work item (the kernel derives the same figure from the same arguments)
inline dim3 mon_grid(int N, int n_first, long P, int per_thread) {
    const long big = (long)(n_first > N - n_first ? n_first : N - n_first) * P;
    return dim3(mon_slots(big / per_thread), 2);
}
inline bool aligned16(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }

}  // namespace

extern "C" int chap_monitor_accumulate(const chap_monitor_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->logits[0] && p->logits[1] && p->labels && p->ws, "chap_monitor_accumulate: null argument");
    MON_CHECK_C("chap_monitor_accumulate", p->C);
    CHAP_CHECK_ARG(p->N > 0 && p->P > 0 && p->n_first >= 0 && p->n_first <= p->N, "chap_monitor_accumulate: bad shape (N=%d P=%d n_first=%d)", p->N, p->P, p->n_first);
    CHAP_CHECK_ARG((long)p->N * p->P < (1L << 32), "chap_monitor_accumulate: N*P=%ld exceeds the 32-bit pixel index", (long)p->N * p->P);
    CHAP_CHECK_ARG((((uintptr_t)p->logits[0] | (uintptr_t)p->logits[1]) & 3) == 0 && (((uintptr_t)p->labels | (uintptr_t)p->ws) & 7) == 0,
                   "chap_monitor_accumulate: logits must be 4-byte, labels and ws 8-byte aligned");
    const bool quads = (p->P & 3) == 0 && aligned16(p->logits[0], p->logits[1], p->labels);       // monitor_acc_kernel's own test
    MON_LAUNCH(monitor_acc_kernel, p->C, mon_grid(p->N, p->n_first, p->P, quads ? 4 : 1), (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_monitor_accumulate");
    return CHAP_OK;
}

extern "C" int chap_monitor_accumulate_labels(const chap_monitor_labels_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->maps[0] && p->maps[1] && p->labels && p->ws, "chap_monitor_accumulate_labels: null argument");
    MON_CHECK_C("chap_monitor_accumulate_labels", p->C);
    CHAP_CHECK_ARG(p->N > 0 && p->P > 0 && p->n_first >= 0 && p->n_first <= p->N, "chap_monitor_accumulate_labels: bad shape (N=%d P=%d n_first=%d)", p->N, p->P, p->n_first);
    CHAP_CHECK_ARG((long)p->N * p->P < (1L << 32), "chap_monitor_accumulate_labels: N*P=%ld exceeds the 32-bit pixel index", (long)p->N * p->P);
    CHAP_CHECK_ARG((((uintptr_t)p->maps[0] | (uintptr_t)p->maps[1] | (uintptr_t)p->labels | (uintptr_t)p->ws) & 7) == 0,
                   "chap_monitor_accumulate_labels: maps, labels and ws must be 8-byte aligned");
    const bool pairs = (p->P & 1) == 0 && aligned16(p->maps[0], p->maps[1], p->labels);           // monitor_labels_kernel's own test
    MON_LAUNCH(monitor_labels_kernel, p->C, mon_grid(p->N, p->n_first, p->P, pairs ? 2 : 1), (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_monitor_accumulate_labels");
    return CHAP_OK;
}

extern "C" int chap_monitor_finalize(const chap_monitor_finalize_params* p, void* stream) {
    CHAP_CHECK_ARG(p && p->ws && p->ring && p->slot_iter, "chap_monitor_finalize: null argument");
    MON_CHECK_C("chap_monitor_finalize", p->C);
    CHAP_CHECK_ARG(p->ring_rows > 0 && p->nscalars >= 0 && p->nscalars <= CHAP_MONITOR_MAX_SCALARS, "chap_monitor_finalize: bad argument (ring_rows=%d nscalars=%d)",
                   p->ring_rows, p->nscalars);
    for (int k = 0; k < p->nscalars; ++k) CHAP_CHECK_ARG(p->scalars[k], "chap_monitor_finalize: null scalar %d", k);
    uintptr_t al = 0;
    for (int k = 0; k < p->nscalars; ++k) al |= (uintptr_t)p->scalars[k];
    CHAP_CHECK_ARG((((uintptr_t)p->ws | (uintptr_t)p->ring) & 7) == 0 && (((uintptr_t)p->slot_iter | al) & 3) == 0,
                   "chap_monitor_finalize: ws and ring must be 8-byte, slot_iter and scalars 4-byte aligned");
    hipLaunchKernelGGL(monitor_final_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, *p);
    CHAP_LAUNCH_CHECK("chap_monitor_finalize");
    return CHAP_OK;
}
