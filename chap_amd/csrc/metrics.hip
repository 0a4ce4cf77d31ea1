// Segmentation metrics (medpy.metric.binary dc / jc / ravd / hd / hd95 / asd / assd) for K classes of one pair of maps:
// border maps + class counts, exact squared Euclidean distance transform, per-class reductions, HD95 order statistics.
// Contract and layout: include/chap_hip.h (chap_metrics); algorithm and exactness argument: DESIGN.md "Segmentation metrics".
#include <climits>
#include <cmath>
#include "common.h"

namespace {

constexpr int MET_TB = 256;             // threads per block of every kernel here
constexpr int MET_LDS_BUDGET = 40960;   // bytes of one column tile of the brute-force EDT pass: 4 blocks per CU
constexpr int MET_RC_MAX = 8;           // outputs per thread and round of the brute-force pass

__device__ __forceinline__ int64_t met_ld(const void* p, int is64, unsigned i) {
    return is64 ? ((const int64_t*)p)[i] : (int64_t)((const uint8_t*)p)[i];
}

// Class index of voxel i of one map (-1: none) and whether it is a border voxel of that class: some 4- (2D) or 6-neighbour (3D) lies
// outside the array or outside the class (scipy binary_erosion, cross footprint, border_value = 0).
__device__ __forceinline__ int met_border(const void* X, int is64, int binary, const int64_t* cls, int K, unsigned i,
                                          int d, int h, int w, int D, int H, int W, int ndim, bool& border) {
    const int64_t v = met_ld(X, is64, i);
    int k = -1;
    if (binary) k = v != 0 ? 0 : -1;
    else for (int c = 0; c < K; ++c) if (cls[c] == v) { k = c; break; }
    border = false;
    if (k < 0) return k;
    const unsigned HW = (unsigned)H * (unsigned)W;
#define MET_OUT(cond, j) (cond) || (binary ? met_ld(X, is64, (j)) == 0 : met_ld(X, is64, (j)) != v)
    border = MET_OUT(w == 0, i - 1) || MET_OUT(w == W - 1, i + 1) || MET_OUT(h == 0, i - W) || MET_OUT(h == H - 1, i + W);
    if (!border && ndim == 3) border = MET_OUT(d == 0, i - HW) || MET_OUT(d == D - 1, i + HW);
#undef MET_OUT
    return k;
}

// One increment per distinct class of a wave (a leader adds the group's count): a map of one class puts every lane on one LDS word.
__device__ __forceinline__ void met_wave_count(unsigned* cnt, int k) {
    unsigned long long todo = __ballot(k >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lk = __shfl(k, leader, 64);
        const unsigned long long same = __ballot(k == lk) & todo;
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&cnt[lk], (unsigned)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(MET_TB) void met_surface_kernel(const chap_metrics_params P) {
    __shared__ int64_t cls[255];
    __shared__ unsigned cnt[3][255];
    const int K = P.K;
    for (int t = threadIdx.x; t < K; t += MET_TB) {
        cls[t] = P.binary ? 1 : P.classes[t];
        cnt[0][t] = cnt[1][t] = cnt[2][t] = 0;
    }
    __syncthreads();
    const int D = P.D, H = P.H, W = P.W;
    const unsigned HW = (unsigned)H * (unsigned)W, V = HW * (unsigned)D;
    const unsigned span = gridDim.x * MET_TB;
    const unsigned trips = (V + span - 1) / span;          // whole waves go through the loop (ballots)
    for (unsigned q = 0; q < trips; ++q) {
        const unsigned i = q * span + blockIdx.x * MET_TB + threadIdx.x;
        int ka = -1, kb = -1;
        if (i < V) {
            const int w = (int)(i % (unsigned)W), h = (int)((i / (unsigned)W) % (unsigned)H), d = (int)(i / HW);
            bool ba, bb;
            ka = met_border(P.a, P.a_i64, P.binary, cls, K, i, d, h, w, D, H, W, P.ndim, ba);
            kb = met_border(P.b, P.b_i64, P.binary, cls, K, i, d, h, w, D, H, W, P.ndim, bb);
            P.border_a[i] = ba ? (uint8_t)(ka + 1) : (uint8_t)0;
            P.border_b[i] = bb ? (uint8_t)(kb + 1) : (uint8_t)0;
        }
        met_wave_count(cnt[0], ka);
        met_wave_count(cnt[1], kb);
        met_wave_count(cnt[2], ka == kb ? ka : -1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K; t += MET_TB) {         // integer atomics: the totals do not depend on the order
        if (cnt[0][t]) atomicAdd((unsigned long long*)&P.results[t].n_a, (unsigned long long)cnt[0][t]);
        if (cnt[1][t]) atomicAdd((unsigned long long*)&P.results[t].n_b, (unsigned long long)cnt[1][t]);
        if (cnt[2][t]) atomicAdd((unsigned long long*)&P.results[t].n_ab, (unsigned long long)cnt[2][t]);
    }
}

// EDT pass 1, along W: one wave per row of field f = 2k + dir (dir 0: feature = border(B) of class k, dir 1: border(A)).  The nearest
// feature at or left of x is a running max-scan of the feature positions, the one at or right of x a running min-scan from the right
// (the two sweeps, 64 positions per step); the row of distances in between lives in the output itself.  Result (dx * sW)^2, +inf when
// the row holds no feature.
__global__ __launch_bounds__(MET_TB) void met_edt_rows_kernel(const chap_metrics_params P) {
    const int lane = threadIdx.x & 63;
    const int D = P.D, H = P.H, W = P.W;
    const long rows = (long)D * H, V = rows * W;
    const long line = (long)blockIdx.x * (MET_TB / 64) + (threadIdx.x >> 6);
    if (line >= 2L * P.K * rows) return;                  // a whole wave
    const int f = (int)(line / rows);
    const long row = line - (long)f * rows;
    const uint8_t* m = ((f & 1) ? P.border_a : P.border_b) + row * W;
    const uint8_t want = (uint8_t)((f >> 1) + 1);
    double* o = P.dist + (long)f * V + row * W;
    int carry = -1;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        int v = (x < W && m[x] == want) ? x : -1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(v, off, 64); if (lane >= off) v = max(v, t); }
        v = max(v, carry);
        carry = __shfl(v, 63, 64);
        if (x < W) o[x] = v >= 0 ? (double)(x - v) : (double)INFINITY;
    }
    const double s = P.spacing[2];
    carry = INT_MAX;
    for (int x0 = ((W - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
        const int x = x0 + lane;
        int v = (x < W && m[x] == want) ? x : INT_MAX;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_down(v, off, 64); if (lane + off < 64) v = min(v, t); }
        v = min(v, carry);
        carry = __shfl(v, 0, 64);
        if (x < W) {
            double dx = o[x];                               // written by this lane in the first sweep
            if (v != INT_MAX) dx = fmin(dx, (double)(v - x));
            const double g = dx * s;
            o[x] = g * g;
        }
    }
}

// EDT passes 2 and 3, along H or D: f(i) = min_j g(j) + ((i - j) * s)^2 by brute force over a tile of TW neighbouring lines staged in
// LDS ([n][TW] doubles, loaded and stored with TW consecutive doubles per row).  T = 256 / TW threads per line; thread t owns the
// positions t, t + T, t + 2T, ... in rounds of RC, each LDS read of g(j) serving RC candidates.  The minimum of a set of doubles does not
// depend on the order: the result is the same for any launch geometry.
template <int RC, bool UNIT>
__device__ __forceinline__ void met_cols_round(const double* col, int TW, int n, int i0, int T, double s, double (&m)[RC]) {
    double off[RC];
#pragma unroll
    for (int r = 0; r < RC; ++r) { m[r] = INFINITY; off[r] = (double)(T * r); }
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const double g = col[j * TW];
        const double db = (double)(i0 - j);
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const double d = UNIT ? db + off[r] : (db + off[r]) * s;
            m[r] = fmin(m[r], fma(d, d, g));
        }
    }
}

template <int RC>
__global__ __launch_bounds__(MET_TB) void met_edt_cols_kernel(double* __restrict__ dist, int n, long stride, int W, int O1, long ostride,
                                                             long V, int TW, int ntw, double s) {
    extern __shared__ double tile[];
    const int tw = blockIdx.x % ntw;
    const long o = blockIdx.x / ntw;
    double* base = dist + (o / O1) * V + (o % O1) * ostride + (long)tw * TW;
    const int valid = min(TW, W - tw * TW);
    for (int e = threadIdx.x; e < n * TW; e += MET_TB) {
        const int i = e / TW, c = e - i * TW;
        tile[e] = c < valid ? base[i * stride + c] : (double)INFINITY;
    }
    __syncthreads();
    const int c = threadIdx.x % TW, t = threadIdx.x / TW, T = MET_TB / TW;
    if (c >= valid) return;
    const int per = (n + T - 1) / T;
    for (int p0 = 0; p0 < per; p0 += RC) {
        double m[RC];
        const int i0 = t + T * p0;
        if (s == 1.0) met_cols_round<RC, true>(tile + c, TW, n, i0, T, s, m);
        else met_cols_round<RC, false>(tile + c, TW, n, i0, T, s, m);
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const int i = i0 + T * r;
            if (i < n) base[i * stride + c] = m[r];
        }
    }
}

// Fixed-tree block reduction of 256 values (xor butterfly in each wave, then the four waves in a fixed order): bitwise the same
// result on every run.
__device__ __forceinline__ double met_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double met_block_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

struct MetWs {          // views of the workspace (chap_metrics_ws), per class k and direction dir
    long* cnt;          // [K][2][nb] samples per block
    double* sum;        // [K][2][nb] sum of sqrt(d^2) per block
    double* mx;         // [K][2][nb] max d^2 per block
    unsigned* hist;     // [K][2][256] radix histogram of the running pass (lo / hi order statistic)
    uint64_t* prefix;   // [K][2] bits of the order statistic found so far
    long* rank;         // [K][2] rank still to find below the prefix; -1: no sample
    int nb; long chunk;
};

// Samples of class k: sds(A,B) at the border voxels of A (field 2k), sds(B,A) at those of B (field 2k + 1).  Block b reduces the voxel
// range [b * chunk, (b + 1) * chunk) in a fixed order.
__global__ __launch_bounds__(MET_TB) void met_reduce_kernel(const chap_metrics_params P, const MetWs S) {
    __shared__ double red[4];
    const int k = blockIdx.y;
    const uint8_t want = (uint8_t)(k + 1);
    const long V = (long)P.D * P.H * P.W;
    const long i0 = (long)blockIdx.x * S.chunk, i1 = min(V, i0 + S.chunk);
    const double* fab = P.dist + (2L * k) * V;
    const double* fba = fab + V;
    long c0 = 0, c1 = 0;
    double s0 = 0.0, s1 = 0.0, m0 = 0.0, m1 = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += MET_TB) {
        if (P.border_a[i] == want) { const double v = fab[i]; ++c0; s0 += sqrt(v); m0 = fmax(m0, v); }
        if (P.border_b[i] == want) { const double v = fba[i]; ++c1; s1 += sqrt(v); m1 = fmax(m1, v); }
    }
    const double tc0 = met_block_sum((double)c0, red), tc1 = met_block_sum((double)c1, red);     // exact: < 2^53
    const double ts0 = met_block_sum(s0, red), ts1 = met_block_sum(s1, red);
    const double tm0 = met_block_max(m0, red), tm1 = met_block_max(m1, red);
    if (threadIdx.x == 0) {
        const long j0 = ((long)k * 2 + 0) * S.nb + blockIdx.x, j1 = j0 + S.nb;
        S.cnt[j0] = (long)tc0; S.sum[j0] = ts0; S.mx[j0] = tm0;
        S.cnt[j1] = (long)tc1; S.sum[j1] = ts1; S.mx[j1] = tm1;
    }
}

// One block per class: the block partials in a fixed order; the ranks of the two HD95 order statistics over the union of both
// directions, numpy.percentile(..., 95) 'linear': virtual index (n - 1) * 0.95, its floor and the next one (both n - 1 at the top).
__global__ __launch_bounds__(MET_TB) void met_finalize_kernel(const chap_metrics_params P, const MetWs S) {
    __shared__ double red[4];
    const int k = blockIdx.x;
    double c[2], s[2], m[2];
    for (int dir = 0; dir < 2; ++dir) {
        const long j0 = ((long)k * 2 + dir) * S.nb;
        double tc = 0.0, ts = 0.0, tm = 0.0;
        for (int b = threadIdx.x; b < S.nb; b += MET_TB) { tc += (double)S.cnt[j0 + b]; ts += S.sum[j0 + b]; tm = fmax(tm, S.mx[j0 + b]); }
        c[dir] = met_block_sum(tc, red);
        s[dir] = met_block_sum(ts, red);
        m[dir] = met_block_max(tm, red);
    }
    if (threadIdx.x == 0) {
        chap_metric_result& R = P.results[k];
        R.n_ab_s = (int64_t)c[0]; R.n_ba_s = (int64_t)c[1];
        R.sum_ab = s[0]; R.sum_ba = s[1]; R.max2_ab = m[0]; R.max2_ba = m[1];
        const long n = (long)c[0] + (long)c[1];
        long lo = -1, hi = -1;
        if (R.n_a > 0 && R.n_b > 0 && n > 0) {
            const double vi = (double)(n - 1) * 0.95;
            if (vi >= (double)(n - 1)) lo = hi = n - 1;
            else { lo = (long)floor(vi); hi = lo + 1; }
        }
        R.q_lo = lo; R.q_hi = hi;
        R.v2_lo = R.v2_hi = (double)NAN;
        S.prefix[2 * k] = S.prefix[2 * k + 1] = 0;
        S.rank[2 * k] = lo; S.rank[2 * k + 1] = hi;
    }
}

// Radix select of the two order statistics on the bit patterns of the squared distances (non-negative doubles order like their
// uint64 patterns), 8 bits per pass from the top: histogram of the samples that match the prefix found so far (one 256-bin histogram
// per wave and order statistic in LDS, then integer atomics into the class's global histogram), then met_pick_kernel.
__global__ __launch_bounds__(MET_TB) void met_hist_kernel(const chap_metrics_params P, const MetWs S, int shift) {
    __shared__ unsigned wh[MET_TB / 64][2][256];
    const int k = blockIdx.y;
    if (S.rank[2 * k] < 0) return;                          // the whole block: no samples
    for (int e = threadIdx.x; e < (MET_TB / 64) * 2 * 256; e += MET_TB) (&wh[0][0][0])[e] = 0;
    __syncthreads();
    const uint8_t want = (uint8_t)(k + 1);
    const long V = (long)P.D * P.H * P.W;
    const long i0 = (long)blockIdx.x * S.chunk, i1 = min(V, i0 + S.chunk);
    const uint64_t himask = shift >= 56 ? 0ull : ~((1ull << (shift + 8)) - 1ull);
    const uint64_t p0 = S.prefix[2 * k], p1 = S.prefix[2 * k + 1];
    unsigned (*h)[256] = wh[threadIdx.x >> 6];
    const double* f0 = P.dist + (2L * k) * V;
    for (long i = i0 + threadIdx.x; i < i1; i += MET_TB) {
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            if ((dir ? P.border_b : P.border_a)[i] != want) continue;
            const uint64_t u = (uint64_t)__double_as_longlong(f0[dir * V + i]);
            const unsigned bin = (unsigned)(u >> shift) & 255u;
            if ((u & himask) == p0) atomicAdd(&h[0][bin], 1u);
            if ((u & himask) == p1) atomicAdd(&h[1][bin], 1u);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * 256; e += MET_TB) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < MET_TB / 64; ++w) t += (&wh[w][0][0])[e];
        if (t) atomicAdd(&S.hist[(long)k * 512 + e], t);
    }
}

// One block per class: the bin holding each order statistic, the prefix and the rank within the bin; clears the histogram for the
// next pass.  After the last pass (shift 0) the prefixes are the values.
__global__ __launch_bounds__(MET_TB) void met_pick_kernel(const chap_metrics_params P, const MetWs S, int shift) {
    __shared__ unsigned hb[256];
    const int k = blockIdx.x;
    for (int sel = 0; sel < 2; ++sel) {
        const long r = S.rank[2 * k + sel];
        if (r < 0) return;                                  // uniform: both ranks are -1 together
        unsigned* gh = S.hist + (long)k * 512 + sel * 256;
        hb[threadIdx.x] = gh[threadIdx.x];
        gh[threadIdx.x] = 0;
        __syncthreads();
        long below = 0;
        for (int b = 0; b < (int)threadIdx.x; ++b) below += hb[b];
        if (below <= r && r < below + (long)hb[threadIdx.x]) {      // exactly one thread
            S.prefix[2 * k + sel] |= (uint64_t)threadIdx.x << shift;
            S.rank[2 * k + sel] = r - below;
        }
        __syncthreads();
    }
    if (shift == 0 && threadIdx.x == 0) {
        P.results[k].v2_lo = __longlong_as_double((long long)S.prefix[2 * k]);
        P.results[k].v2_hi = __longlong_as_double((long long)S.prefix[2 * k + 1]);
    }
}

int met_nb(long V) {
    long nb = (V + 16383) / 16384;
    return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}

size_t met_align(size_t x) { return (x + 255) & ~(size_t)255; }

MetWs met_ws(const chap_metrics_params* p) {
    MetWs S;
    const long V = (long)p->D * p->H * p->W;
    S.nb = met_nb(V);
    S.chunk = (V + S.nb - 1) / S.nb;
    char* w = (char*)p->ws;
    const size_t part = met_align(sizeof(double) * 2 * (size_t)p->K * S.nb);
    S.cnt = (long*)w; w += part;
    S.sum = (double*)w; w += part;
    S.mx = (double*)w; w += part;
    S.hist = (unsigned*)w; w += met_align(sizeof(unsigned) * 512 * (size_t)p->K);
    S.prefix = (uint64_t*)w; w += met_align(sizeof(uint64_t) * 2 * (size_t)p->K);
    S.rank = (long*)w;
    return S;
}

template <int RC>
void met_launch_cols(dim3 grid, size_t lds, hipStream_t s, double* dist, int n, long stride, int W, int O1, long ostride, long V, int TW, int ntw, double sp) {
    hipLaunchKernelGGL(met_edt_cols_kernel<RC>, grid, dim3(MET_TB), lds, s, dist, n, stride, W, O1, ostride, V, TW, ntw, sp);
}

// One brute-force pass over F fields along an axis of length n (stride between its positions), lines = F * O1 * W.
int met_cols(hipStream_t s, double* dist, int F, int n, long stride, int W, int O1, long ostride, long V, double sp) {
    if (n <= 1) return CHAP_OK;                             // min over the single j = i: g itself
    int TW = 16;
    while (TW > 1 && (long)n * TW * (long)sizeof(double) > MET_LDS_BUDGET) TW >>= 1;
    const int T = MET_TB / TW, per = (n + T - 1) / T;
    const int rounds = (per + MET_RC_MAX - 1) / MET_RC_MAX, rc = (per + rounds - 1) / rounds;
    const int ntw = (W + TW - 1) / TW;
    const dim3 grid((unsigned)((long)F * O1 * ntw));
    const size_t lds = (size_t)n * TW * sizeof(double);
    switch (rc) {
#define MET_RC(R) case R: met_launch_cols<R>(grid, lds, s, dist, n, stride, W, O1, ostride, V, TW, ntw, sp); break;
        MET_RC(1) MET_RC(2) MET_RC(3) MET_RC(4) MET_RC(5) MET_RC(6) MET_RC(7) MET_RC(8)
#undef MET_RC
        default: chap_set_error("chap_metrics: internal error (rc %d)", rc); return CHAP_EINVAL;
    }
    void* const stream = (void*)s;                          // the lab build's end-of-launch marker names it (common.h, CHAP_TL_MARK)
    (void)stream;
    CHAP_LAUNCH_CHECK("chap_metrics(edt)");
    return CHAP_OK;
}

int met_check(const chap_metrics_params* p) {
    CHAP_CHECK_ARG(p && p->a && p->b && p->border_a && p->border_b && p->results, "chap_metrics: null argument");
    CHAP_CHECK_ARG(p->K >= 1 && p->K <= 255, "chap_metrics: K must be in [1, 255] (got %d)", p ? p->K : 0);
    CHAP_CHECK_ARG(p->binary ? p->K == 1 : p->classes != nullptr, "chap_metrics: binary needs K == 1, class mode a class list");
    CHAP_CHECK_ARG(p->ndim == 3 || (p->ndim == 2 && p->D == 1), "chap_metrics: ndim must be 3, or 2 with D == 1");
    CHAP_CHECK_ARG(p->D >= 1 && p->H >= 1 && p->W >= 1, "chap_metrics: empty shape");
    CHAP_CHECK_ARG(p->D <= CHAP_METRICS_MAX_AXIS && p->H <= CHAP_METRICS_MAX_AXIS && p->W <= CHAP_METRICS_MAX_AXIS,
                   "chap_metrics: axis longer than CHAP_METRICS_MAX_AXIS (%d): D=%d H=%d W=%d", CHAP_METRICS_MAX_AXIS, p->D, p->H, p->W);
    CHAP_CHECK_ARG((long)p->D * p->H * p->W < (1L << 31), "chap_metrics: more than 2^31 - 1 voxels");
    CHAP_CHECK_ARG(p->a_i64 == 0 || p->a_i64 == 1, "chap_metrics: a_i64 must be 0 or 1");
    CHAP_CHECK_ARG(p->b_i64 == 0 || p->b_i64 == 1, "chap_metrics: b_i64 must be 0 or 1");
    if (p->distances) {
        CHAP_CHECK_ARG(p->dist && p->ws, "chap_metrics: distances need dist and ws");
        for (int a = 0; a < 3; ++a)
            CHAP_CHECK_ARG(std::isfinite(p->spacing[a]) && p->spacing[a] > 0.0, "chap_metrics: spacing[%d] must be positive and finite", a);
    }
    return CHAP_OK;
}

}  // namespace

extern "C" size_t chap_metrics_ws(const chap_metrics_params* p) {
    if (!p || p->K < 1) return 0;
    const long V = (long)p->D * p->H * p->W;
    const int nb = met_nb(V);
    return 3 * met_align(sizeof(double) * 2 * (size_t)p->K * nb) + met_align(sizeof(unsigned) * 512 * (size_t)p->K)
         + met_align(sizeof(uint64_t) * 2 * (size_t)p->K) + met_align(sizeof(long) * 2 * (size_t)p->K);
}

extern "C" int chap_metrics(const chap_metrics_params* p, void* stream) {
    const int rc = met_check(p);
    if (rc != CHAP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int K = p->K, D = p->D, H = p->H, W = p->W;
    const long V = (long)D * H * W;
    if (hipMemsetAsync(p->results, 0, sizeof(chap_metric_result) * K, s) != hipSuccess) {
        chap_set_error("chap_metrics: hipMemsetAsync failed");
        return CHAP_ELAUNCH;
    }
    hipLaunchKernelGGL(met_surface_kernel, dim3(chap_blocks(V, 2048)), dim3(MET_TB), 0, s, *p);
    CHAP_LAUNCH_CHECK("chap_metrics(surface)");
    if (!p->distances) return CHAP_OK;
    const MetWs S = met_ws(p);
    if (hipMemsetAsync(S.hist, 0, sizeof(unsigned) * 512 * K, s) != hipSuccess) {
        chap_set_error("chap_metrics: hipMemsetAsync failed");
        return CHAP_ELAUNCH;
    }
    const long rows = 2L * K * D * H;
    hipLaunchKernelGGL(met_edt_rows_kernel, dim3((unsigned)((rows + MET_TB / 64 - 1) / (MET_TB / 64))), dim3(MET_TB), 0, s, *p);
    CHAP_LAUNCH_CHECK("chap_metrics(edt rows)");
    int e = met_cols(s, p->dist, 2 * K, H, W, W, D, (long)H * W, V, p->spacing[1]);           // along H: lines (field, d, w)
    if (e != CHAP_OK) return e;
    if (p->ndim == 3) {
        e = met_cols(s, p->dist, 2 * K, D, (long)H * W, W, H, W, V, p->spacing[0]);           // along D: lines (field, h, w)
        if (e != CHAP_OK) return e;
    }
    hipLaunchKernelGGL(met_reduce_kernel, dim3(S.nb, K), dim3(MET_TB), 0, s, *p, S);
    hipLaunchKernelGGL(met_finalize_kernel, dim3(K), dim3(MET_TB), 0, s, *p, S);
    CHAP_LAUNCH_CHECK("chap_metrics(reduce)");
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(met_hist_kernel, dim3(S.nb, K), dim3(MET_TB), 0, s, *p, S, shift);
        hipLaunchKernelGGL(met_pick_kernel, dim3(K), dim3(MET_TB), 0, s, *p, S, shift);
    }
    CHAP_LAUNCH_CHECK("chap_metrics(select)");
    return CHAP_OK;
}
