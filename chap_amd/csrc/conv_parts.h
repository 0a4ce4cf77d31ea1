// Conventions that are contracts BETWEEN the kernels of the MFMA convolution family (conv_fwd_kernel, conv_kpar_kernel, conv_kpar2d_kernel,
// conv_wp_kernel, conv_c1_mfma_kernel, wgrad_kernel, wgrad_wp_kernel), each written once.  Every piece hides one format; the kernels keep
// their own scheduling.  Included by conv_kernel.h, through which every kernel header of the family gets it.
#pragma once
#include "common.h"

template <typename T> struct frag;                          // conv_kernel.h: 8 K-values of one MFMA operand row

// "Plain" source: the staged halo is the raw data (no scale / shift, no activation, no keep mask, no channel multipliers).
__device__ __forceinline__ bool src_is_plain(const chap_src_t& s) {
    return s.scale == nullptr && !s.act && s.keep == nullptr && s.chan_mul == nullptr;
}

// ---- BatchNorm statistics: registers -> 16-lane DPP reduce -> LDS row of this wave -> the four rows summed in a fixed
// order -> this block's partial slot (plain stores: no atomics anywhere, chap_bn_finalize sums the slots in a fixed
// order, so the statistics are bitwise reproducible for a given launch geometry).
// conv_stats_row takes one of the lane's moments pairs -- output channel (nt0 + t) * 16 + 4 * g + j over the pixels it owned -- to the wave's row;
// conv_stats_flush, once all 4 * NT pairs are there, writes the slot.  bstat: 4 * 2 * 16 * NT floats that no wave still reads (a kernel whose
// bstat follows a reused buffer puts its barrier in front).  256 threads, grid (slots, channel groups).  Scalars only in the interface: an
// accumulator array passed by reference keeps its stack slot until after inlining, which moved the register allocation of conv_fwd_kernel.
template <int NT>
__device__ __forceinline__ void conv_stats_row(float* bstat, int t, int j, float sum, float sq, int wave, int g, int px) {
    const float s = row16_sum(sum), q = row16_sum(sq);
    if (px == 0) {
        bstat[(wave * 2 + 0) * 16 * NT + t * 16 + 4 * g + j] = s;
        bstat[(wave * 2 + 1) * 16 * NT + t * 16 + 4 * g + j] = q;
    }
}
template <int NT>
__device__ __forceinline__ void conv_stats_flush(float* bstat, float* stats, int Cout, int nt0) {
    __syncthreads();
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *(int*)stats = (int)gridDim.x;      // header: slots in use
    float* st = stats + CHAP_STATS_HDR + (long)blockIdx.x * 2 * Cout;      // slot rows are indexed by the LOGICAL channel (a transposed conv's sub-lattices are folded by the finalize)
    for (int i = threadIdx.x; i < 2 * 16 * NT; i += 256) {
        const int which = i / (16 * NT), k = i % (16 * NT);
        const int nl = nt0 * 16 + k;
        const float v = (bstat[(0 * 2 + which) * 16 * NT + k] + bstat[(1 * 2 + which) * 16 * NT + k]) + (bstat[(2 * 2 + which) * 16 * NT + k] + bstat[(3 * 2 + which) * 16 * NT + k]);
        if (nl < Cout) st[which * Cout + nl] = v;
    }
}

// ---- MFMA pixel fragments.  Step `step` of a K-chunk multiplies the packed-weight fragment block `step` (chap_pack_weights: lane group g holds
// position p = step * 4 + g of the chunk's (tap, 8-channel group) list) with this lane's pixel fragment at LDS element offset xo (+ rowoff for
// the row); xo = -1: zero fragment (the positions behind the last tap, only in the chunk's last step).  The kernels compute xo themselves: it
// is their halo geometry.
template <typename T, int NP>
__device__ __forceinline__ typename frag<T>::type load_xfrag(const T* halo, int xo, int rowoff, int step) {
    if (step * 4 + 3 < NP) return frag<T>::load(halo + xo + rowoff);        // every lane group has a tap
    return xo >= 0 ? frag<T>::load(halo + xo + rowoff) : frag<T>::zero();
}

// ---- halo bounds test (see "register-staged prefetch" in conv_kernel.h): whether a unit lies inside the input; a unit that does not loads the
// tile's first output pixel (always inside) and is zeroed at commit time.
constexpr int UNIT_UNUSED = 511 << 20;                          // z field beyond any halo: never inside
constexpr unsigned UNIT_GUARD = (1u << 29) | (1u << 19) | (1u << 9);
struct halo_bounds_t {
    long gp0;                  // halo origin in input pixels (may lie outside: only offsets that pass the bounds test are used)
    unsigned PA, PB, rsafe;    // packed (512 - lo), (512 - hi) of the valid range; pixel offset of the tile's first output pixel
    // hzyx: a unit's packed halo coordinates (unit_desc)
    __device__ __forceinline__ bool inside(int hzyx) const { const unsigned d = (unsigned)hzyx; return (((d + PA) ^ (d + PB)) & UNIT_GUARD) == UNIT_GUARD; }
};
template <typename G, bool D3, int ST>
__device__ __forceinline__ halo_bounds_t halo_bounds(int ID, int IH, int IW, int n, int z0, int y0, int x0) {
    halo_bounds_t B;
    const int gz0 = z0 * G::STD - (D3 ? G::PAD : 0), gy0 = y0 * ST - G::PAD, gx0 = x0 * ST - G::PAD;
    B.gp0 = (((long)n * ID + gz0) * IH + gy0) * IW + gx0;
    const int loz = max(0, -gz0), hiz = min(G::HD, ID - gz0), loy = max(0, -gy0), hiy = min(G::HH, IH - gy0), lox = max(0, -gx0), hix = min(G::HW, IW - gx0);
    B.PA = ((unsigned)(512 - loz) << 20) | ((unsigned)(512 - loy) << 10) | (unsigned)(512 - lox);
    B.PB = ((unsigned)(512 - hiz) << 20) | ((unsigned)(512 - hiy) << 10) | (unsigned)(512 - hix);
    B.rsafe = ((D3 ? G::PAD : 0) * IH + G::PAD) * IW + G::PAD;
    return B;
}

// ---- scale / shift cache in LDS: per source [scale | shift] halves of AFFC / 2 channels each (identity when a source has none).
// Fill of one source's part by the 256 threads of the block.  (conv_fwd_kernel and conv_kpar2d_kernel fill the same layout in two phases,
// loads first, inside their prologues' load batches.)
template <int AFFC>
__device__ __forceinline__ void aff_cache_fill(float* aff_s, const chap_src_t& S) {
    const bool has = S.scale != nullptr;
    for (int c = threadIdx.x; c < S.C && c < AFFC / 2; c += 256) {
        aff_s[c] = has ? S.scale[c] : 1.f;
        aff_s[AFFC / 2 + c] = has ? S.shift[c] : 0.f;
    }
}

// ---- wave-private tile assignment (conv_wp_kernel, wgrad_wp_kernel): XCD-aware, waves as the unit.  Blocks b and b + 8 share an XCD, which
// owns a contiguous eighth of the tiles; its waves take them round-robin, so the tiles in flight on an XCD are neighbours (halo rows hit in its L2).
struct wp_tile_walk {
    long t_lo, my_tiles, last_tile;
    int sj, bpx;
    __device__ __forceinline__ wp_tile_walk(int nblocks, int block, int wave, long ntiles) {
        const int NG = nblocks < 8 ? nblocks : 8;
        const int xcd = block % NG;
        sj = (block / NG) * 4 + wave;
        bpx = ((nblocks + NG - 1 - xcd) / NG) * 4;
        const long per = (ntiles + NG - 1) / NG;
        t_lo = per * xcd;
        const long t_hi = t_lo + per < ntiles ? t_lo + per : ntiles;
        my_tiles = (bpx > 0 && t_lo + sj < t_hi) ? (t_hi - t_lo - sj + bpx - 1) / bpx : 0;
        last_tile = t_lo + sj + (my_tiles > 0 ? my_tiles - 1 : 0) * bpx;
    }
    // k-th tile of this wave; past the end: its last tile again (the tail re-requests it: every prefetch register is consumed on every path)
    __device__ __forceinline__ long tile_of(long k) const { const long t = t_lo + sj + k * bpx; return t < last_tile ? t : last_tile; }
};

// A wave's region is single-buffered: it commits tile k + 1 over tile k.  The hardware executes a wave's LDS operations in order; these two
// tell the COMPILER the order as well (no instructions: per-lane accesses it can prove disjoint could otherwise move across), one lane's commit
// stores against the other lanes' fragment reads.  wp_lds_committed: behind a commit, before the first fragment read; wp_lds_consumed: behind
// a tile's last fragment read, before the next commit.
__device__ __forceinline__ void wp_lds_committed() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ void wp_lds_consumed() { __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// ---- channel-last output: element offset of logical output channel nl of tile column px (out2: the channels from out2_from on land in a
// second dense tensor, at channel nl - out2_from)
__device__ __forceinline__ int cl_out_offset(const chap_conv_params& P, int nl, int px) {
    return px * P.out_ld + P.out_coff + ((P.out2 && nl >= P.out2_from) ? nl - P.out2_from : nl);
}
