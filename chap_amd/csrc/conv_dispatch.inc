// Included by the conv_inst_*.hip translation units with CONV_T (element type), CONV_FN (exported
// launcher name) and CONV_GEOM (1..5) defined: instantiates ONE geometry family for ONE element type
// (the table is split over translation units so that the build parallelises).
#include "conv_kernel.h"
#include "launchers.h"

// Per-device launch caches (CU count, LDS attribute, occupancy), safe for concurrent callers on different streams /
// devices: one atomic word per cached value (launch.h: chap_raise_lds).
static int conv_cu_count(int dev) {
    static std::atomic<int> cus[CHAP_MAX_DEVICES];
    int c = cus[dev].load(std::memory_order_acquire);
    if (!c) {
        hipDeviceProp_t pr;
        c = (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
        cus[dev].store(c, std::memory_order_release);
    }
    return c;
}

template <int KS, int ST, bool D3, int KC, int NT, int MR, bool ADD2, bool WLDS, bool ZW, bool ONE>
static int launch_inst(const chap_conv_params* p, size_t lds, long ntiles, int gy, hipStream_t stream) {
    const void* kern = chap_kernel<chap_conv_params, conv_fwd_kernel<CONV_T, KS, ST, D3, KC, NT, MR, ADD2, WLDS, ZW, ONE>, 256, conv_min_waves<KC, D3, CONV_T>()>();
    // per (instance, device): the LDS attribute, and (LDS size << 8 | occupancy) of the last occupancy query
    static chap_lds_cache attr_lds;
    static std::atomic<unsigned long long> occ_key[CHAP_MAX_DEVICES];
    const int dev = chap_device();
    if (int r = chap_raise_lds(attr_lds, dev, kern, lds, "chap_conv_fwd")) return r;
    unsigned long long ok = occ_key[dev].load(std::memory_order_acquire);
    if ((ok >> 8) != (unsigned long long)lds + 1) {          // resident blocks per CU for this (kernel, LDS size): sizes the persistent grid
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kern, 256, lds) != hipSuccess || o < 1) o = 1;
        ok = (((unsigned long long)lds + 1) << 8) | (unsigned long long)(o > 4 ? 4 : o);
        occ_key[dev].store(ok, std::memory_order_release);
    }
    int occ = (int)(ok & 0xff);
    // blocks per CU of the persistent grid: 2D at most 2 (round 3, whole iteration, three on-box A/B pairs: 6.757-6.777 -> 6.700-6.735 ms; 3: 6.72-6.77),
    // 3D whatever fits (1 is +0.5 ms, 2 = flat).  CHAP_CONV_OCC_CAP (lab knob) overrides both.
    { const int occ_cap = (int)chap_knob(KNOB_CONV_OCC_CAP), cap_ = occ_cap ? occ_cap : (D3 ? 0 : 2); if (cap_ && occ > cap_) occ = cap_; }
    long cap = (long)conv_cu_count(dev) * occ / gy;
    if (cap > CHAP_STATS_MAX_SLOTS) cap = CHAP_STATS_MAX_SLOTS;      // one statistics slot per block (chap_hip.h)
    cap = cap / 8 * 8;
    if (cap < 8) cap = 8;
    long gx = (ntiles + 7) / 8 * 8;
    if (gx > cap) gx = cap;
    return chap_launch_ptr<chap_conv_params>(kern, dim3((unsigned)gx, gy), dim3(256), lds, stream, *p, "chap_conv_fwd");
}

template <int KS, int ST, bool D3, int KC, int NT, int MR, bool ADD2, bool ZW = false>
static int launch_one(const chap_conv_params* p, const conv_blocking& b, hipStream_t stream) {
    typedef conv_geom<KS, ST, D3, MR, ZW> G;
    constexpr int GPT = KC / 8, NP = G::NTAPS * GPT, STEPS = (NP + 3) / 4;
    const size_t fixed = conv_lds_fixed_bytes<CONV_T, KS, ST, D3, KC, MR, ZW>(NT) + 2 * CONV_MAX_AFFINE_C * sizeof(float);
    const size_t wbytes = (size_t)b.nchunks * STEPS * NT * 64 * 8 * sizeof(CONV_T);
    // Resident weights (all K-chunks of the block's output channels, loaded once) while they fit beside the halo buffers: up to 100 KB of
    // LDS per block in 2D, the whole CU (158 KB) in 3D.  Round 1 set 40 KB from stand-alone layer timings (">= 4 blocks per CU"); swept on the
    // whole iteration (CHAP_CONV_WLDS_KB = 24 / 40 / 80 / 100 / 120 / 150 / 158: 2D 7.33 / 7.14 / 7.10 / 7.08 / 7.22 / 7.24 / - ms per step, 3D
    // 16.65 / 16.63 / - / 16.45 / 16.29 / 16.21 / 16.20) fewer, fatter blocks that never re-stage their weights win.
    const long wlds_env = chap_knob(KNOB_CONV_WLDS_KB);      // lab knob
    const size_t wlds_kb = wlds_env ? (size_t)wlds_env : (D3 ? 158 : 100);
    const bool wlds = fixed + wbytes <= wlds_kb * 1024;
    // otherwise one K-chunk's weights are staged through an LDS buffer when they fit (conv_wstaged)
    const size_t wst_bytes = (conv_one_wbuf<CONV_T>() ? 1 : 2) * (size_t)STEPS * NT * 512 * sizeof(CONV_T);      // bf16: ONE buffer (conv_kernel.h: the commit at the end of an item)
    const bool wstage = !wlds && conv_wstaged<CONV_T, KS, ST, D3, KC, NT, MR, ZW>();
    const size_t lds = fixed + (wlds ? wbytes : (wstage ? wst_bytes : 0));
    const long ntiles = (long)p->N * cdiv(p->D, G::TD) * cdiv(p->H, G::TH) * cdiv(p->W, G::TW);
    const int gy = cdiv(b.ntiles, NT);
    if constexpr (!ADD2) {
        if (p->nsrc == 1) {                                      // single-source specialisation (no source selects, fewer SGPRs)
            if (wlds) return launch_inst<KS, ST, D3, KC, NT, MR, ADD2, true, ZW, true>(p, lds, ntiles, gy, stream);
            return launch_inst<KS, ST, D3, KC, NT, MR, ADD2, false, ZW, true>(p, lds, ntiles, gy, stream);
        }
    }
    if (wlds) return launch_inst<KS, ST, D3, KC, NT, MR, ADD2, true, ZW, false>(p, lds, ntiles, gy, stream);
    return launch_inst<KS, ST, D3, KC, NT, MR, ADD2, false, ZW, false>(p, lds, ntiles, gy, stream);
}

template <int KS, int ST, bool D3, int MR, bool ADD2, bool ZW = false>
static int launch_geom(const chap_conv_params* p, const conv_plan& q, hipStream_t s) {
    if (q.b.KC == 32) {
        if (q.NT == 4) return launch_one<KS, ST, D3, 32, 4, MR, ADD2, ZW>(p, q.b, s);
        if (q.NT == 2) return launch_one<KS, ST, D3, 32, 2, MR, ADD2, ZW>(p, q.b, s);
        return launch_one<KS, ST, D3, 32, 1, MR, ADD2, ZW>(p, q.b, s);
    }
    if (q.NT == 4) return launch_one<KS, ST, D3, 16, 4, MR, ADD2, ZW>(p, q.b, s);
    if (q.NT == 2) return launch_one<KS, ST, D3, 16, 2, MR, ADD2, ZW>(p, q.b, s);
    return launch_one<KS, ST, D3, 16, 1, MR, ADD2, ZW>(p, q.b, s);
}

// q.MR = rows of 16 pixels per wave (tile = 4*MR x 16); conv_make_plan (conv_plan.h) picked KC, NT, MR.
int CONV_FN(const chap_conv_params* p, const conv_plan& q, hipStream_t s) {
#if CONV_GEOM == 1      // 2D 3x3 s1; add-combine variant (UpBlock_plus, unet.py:100-122) on the 8 x 16 tile only
    if (p->combine == 1 && p->nsrc == 2) return launch_geom<3, 1, false, 2, true>(p, q, s);
    if (q.MR == 4) return launch_geom<3, 1, false, 4, false>(p, q, s);
    if (q.MR == 2) return launch_geom<3, 1, false, 2, false>(p, q, s);
    return launch_geom<3, 1, false, 1, false>(p, q, s);
#elif CONV_GEOM == 2    // 3D 3x3x3 s1; add-combine variant for the V-Net skip add
    // MR == 4 (bf16): 4 x 4 x 16 output brick, one z-plane per wave (halo 6x6x18 = 2.5 loads per output instead
    // of 5.1 for the 1 x 4 x 16 slab, which is what still fits the LDS twice in fp32).
    if constexpr (sizeof(CONV_T) == 2) if (q.MR == 4) {
        if (p->combine == 1 && p->nsrc == 2) return launch_geom<3, 1, true, 4, true, true>(p, q, s);
        return launch_geom<3, 1, true, 4, false, true>(p, q, s);
    }
    if (p->combine == 1 && p->nsrc == 2) return launch_geom<3, 1, true, 1, true>(p, q, s);
    return launch_geom<3, 1, true, 1, false>(p, q, s);
#elif CONV_GEOM == 3    // 1x1(x1)
    if (q.MR == 2) return launch_geom<1, 1, false, 2, false>(p, q, s);
    return launch_geom<1, 1, false, 1, false>(p, q, s);
#elif CONV_GEOM == 4    // 2D k2 s2
    return launch_geom<2, 2, false, 2, false>(p, q, s);
#else                   // 3D k2 s2
    return launch_geom<2, 2, true, 1, false>(p, q, s);
#endif
}
