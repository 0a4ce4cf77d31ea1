// Included by wgrad_bf16.hip / wgrad_f32.hip with WG_T and WG_FN defined.
#include "wgrad_kernel.h"
#include "wgrad_wp.h"
#include "launchers.h"

// Prefetch distance (tiles in flight per block).  Measured (round 2, gpurun_out/wg_pd_*.log): PD = 3 / 2 (16- / 32-channel
// chunks) is SLOWER than PD = 1 on every layer shape (2D weight gradients 2.22 -> 2.72 ms per iteration, 3D 5.61 -> 6.29):
// the ring's registers (188 VGPRs for the 16-channel 2D kernel) cost a resident block per CU, and hipcc still drains the
// load queue (s_waitcnt vmcnt(0)) at the head of the tile loop, so the extra tiles in flight buy less than the lost block.
template <int KC> constexpr int wg_pd() {
#ifdef CHAP_WGRAD_PD
    return CHAP_WGRAD_PD;
#else
    return 1;
#endif
}

// grid = (pixel splits, A chunks, B tiles): the layout of the nsplit slabs wg_make_plan sized the workspace for
template <int KC, int BN>
static int wg_issue(const void* kern, size_t lds, chap_lds_cache& attr, const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t stream, const char* who) {
    if (int r = chap_raise_lds(attr, chap_device(), kern, lds, who)) return r;
    dim3 grid((unsigned)q.nsplit, (unsigned)(q.Ca / KC), (unsigned)cdiv(q.Cb, BN));
    const wgrad_args a = {*p, ws, ws_db, q.nsplit, q.Ca, q.Cb, (int)grid.z};
    return chap_launch_ptr<wgrad_args>(kern, grid, dim3(256), lds, stream, a, who);
}

template <int KS, int ST, bool D3, int KC, int MR, bool ADD2, int BN, bool ZW>
static int wg_launch_bn(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t stream) {
    static chap_lds_cache attr;
    return wg_issue<KC, BN>((const void*)chap_grouped_z<wgrad_args, wgrad_kernel<WG_T, KS, ST, D3, KC, MR, ADD2, BN, wg_pd<KC>(), ZW>, 256, (sizeof(WG_T) == 2 ? CHAP_WGRAD_MINW : 1)>,
                            wgrad_lds_bytes<WG_T, KS, ST, D3, KC, MR, BN, ZW>(), attr, p, q, ws, ws_db, stream, "chap_wgrad");
}

// q.bn: 16-wide B tiles for the full-resolution levels (half the B staging and MFMAs), 32 otherwise
template <int KS, int ST, bool D3, int KC, int MR, bool ADD2, bool ZW = false>
static int wg_launch_one(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t stream) {
    if (q.bn == 16) return wg_launch_bn<KS, ST, D3, KC, MR, ADD2, 16, ZW>(p, q, ws, ws_db, stream);
    return wg_launch_bn<KS, ST, D3, KC, MR, ADD2, 32, ZW>(p, q, ws, ws_db, stream);
}

// wave-private pipelines (wgrad_wp.h): 2D 3x3 bf16 layers picked by wg_make_plan (brick == 2)
template <int KC, int MR, int BN>
static int wg_launch_wp(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t stream) {
    if constexpr (sizeof(WG_T) == 2) {
        static chap_lds_cache attr;
        return wg_issue<KC, BN>((const void*)chap_grouped_z<wgrad_args, wgrad_wp_kernel<KC, MR, BN>, 256, (MR == 1 && BN == 16) ? 3 : 2>, wgrad_wp_lds_bytes<KC, MR, BN>(), attr, p, q, ws, ws_db, stream, "chap_wgrad(wp)");
    } else {
        chap_set_error("chap_wgrad: wave-private pipelines are bf16 only");
        return CHAP_EUNSUPPORTED;
    }
}

template <int KS, int ST, bool D3, int MR, bool ADD2 = false>
static int wg_launch_geom(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t s) {
    if (q.KC == 32) return wg_launch_one<KS, ST, D3, 32, MR, ADD2>(p, q, ws, ws_db, s);
    return wg_launch_one<KS, ST, D3, 16, MR, ADD2>(p, q, ws, ws_db, s);
}

int WG_FN(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t s) {
    const bool d3 = p->dims == 3;
    const bool add2 = p->combine == 1 && p->na == 2;
    if (add2 && !(p->ksize == 3 && p->stride == 1)) { chap_set_error("chap_wgrad: add-combine is built for k3 s1 only"); return CHAP_EUNSUPPORTED; }
    if (q.brick == 2) {       // 2D 3x3, wave-private pipelines, 16-channel A chunks (wgrad_plan.h: wg_make_plan)
        if (d3 || add2 || p->ksize != 3 || p->stride != 1 || q.KC != 16) { chap_set_error("chap_wgrad: wave-private pipelines are built for 2D k3 s1, KC 16"); return CHAP_EUNSUPPORTED; }
        if (q.bn == 32) return wg_launch_wp<16, 1, 32>(p, q, ws, ws_db, s);
        return q.mr == 1 ? wg_launch_wp<16, 1, 16>(p, q, ws, ws_db, s) : wg_launch_wp<16, 2, 16>(p, q, ws, ws_db, s);
    }
    if constexpr (sizeof(WG_T) == 2) {
        if (q.brick == 1) {   // 3D 3x3x3, 4 x 4 x 16 bricks, 16-channel A chunks (wgrad_plan.h: wg_make_plan)
            if (!(d3 && p->ksize == 3 && p->stride == 1 && q.KC == 16)) { chap_set_error("chap_wgrad: brick tiles are built for 3D k3 s1, KC 16"); return CHAP_EUNSUPPORTED; }
            return add2 ? wg_launch_one<3, 1, true, 16, 4, true, true>(p, q, ws, ws_db, s) : wg_launch_one<3, 1, true, 16, 4, false, true>(p, q, ws, ws_db, s);
        }
    }
    if (p->ksize == 3 && p->stride == 1) {
        if (d3) return add2 ? wg_launch_geom<3, 1, true, 1, true>(p, q, ws, ws_db, s) : wg_launch_geom<3, 1, true, 1, false>(p, q, ws, ws_db, s);
        return add2 ? wg_launch_geom<3, 1, false, 2, true>(p, q, ws, ws_db, s) : wg_launch_geom<3, 1, false, 2>(p, q, ws, ws_db, s);
    }
    if (p->ksize == 1 && p->stride == 1) return wg_launch_geom<1, 1, false, 2>(p, q, ws, ws_db, s);
    if (p->ksize == 2 && p->stride == 2) return d3 ? wg_launch_geom<2, 2, true, 1>(p, q, ws, ws_db, s) : wg_launch_geom<2, 2, false, 2>(p, q, ws, ws_db, s);
    chap_set_error("chap_wgrad: unsupported (ksize=%d, stride=%d)", p->ksize, p->stride);
    return CHAP_EUNSUPPORTED;
}
