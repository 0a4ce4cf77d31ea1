// Launcher of conv_kpar_kernel (conv_kpar.h): the deep, small 3x3(x3) layers in bf16.  conv_make_plan (conv_plan.h) decides eligibility.
#include "conv_kpar.h"
#include "conv_kpar2d.h"
#include "launchers.h"

// one block per tile of TH x 16 pixels and pair of 16-channel tiles (NT = 2), one statistics slot per block (chap_hip.h)
static int kpar_issue(const void* kern, size_t lds, chap_lds_cache& attr, const chap_conv_params* p, const conv_blocking& b, int TH, hipStream_t stream, const char* name) {
    if (int r = chap_raise_lds(attr, chap_device(), kern, lds, name)) return r;
    const long ntiles = (long)p->N * p->D * cdiv(p->H, TH) * cdiv(p->W, 16);
    const long gx = ntiles < CHAP_STATS_MAX_SLOTS ? ntiles : CHAP_STATS_MAX_SLOTS;
    return chap_launch_ptr<chap_conv_params>(kern, dim3((unsigned)gx, cdiv(b.ntiles, 2)), dim3(256), lds, stream, *p, name);
}

template <bool D3, int KC, int CPAR, bool ONE>
static int kpar_launch(const chap_conv_params* p, const conv_blocking& b, hipStream_t stream) {
    static chap_lds_cache attr;
    return kpar_issue(chap_kernel<chap_conv_params, conv_kpar_kernel<bf16_t, D3, KC, 2, CPAR, ONE>, 256, 2>(), conv_kpar_lds_bytes<bf16_t, D3, KC, CPAR>(2), attr, p, b,
                      conv_geom<3, 1, D3, D3 ? 1 : 2>::TH, stream, "chap_conv_fwd(kpar)");
}

// 2D, 32-channel chunks: the round-4 kernel (conv_kpar2d.h)
template <int CPAR, bool ONE, bool KEEPM, bool SINGLE>
static int kpar2d_launch(const chap_conv_params* p, const conv_blocking& b, hipStream_t stream) {
    static chap_lds_cache attr;
    return kpar_issue(chap_kernel<chap_conv_params, conv_kpar2d_kernel<2, CPAR, ONE, KEEPM, SINGLE>, 256, 2>(), conv_kpar_lds_bytes<bf16_t, false, 32, CPAR>(2), attr, p, b,
                      conv_geom<3, 1, false, 2>::TH, stream, "chap_conv_fwd(kpar2d)");
}
template <int CPAR>
static int kpar2d_one(const chap_conv_params* p, const conv_blocking& b, hipStream_t s) {
    const bool single = b.nchunks == CPAR, keep = p->src[0].keep || (p->nsrc > 1 && p->src[1].keep), one = p->nsrc == 1;
#define CHAP_K2D(O, K, S) if (one == O && keep == K && single == S) return kpar2d_launch<CPAR, O, K, S>(p, b, s)
    CHAP_K2D(true, false, true); CHAP_K2D(true, true, true); CHAP_K2D(false, false, true); CHAP_K2D(false, true, true);
    CHAP_K2D(true, false, false); CHAP_K2D(true, true, false); CHAP_K2D(false, false, false); CHAP_K2D(false, true, false);
#undef CHAP_K2D
    return CHAP_EUNSUPPORTED;
}

template <bool D3, int KC, int CPAR>
static int kpar_one(const chap_conv_params* p, const conv_blocking& b, hipStream_t s) {
    return p->nsrc == 1 ? kpar_launch<D3, KC, CPAR, true>(p, b, s) : kpar_launch<D3, KC, CPAR, false>(p, b, s);
}

// q.b.KC: the K-chunk the weights were packed with (16 / 32); q.cpar: chunks side by side (2 / 4)
int chap_conv_launch_kpar_bf16(const chap_conv_params* p, const conv_plan& q, hipStream_t s) {
    const bool d3 = p->dims == 3;
    if (q.b.KC == 32) {
        if (q.cpar == 4) return d3 ? kpar_one<true, 32, 4>(p, q.b, s) : kpar2d_one<4>(p, q.b, s);
        return d3 ? kpar_one<true, 32, 2>(p, q.b, s) : kpar2d_one<2>(p, q.b, s);
    }
    if (q.cpar == 4) return d3 ? kpar_one<true, 16, 4>(p, q.b, s) : kpar_one<false, 16, 4>(p, q.b, s);
    return d3 ? kpar_one<true, 16, 2>(p, q.b, s) : kpar_one<false, 16, 2>(p, q.b, s);
}
