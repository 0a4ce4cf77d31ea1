// Launcher of conv_wp_kernel (conv_wp.h): the 2D full-resolution 3x3 layers in bf16, wave-private pipelines.  conv_make_plan (conv_plan.h) decides eligibility.
#include "conv_wp.h"
#include "launchers.h"

template <int KC, int NT, bool LANESEL>
static int conv_wp_launch(const chap_conv_params* p, const conv_blocking& b, hipStream_t stream) {
    typedef conv_geom<3, 1, false, 1, false> G;
    constexpr int MINW = KC == 16 ? (NT == 1 ? 4 : 3) : 2;      // waves per SIMD the registers allow without spilling (128 / 168 / 256 VGPRs)
    const void* kern = chap_kernel<chap_conv_params, conv_wp_kernel<KC, NT, LANESEL>, 256, MINW>();
    const size_t lds = conv_wp_lds_bytes<KC, NT>();
    static chap_lds_cache attr_lds;
    if (int r = chap_raise_lds(attr_lds, chap_device(), kern, lds, "chap_conv_fwd(wp)")) return r;
    const long ntiles = (long)p->N * cdiv(p->H, G::TH) * cdiv(p->W, G::TW);
    const int gy = cdiv(b.ntiles, NT);
    // persistent blocks of four wave pipelines: CHAP_CONV_WP_BPC blocks per CU (lab knob; default 4 with 16-channel chunks, 2 with 32), at least two tiles per wave
    const long bpc_env = chap_knob(KNOB_CONV_WP_BPC), bpc = bpc_env ? bpc_env : (KC == 16 ? 4 : 2);
    long gx = 256 * bpc / gy;
    const long need = (ntiles + 7) / 8;                         // two tiles per wave
    if (gx > need) gx = need;
    if (gx > CHAP_STATS_MAX_SLOTS) gx = CHAP_STATS_MAX_SLOTS;
    gx = gx >= 8 ? gx / 8 * 8 : (gx < 1 ? 1 : gx);
    return chap_launch_ptr<chap_conv_params>(kern, dim3((unsigned)gx, gy), dim3(256), lds, stream, *p, "chap_conv_fwd(wp)");
}

// q.b.KC = all input channels (16 or 32) in one chunk; two concatenated sources inside it: per-lane source select.  q.NT = 1 / 2 block tiles.
int chap_conv_launch_wp_bf16(const chap_conv_params* p, const conv_plan& q, hipStream_t s) {
    const bool two = p->nsrc == 2;
    if (q.b.KC == 16) {
        if (two) { chap_set_error("chap_conv_fwd(wp): two sources need a 32-channel chunk"); return CHAP_EUNSUPPORTED; }
        return q.NT == 1 ? conv_wp_launch<16, 1, false>(p, q.b, s) : conv_wp_launch<16, 2, false>(p, q.b, s);
    }
    if (q.NT == 1) return two ? conv_wp_launch<32, 1, true>(p, q.b, s) : conv_wp_launch<32, 1, false>(p, q.b, s);
    return two ? conv_wp_launch<32, 2, true>(p, q.b, s) : conv_wp_launch<32, 2, false>(p, q.b, s);
}
