#define CONV_T bf16_t
#define CONV_GEOM 3
#define CONV_FN chap_conv_launch_bf16_g3
#include "conv_dispatch.inc"

// the V-Net heads (conv_head1x1_kernel, conv_kernel.h): the 1x1 layers conv_make_plan routes past the MFMA kernel
int chap_conv_launch_head_bf16(const chap_conv_params* p, hipStream_t s) {
    const long total = (long)p->N * p->D * p->H * p->W;
    return chap_launch<chap_conv_params, conv_head1x1_kernel<bf16_t>, 256>(dim3(chap_blocks(total, 4096)), dim3(256), 0, s, *p, "chap_conv_fwd(head)");
}
