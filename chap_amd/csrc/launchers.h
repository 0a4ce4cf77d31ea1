// Prototypes of the instance launchers behind chap_conv_fwd and chap_wgrad: each takes the params and the plan that host code made
// (conv_plan.h, wgrad_plan.h) and picks the template instance the plan names.
#pragma once
#include "common.h"
#include "conv_plan.h"
#include "wgrad_plan.h"

// generic conv_fwd_kernel, one translation unit per (element type, geometry family): conv_inst_*.hip -> conv_dispatch.inc
#define CHAP_DECL_GEOM(dt, g) int chap_conv_launch_##dt##_g##g(const chap_conv_params* p, const conv_plan& q, hipStream_t s);
CHAP_DECL_GEOM(bf16, 1) CHAP_DECL_GEOM(bf16, 2) CHAP_DECL_GEOM(bf16, 3) CHAP_DECL_GEOM(bf16, 4) CHAP_DECL_GEOM(bf16, 5)
CHAP_DECL_GEOM(f32, 1) CHAP_DECL_GEOM(f32, 2) CHAP_DECL_GEOM(f32, 3) CHAP_DECL_GEOM(f32, 4) CHAP_DECL_GEOM(f32, 5)
#undef CHAP_DECL_GEOM
int chap_conv_launch_head_bf16(const chap_conv_params* p, hipStream_t s);                       // conv_inst_bf16_g3.hip
int chap_conv_launch_wp_bf16(const chap_conv_params* p, const conv_plan& q, hipStream_t s);     // conv_wp_bf16.hip
int chap_conv_launch_kpar_bf16(const chap_conv_params* p, const conv_plan& q, hipStream_t s);   // conv_kpar_bf16.hip

// wgrad_bf16.hip / wgrad_f32.hip -> wgrad_dispatch.inc
int chap_wgrad_launch_bf16(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t s);
int chap_wgrad_launch_f32(const chap_wgrad_params* p, const wg_plan& q, float* ws, float* ws_db, hipStream_t s);
