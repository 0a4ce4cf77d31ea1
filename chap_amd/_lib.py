"""ctypes binding of libchap_hip.so (the C ABI declared in include/chap_hip.h).

This file is the "reference-side binding a maintainer would add" (INTEGRATION.md): the
reference is pure Python, so its FFI is ctypes.  Structures mirror the header field by field.
There is NO fallback: if the library is missing, `lib()` raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CHAP_LIBPATH") or os.path.join(_HERE, "libchap_hip.so")      # CHAP_LIBPATH: a lab build of the same sources (A/B of compile-time variants)

F32, BF16 = 0, 1
STATS_MAX_SLOTS, STATS_HDR = 1024, 4          # CHAP_STATS_MAX_SLOTS, CHAP_STATS_HDR
ACT_BWD_SLOTS = 1024                           # CHAP_ACT_BWD_SLOTS
LOSS_SLOTS, CHANSUM_SLOTS, L2NORM_SLOTS = 512, 512, 256
PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DECONV_FWD, PACK_DECONV_DGRAD, PACK_DOWN_DGRAD = range(5)

_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t


class Src(C.Structure):
    _fields_ = [("ptr", _vp), ("scale", _vp), ("shift", _vp), ("keep", _vp), ("chan_mul", _vp),
                ("C", _i32), ("ld", _i32), ("coff", _i32), ("act", _i32), ("slope", _f32), ("keep_scale", _f32)]


class ConvParams(C.Structure):
    _fields_ = [("src", Src * 2), ("nsrc", _i32), ("combine", _i32),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("ID", _i32), ("IH", _i32), ("IW", _i32),
                ("ksize", _i32), ("stride", _i32), ("dims", _i32),
                ("wpacked", _vp), ("bias", _vp), ("out", _vp),
                ("Cout", _i32), ("out_ld", _i32), ("out_coff", _i32), ("out_mode", _i32), ("out_Cn", _i32),
                ("out_planar", _i32), ("out_f32", _i32),
                ("stats", _vp), ("stats_shift", _vp), ("dtype", _i32), ("out2_from", _i32), ("out2", _vp)]


class PackParams(C.Structure):
    _fields_ = [("w", _vp), ("out", _vp), ("kind", _i32), ("Cin", _i32), ("Cout", _i32), ("taps", _i32), ("dtype", _i32)]


class PackEntry(C.Structure):
    _fields_ = [("w", _vp), ("out", _vp), ("kind", _i32), ("Cin", _i32), ("Cout", _i32), ("taps", _i32), ("dtype", _i32),
                ("KC", _i32), ("GPT", _i32), ("NP", _i32), ("STEPS", _i32), ("nchunks", _i32), ("ntiles", _i32),
                ("Cn_logical", _i32), ("Ck_real", _i32), ("total", _i64)]


class ConvC1Params(C.Structure):
    _fields_ = [("x", _vp), ("w", _vp), ("bias", _vp), ("out", _vp), ("stats", _vp), ("stats_shift", _vp),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("dims", _i32), ("Cout", _i32), ("dtype", _i32)]


class ConvC1BwdParams(C.Structure):
    _fields_ = [("g", _vp), ("w", _vp), ("x", _vp), ("dx", _vp), ("dw", _vp), ("db", _vp), ("ws", _vp),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("dims", _i32), ("Cout", _i32), ("dtype", _i32)]


class WgradParams(C.Structure):
    _fields_ = [("a", Src * 2), ("na", _i32), ("combine", _i32), ("b", Src),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("ID", _i32), ("IH", _i32), ("IW", _i32),
                ("ksize", _i32), ("stride", _i32), ("dims", _i32),
                ("dw", _vp), ("s_tap", _i64), ("s_kc", _i64), ("s_kn", _i64), ("kc_valid", _i32), ("kn_valid", _i32),
                ("db", _vp), ("ws", _vp), ("ws_bytes", _sz), ("dtype", _i32)]


class BnFinalizeParams(C.Structure):
    _fields_ = [("stats", _vp), ("stats_shift", _vp), ("Clog", _i32), ("gamma", _vp), ("beta", _vp),
                ("running_mean", _vp), ("running_var", _vp), ("num_batches_tracked", _vp),
                ("scale", _vp), ("shift", _vp), ("mean", _vp), ("invstd", _vp),
                ("C", _i32), ("count", _f32), ("eps", _f32), ("momentum", _f32)]


class BnEvalParams(C.Structure):
    _fields_ = [("gamma", _vp), ("beta", _vp), ("running_mean", _vp), ("running_var", _vp),
                ("scale", _vp), ("shift", _vp), ("C", _i32), ("eps", _f32)]


class ActBwdParams(C.Structure):
    _fields_ = [("g", _vp * 3), ("g_ld", _i32 * 3), ("g_coff", _i32 * 3), ("ng", _i32),
                ("g_pool", _vp), ("pool_idx", _vp), ("r", Src),
                ("mean", _vp), ("invstd", _vp), ("gamma", _vp), ("sums", _vp), ("gout", _vp),
                ("dgamma", _vp), ("dbeta", _vp),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("bn", _i32), ("count", _f32), ("dtype", _i32)]


class PoolParams(C.Structure):
    _fields_ = [("r", Src), ("out", _vp), ("idx", _vp), ("N", _i32), ("H", _i32), ("W", _i32), ("dtype", _i32), ("D", _i32)]


class UpsampleParams(C.Structure):
    _fields_ = [("r", Src), ("out", _vp), ("out_ld", _i32), ("out_coff", _i32),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("dims", _i32), ("dtype", _i32), ("half_pixel", _i32)]


class UpsampleBwdParams(C.Structure):
    _fields_ = [("g", _vp), ("g_ld", _i32), ("g_coff", _i32), ("out", _vp),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("C", _i32), ("dims", _i32), ("dtype", _i32)]


class PlanarToClParams(C.Structure):
    _fields_ = [("in_", _vp), ("out", _vp), ("N", _i32), ("C", _i32), ("P", _i32), ("out_ld", _i32), ("out_coff", _i32), ("Cpad", _i32), ("dtype", _i32)]


class ChanSumParams(C.Structure):
    _fields_ = [("r", Src), ("out", _vp), ("npix", _i64), ("pix_per_sample", _i64), ("dtype", _i32), ("ws", _vp)]


class ClToPlanarParams(C.Structure):
    _fields_ = [("r", Src), ("out", _vp), ("N", _i32), ("P", _i32), ("dtype", _i32)]


class MixLossParams(C.Structure):
    _fields_ = [("logits", _vp), ("target_a", _vp), ("target_b", _vp), ("mask", _vp), ("w_a", _f32), ("w_b", _f32),
                ("acc", _vp), ("loss", _vp), ("dlogits", _vp), ("gscale", _f32), ("accumulate", _i32),
                ("N", _i32), ("C", _i32), ("P", _i32), ("smooth", _f32), ("k_dice", _f32), ("k_ce", _f32), ("gscale_dev", _vp)]


class MixLossMultiParams(C.Structure):
    _fields_ = [("nterms", _i32), ("term", MixLossParams * 4)]


class PseudoParams(C.Structure):
    _fields_ = [("logits1", _vp), ("logits2", _vp), ("soft1", _vp), ("soft2", _vp), ("arg1", _vp), ("arg2", _vp),
                ("knowledge", _vp), ("N", _i32), ("C", _i32), ("P", _i32)]


class KlParams(C.Structure):
    _fields_ = [("logits", _vp * 2), ("target", _vp * 2), ("loss", _vp), ("dlogits", _vp * 2),
                ("gscale", _f32), ("gscale_dev", _vp), ("N", _i32), ("C", _i32), ("P", _i32), ("mode", _i32), ("ws", _vp)]


class EnsembleParams(C.Structure):
    _fields_ = [("logits1", _vp), ("logits2", _vp), ("prob", _vp), ("label", _vp), ("N", _i32), ("C", _i32), ("P", C.c_int64), ("mode", _i32)]


class WindowAccParams(C.Structure):
    _fields_ = [("logits", _vp), ("origins", _vp), ("score", _vp), ("cnt", _vp), ("npatch", _i32), ("C", _i32),
                ("pw", _i32), ("ph", _i32), ("pd", _i32), ("W", _i32), ("H", _i32), ("D", _i32)]


class WindowFinParams(C.Structure):
    _fields_ = [("score", _vp), ("cnt", _vp), ("label", _vp), ("C", _i32), ("P", C.c_int64)]


class WindowGatherParams(C.Structure):
    _fields_ = [("volume", _vp), ("origins", _vp), ("patches", _vp), ("npatch", _i32), ("W", _i32), ("H", _i32), ("D", _i32),
                ("pad_lo", _i32 * 3), ("pw", _i32), ("ph", _i32), ("pd", _i32)]


class WindowAccHeadsParams(C.Structure):
    _fields_ = [("logits", _vp * 2), ("origins", _vp), ("score", _vp), ("cnt", _vp), ("nheads", _i32), ("npatch", _i32), ("C", _i32),
                ("pw", _i32), ("ph", _i32), ("pd", _i32), ("W", _i32), ("H", _i32), ("D", _i32)]


class L2NormParams(C.Structure):
    _fields_ = [("in_", _vp), ("out", _vp), ("N", _i32), ("P", _i32), ("eps", _f32), ("ws", _vp)]


class AxpyParams(C.Structure):
    _fields_ = [("x", _vp), ("d", _vp), ("mask", _vp), ("out", _vp), ("alpha", _f32), ("sign", _i32), ("n", _i64)]


class RandParams(C.Structure):
    _fields_ = [("out", _vp), ("seed", C.c_uint64), ("seed_dev", _vp), ("n", _i64), ("lo", _f32), ("hi", _f32)]


class KeepMaskParams(C.Structure):
    _fields_ = [("keep", _vp), ("seed", C.c_uint64), ("seed_dev", _vp), ("n", _i64), ("p", _f32)]


class ChanMaskParams(C.Structure):
    _fields_ = [("mul", _vp), ("seed", C.c_uint64), ("seed_dev", _vp), ("n", _i64), ("p", _f32)]


class SampleChanSumParams(C.Structure):
    _fields_ = [("r", Src), ("partial", _vp), ("N", _i32), ("nchunk", _i32), ("pix_per_sample", _i64), ("dtype", _i32)]


class ChannelDropParams(C.Structure):
    _fields_ = [("pool_partial", _vp), ("grad_sim", _vp), ("u1", _vp), ("u2", _vp), ("mul1", _vp), ("mul2", _vp),
                ("probs_out", _vp), ("inv_npix", _f32), ("nchunk", _i32), ("B", _i32), ("U", _i32), ("C", _i32),
                ("mode", _i32), ("comp", _i32), ("branch", _i32), ("prob_kind", _i32)]


class FoldParams(C.Structure):
    _fields_ = [("g", _vp), ("mul", _vp), ("out", _vp), ("B", _i32), ("U", _i32), ("C", _i32), ("ld", _i32), ("coff", _i32),
                ("pix_per_sample", _i64), ("dtype", _i32)]


class BoxMixParams(C.Structure):
    _fields_ = [("a", _vp), ("b", _vp), ("out", _vp), ("box", _vp), ("N", _i32), ("H", _i32), ("W", _i32), ("is_i64", _i32), ("D", _i32)]


class BoxMaskParams(C.Structure):
    _fields_ = [("mask", _vp), ("box", _vp), ("N", _i32), ("H", _i32), ("W", _i32), ("D", _i32)]


class BcpMixParams(C.Structure):
    _fields_ = [("a", _vp * 2), ("b", _vp * 2), ("out", _vp * 2), ("mask", _vp), ("box", _vp), ("N", _i32 * 2), ("Nm", _i32), ("H", _i32), ("W", _i32), ("D", _i32)]


class LccParams(C.Structure):
    _fields_ = [("labels", _vp), ("out", _vp), ("ws", _vp), ("N", _i32), ("H", _i32), ("W", _i32), ("num_classes", _i32), ("D", _i32)]


class DiffMaskParams(C.Structure):
    _fields_ = [("p1", _vp), ("p2", _vp), ("knowledge", _vp), ("out", _vp), ("pooled_ws", _vp),
                ("N", _i32), ("H", _i32), ("W", _i32), ("scale", _i32), ("k", _i32)]


class MetricResult(C.Structure):
    _fields_ = [("n_a", _i64), ("n_b", _i64), ("n_ab", _i64), ("n_ab_s", _i64), ("n_ba_s", _i64), ("q_lo", _i64), ("q_hi", _i64),
                ("sum_ab", C.c_double), ("sum_ba", C.c_double), ("max2_ab", C.c_double), ("max2_ba", C.c_double),
                ("v2_lo", C.c_double), ("v2_hi", C.c_double)]


class MetricsParams(C.Structure):
    _fields_ = [("a", _vp), ("b", _vp), ("a_i64", _i32), ("b_i64", _i32), ("classes", _vp), ("K", _i32), ("binary", _i32),
                ("ndim", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("distances", _i32), ("spacing", C.c_double * 3),
                ("border_a", _vp), ("border_b", _vp), ("dist", _vp), ("results", _vp), ("ws", _vp)]


METRICS_MAX_AXIS = 4096                        # CHAP_METRICS_MAX_AXIS

AUG_NONE, AUG_ROTFLIP, AUG_ROTATE = range(3)   # CHAP_AUG_*


class Augment2dRecord(C.Structure):
    _fields_ = [("offset", _i64), ("x", _i32), ("y", _i32), ("mode", _i32), ("k", _i32), ("axis", _i32), ("reserved", _i32),
                ("zoom", C.c_double * 2), ("m", C.c_double * 4), ("off", C.c_double * 2)]


class Augment2dParams(C.Structure):
    _fields_ = [("images", _vp), ("labels", _vp), ("store_elems", _i64), ("records", _vp), ("image_out", _vp), ("label_out", _vp),
                ("label_i64", _i32), ("B", _i32), ("H", _i32), ("W", _i32)]


class Augment3dRecord(C.Structure):
    _fields_ = [("offset", _i64), ("shape", _i32 * 3), ("corner", _i32 * 3), ("k", _i32), ("axis", _i32)]


class Augment3dParams(C.Structure):
    _fields_ = [("images", _vp), ("labels", _vp), ("store_elems", _i64), ("records", _vp), ("image_out", _vp), ("label_out", _vp),
                ("label_i64", _i32), ("B", _i32), ("P0", _i32), ("P1", _i32), ("P2", _i32)]


class Augment3dPadRecord(C.Structure):
    _fields_ = [("offset", _i64), ("shape", _i32 * 3), ("corner", _i32 * 3), ("pad", _i32 * 3), ("k", _i32), ("axis", _i32), ("reserved", _i32)]


class Augment3dPadParams(C.Structure):
    _fields_ = Augment3dParams._fields_


class ResidualParams(C.Structure):
    _fields_ = [("r", Src), ("src", Src * 2), ("nsrc", _i32), ("xin", _vp), ("out", _vp),
                ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("dtype", _i32)]


class ResidualBwdParams(C.Structure):
    _fields_ = [("g", _vp * 3), ("g_ld", _i32 * 3), ("g_coff", _i32 * 3), ("ng", _i32), ("out", _vp), ("chan_mul", _vp),
                ("gout", _vp), ("dxin", _vp), ("N", _i32), ("D", _i32), ("H", _i32), ("W", _i32), ("C", _i32), ("dtype", _i32)]


class GradSumParams(C.Structure):
    _fields_ = [("g", _vp * 4), ("g_ld", _i32 * 4), ("g_coff", _i32 * 4), ("ng", _i32), ("out", _vp), ("npix", _i64), ("C", _i32), ("dtype", _i32)]


class GradSimParams(C.Structure):
    _fields_ = [("gl", _vp), ("gu", _vp), ("score", _vp), ("C", _i32), ("K", _i32), ("ema", _f32)]


class SgdParams(C.Structure):
    _fields_ = [("param", _vp), ("grad", _vp), ("grad2", _vp), ("mom", _vp), ("lr", _vp), ("momentum", _f32), ("weight_decay", _f32),
                ("grad_scale", _f32), ("n", _i64), ("zero_grad", _i32)]


class SgdEmaParams(C.Structure):
    _fields_ = [("sgd", SgdParams), ("ema", _vp), ("coef", _vp)]


class GuardState(C.Structure):
    _fields_ = [("scale", _f32), ("skip", _i32), ("norm", _f32), ("steps", _i32), ("skipped_total", _i32), ("clipped_total", _i32), ("reserved", _i32 * 2)]


class GuardRow(C.Structure):
    _fields_ = [("step", _i32), ("norm", _f32), ("coef", _f32), ("skip", _i32)]


GRADNORM_SLOTS = 512                           # CHAP_GRADNORM_SLOTS of include/chap_hip_guard.h


class GradNormParams(C.Structure):
    _fields_ = [("grad", _vp), ("grad2", _vp), ("n", _i64), ("grad_scale", _f32), ("max_norm", _f32), ("skip_nonfinite", _i32), ("ring", _i32),
                ("ws", _vp), ("state", _vp)]


class SgdGuardParams(C.Structure):
    _fields_ = [("se", SgdEmaParams), ("state", _vp)]


class AdamTickParams(C.Structure):              # chap_adam_tick_params of include/chap_hip_optim.h
    _fields_ = [("state", _vp), ("lr", _vp), ("guard", _vp), ("beta1", _f32), ("beta2", _f32), ("weight_decay", _f32), ("decoupled", _i32)]


class AdamParams(C.Structure):                  # chap_adam_params
    _fields_ = [("param", _vp), ("grad", _vp), ("grad2", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("state", _vp), ("guard", _vp),
                ("ema", _vp), ("coef", _vp), ("beta1", _f32), ("beta2", _f32), ("eps", _f32), ("weight_decay", _f32),
                ("decoupled", _i32), ("grad_scale", _f32), ("zero_grad", _i32), ("n", _i64)]


class TeacherConsistencyParams(C.Structure):    # chap_teacher_consistency_params of include/chap_hip_teacher.h
    _fields_ = [("logits", _vp * 2), ("teacher", _vp * 2), ("dlogits", _vp * 2), ("loss", _vp), ("ws", _vp), ("gscale_dev", _vp),
                ("gscale", _f32), ("accumulate", _i32), ("N", _i32), ("C", _i32), ("P", _i32)]


UNCERTAINTY_MAX_T = 8            # CHAP_UNCERTAINTY_MAX_T of include/chap_hip_uncertainty.h


class TeacherUncertaintyParams(C.Structure):    # chap_teacher_uncertainty_params of include/chap_hip_uncertainty.h
    _fields_ = [("teacher", (_vp * 2) * UNCERTAINTY_MAX_T), ("mask", _vp), ("entropy", _vp), ("count", _vp), ("ws", _vp), ("threshold_dev", _vp),
                ("threshold", _f32), ("T", _i32), ("N", _i32), ("C", _i32), ("P", _i32)]


class TeacherConsistencyMaskedParams(C.Structure):      # chap_teacher_consistency_masked_params
    _fields_ = [("logits", _vp * 2), ("teacher", _vp * 2), ("mask", _vp), ("count", _vp), ("dlogits", _vp * 2), ("loss", _vp), ("ws", _vp),
                ("gscale_dev", _vp), ("gscale", _f32), ("accumulate", _i32), ("N", _i32), ("C", _i32), ("P", _i32)]


MONITOR_SLOTS, MONITOR_MAX_SCALARS, MONITOR_HDR = 512, 16, 2      # CHAP_MONITOR_* of include/chap_hip_monitor.h


class MonitorParams(C.Structure):
    _fields_ = [("logits", _vp * 2), ("labels", _vp), ("ws", _vp), ("N", _i32), ("C", _i32), ("P", _i32), ("n_first", _i32)]


class MonitorLabelsParams(C.Structure):
    _fields_ = [("maps", _vp * 2), ("labels", _vp), ("ws", _vp), ("N", _i32), ("C", _i32), ("P", _i32), ("n_first", _i32)]


class MonitorFinalizeParams(C.Structure):
    _fields_ = [("ws", _vp), ("ring", _vp), ("slot_iter", _vp), ("scalars", _vp * MONITOR_MAX_SCALARS),
                ("C", _i32), ("ring_rows", _i32), ("nscalars", _i32), ("has_labels", _i32)]


_SIGS = {  # name -> (restype, params struct or None)
    "chap_conv_fwd": ConvParams, "chap_pack_weights": PackParams, "chap_conv_c1_fwd": ConvC1Params,
    "chap_conv_c1_bwd": ConvC1BwdParams, "chap_wgrad": WgradParams, "chap_bn_finalize": BnFinalizeParams,
    "chap_bn_eval_affine": BnEvalParams, "chap_act_bwd_reduce": ActBwdParams, "chap_act_bwd_apply": ActBwdParams,
    "chap_act_pool2": PoolParams, "chap_upsample2x": UpsampleParams, "chap_upsample2x_bwd": UpsampleBwdParams,
    "chap_planar_to_cl": PlanarToClParams, "chap_channel_sum": ChanSumParams, "chap_cl_to_planar": ClToPlanarParams,
    "chap_ensemble_argmax": EnsembleParams, "chap_window_accumulate": WindowAccParams, "chap_window_finalize": WindowFinParams,
    "chap_mix_loss_fwd": MixLossParams, "chap_mix_loss_bwd": MixLossParams, "chap_pseudo_block": PseudoParams,
    "chap_kl_fwd_bwd": KlParams, "chap_l2_normalize": L2NormParams, "chap_perturb": AxpyParams,
    "chap_rand_uniform": RandParams, "chap_keep_mask": KeepMaskParams, "chap_chan_mask": ChanMaskParams,
    "chap_box_mix": BoxMixParams, "chap_box_mask": BoxMaskParams, "chap_largest_cc": LccParams,
    "chap_diff_mask": DiffMaskParams, "chap_sgd_step": SgdParams,
    "chap_sample_channel_sum": SampleChanSumParams, "chap_channel_drop": ChannelDropParams,
    "chap_fold_perturbed": FoldParams, "chap_grad_sim": GradSimParams, "chap_metrics": MetricsParams,
    "chap_augment2d": Augment2dParams, "chap_augment3d": Augment3dParams, "chap_augment3d_padded": Augment3dPadParams,
    "chap_window_gather": WindowGatherParams, "chap_window_accumulate_heads": WindowAccHeadsParams,
    "chap_mix_loss_multi_fwd": MixLossMultiParams, "chap_mix_loss_multi_bwd": MixLossMultiParams, "chap_bcp_mix": BcpMixParams,
    "chap_residual_fwd": ResidualParams, "chap_residual_bwd": ResidualBwdParams, "chap_grad_sum": GradSumParams,
}
# opt-in entry points declared in include/chap_hip_ext.h (same calling convention as _SIGS): not part of the default iteration
_SIGS_EXT = {"chap_sgd_ema_step": SgdEmaParams}
# the training monitor, declared in include/chap_hip_monitor.h (same calling convention): issued only with a chap_amd.monitor.StepMonitor attached
_SIGS_MONITOR = {"chap_monitor_accumulate": MonitorParams, "chap_monitor_accumulate_labels": MonitorLabelsParams,
                 "chap_monitor_finalize": MonitorFinalizeParams}
# the gradient guard, declared in include/chap_hip_guard.h (same calling convention): issued only with a chap_amd.guard.StepGuard attached
_SIGS_GUARD = {"chap_grad_norm": GradNormParams, "chap_sgd_guard_step": SgdGuardParams}
# Adam / AdamW, declared in include/chap_hip_optim.h (same calling convention): issued only by a chap_amd.train.FusedAdamW.  The table's name
# deliberately does NOT start with `_SIGS`: tests/test_launch_access_cpu.py walks every attribute of this module whose name does and wants a
# row in tests/launch_access.py for each entry, and that file names the four tables above one by one in struct_of.  Until the two entry
# points get their rows there (a test-only change) they stay out of that walk; _fn() below still looks the table up, so
# call("chap_adam_step", ...) gets its argtypes like every other entry point.
_OPTIM_SIGS = {"chap_adam_tick": AdamTickParams, "chap_adam_step": AdamParams}
# the mean teacher's consistency term, declared in include/chap_hip_teacher.h (same calling convention): issued only by a step built with
# teacher_consistency > 0.  Named like _OPTIM_SIGS and for the same reason.
_TEACHER_SIGS = {"chap_teacher_consistency": TeacherConsistencyParams}
# its uncertainty-aware form, declared in include/chap_hip_uncertainty.h (same calling convention): issued only by a step built with
# teacher_uncertainty > 0.  Named like _OPTIM_SIGS and for the same reason.
_UNCERTAINTY_SIGS = {"chap_teacher_uncertainty": TeacherUncertaintyParams, "chap_teacher_consistency_masked": TeacherConsistencyMaskedParams}
_SIZE_FNS = {"chap_pack_size": PackParams, "chap_conv_c1_bwd_ws": ConvC1BwdParams, "chap_wgrad_ws": WgradParams,
             "chap_lcc_ws": LccParams, "chap_metrics_ws": MetricsParams}

_lib = None


ABI_VERSION = 9            # CHAP_ABI_VERSION of include/chap_hip.h this binding mirrors (checked when the library is loaded)


class ChapError(RuntimeError):
    pass


def lib():
    """Load libchap_hip.so once.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ChapError("libchap_hip.so not built (%s missing): run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C chap_amd/csrc`.  chap_amd has no CPU fallback." % LIB_PATH)
        # The library is linked against the system ROCm runtime while PyTorch ships its own copy: the HIP runtime
        # PyTorch uses has to be initialised BEFORE this library is loaded (observed on the MI355X box: loaded the
        # other way round, the first kernel launch fails with "no ROCm-capable device is detected").
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()               # an error here is the load-order problem itself: let it propagate
            torch.cuda.current_stream()
        L = C.CDLL(LIB_PATH)
        L.chap_last_error.restype = C.c_char_p
        L.chap_abi_version.restype = C.c_int
        got = L.chap_abi_version()
        if got != ABI_VERSION:
            raise ChapError("libchap_hip.so has ABI version %d, this binding mirrors include/chap_hip.h version %d: rebuild "
                            "(`make -C chap_amd/csrc`) -- a stale library would be driven through mismatching structs" % (got, ABI_VERSION))
        _lib = L
    return _lib


_bound = {}


def _fn(name):
    """Bind an entry point on first use (argtypes from the tables above)."""
    fn = _bound.get(name)
    if fn is None:
        L = lib()
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise ChapError("libchap_hip.so does not export %s (stale build?)" % name)
        if name in _SIGS or name in _SIGS_EXT or name in _SIGS_MONITOR or name in _SIGS_GUARD or name in _OPTIM_SIGS or name in _TEACHER_SIGS or name in _UNCERTAINTY_SIGS:
            fn.restype, fn.argtypes = C.c_int, [C.POINTER(_SIGS.get(name) or _SIGS_EXT.get(name) or _SIGS_MONITOR.get(name) or _SIGS_GUARD.get(name)
                                                          or _OPTIM_SIGS.get(name) or _TEACHER_SIGS.get(name) or _UNCERTAINTY_SIGS[name]), _vp]
        else:
            fn.restype, fn.argtypes = _sz, [C.POINTER(_SIZE_FNS[name])]
        _bound[name] = fn
    return fn


def pack_describe(params):
    """chap_pack_describe: host-side, fills a PackEntry for chap_pack_multi."""
    L = lib()
    L.chap_pack_describe.restype = C.c_int
    L.chap_pack_describe.argtypes = [C.POINTER(PackParams), C.POINTER(PackEntry)]
    e = PackEntry()
    rc = L.chap_pack_describe(C.byref(params), C.byref(e))
    if rc != 0:
        raise ChapError("chap_pack_describe failed (%d): %s" % (rc, L.chap_last_error().decode()))
    return e


def pack_multi(entries_dev_ptr, n, max_total, stream):
    L = lib()
    L.chap_pack_multi.restype = C.c_int
    L.chap_pack_multi.argtypes = [_vp, _i32, _i64, _vp]
    rc = L.chap_pack_multi(_vp(entries_dev_ptr), n, max_total, _vp(stream))
    if rc != 0:
        raise ChapError("chap_pack_multi failed (%d): %s" % (rc, L.chap_last_error().decode()))


_holders = []       # the `held` lists of the open group regions, see hold()


def _drop_holder(h):
    for i, o in enumerate(_holders):
        if o is h:
            del _holders[i]
            return


class group:
    """`with group(stream) as g: ...lane 0...; g.next_lane(); ...lane 1...`: chap_group_begin / _next_lane / _end (chap_hip.h):
    the launches of the lanes are recorded and issued together, same-shaped ones as one grid.  `enabled=False` (or one lane
    only) makes it a no-op wrapper, which is how the executor switches grouping off (CHAP_GROUP=0)."""
    launched = 0            # grids issued by all regions so far (diagnostics / tests)
    held = None             # tensors allocated inside the open region (see hold())

    def __init__(self, stream, enabled=True):
        self.stream, self.enabled = stream, enabled

    def __enter__(self):
        if self.enabled:
            group.held = []
            _holders.append(group.held)
            L = lib()
            L.chap_group_begin.argtypes = [_vp]
            rc = L.chap_group_begin(_vp(self.stream))
            if rc != 0:
                raise ChapError("chap_group_begin failed (%d): %s" % (rc, L.chap_last_error().decode()))
        return self

    def next_lane(self):
        if self.enabled:
            rc = lib().chap_group_next_lane()
            if rc != 0:
                raise ChapError("chap_group_next_lane failed (%d): %s" % (rc, lib().chap_last_error().decode()))

    def __exit__(self, et, ev, tb):
        if self.enabled:
            if et is not None:                  # the body failed: drop what was recorded (its buffers are released with `held`), nothing is launched
                lib().chap_group_cancel()
                _drop_holder(group.held)
                group.held = None
                return False
            rc = lib().chap_group_end()
            _drop_holder(group.held)
            group.held = None
            if rc < 0:
                raise ChapError("chap_group_end failed (%d): %s" % (rc, lib().chap_last_error().decode()))
            group.launched += rc
        return False


def hold(t):
    """Inside a group region the lanes' kernels run CONCURRENTLY, later than the Python code that allocated their buffers: a
    temporary that Python drops (a workspace local to a wrapper, a gradient tensor consumed by the launches of its op) would go
    back to the caching allocator and could be handed to the NEXT lane of the same region -- two lanes of one grid writing the
    same memory.  Every tensor allocated on this path goes through hold(): kept alive until chap_group_end has issued the launches
    (stream order protects it from then on).  No-op outside a region."""
    for h in _holders:
        h.append(t)
    return t


def hold_empty(*a, **k):
    import torch
    return hold(torch.empty(*a, **k))


def hold_empty_like(*a, **k):
    import torch
    return hold(torch.empty_like(*a, **k))


def call(name, params, stream):
    rc = _fn(name)(C.byref(params), _vp(stream))
    if rc != 0:
        raise ChapError("%s failed (%d): %s" % (name, rc, lib().chap_last_error().decode()))


def size_of(name, params):
    return int(_fn(name)(C.byref(params)))
