"""ctypes binding of ``libcvf_hip.so`` (C ABI declared in ``include/cvf.h``).

PyTorch is plumbing here: it owns device memory and the stream; every compute call goes
through the C ABI with raw device pointers.  There is no CPU or eager-PyTorch fallback: if
the shared library is missing, or a call fails, this module raises.
"""

import ctypes as C
import os

import torch

TILE = 64
MAX_NETS = 8
MAX_LAYERS = 12
AUX_ROWS = 18
EF_HIDDEN_WIDTHS = (8, 12, 16, 20, 24, 32, 48, 64)   # hidden widths the eigenfunction kernels are instantiated for (csrc/ef_mfma.hip)


def ef_widths(n_hidden):
    """Hidden widths the eigenfunction kernels are instantiated for at this depth (csrc/ef_mfma.hip: ef_dispatch)."""
    if n_hidden >= 4:
        return (20, 32) if n_hidden <= 5 else ()
    return tuple(w for w in EF_HIDDEN_WIDTHS if w < 24 or n_hidden >= 2)   # (48 and 64: the plain 64-frame kernels, two or three hidden layers)


FEAT_ANGLE, FEAT_BOND, FEAT_DIHEDRAL, FEAT_POSITION = 0, 1, 2, 3
PP_IDENTITY, PP_ALIGN, PP_FACTORED, PP_FEATURES = 0, 1, 2, 3
FEATURES_MAX_SLOT, FEATURES_MAX_REF = 4096, 6144   # CVF_PP_FEATURES limits (include/cvf.h, csrc/k1_features.hip)
PP_ALIGN_CONTIG, PP_PURE_POSITION, PP_SLOT_BATCHED = 1, 2, 4
# cvf_align_feature_route (include/cvf.h): slice / pipe codes are the base + NI
K1_ROUTE_SMALL, K1_ROUTE_GATHER_CONTIG, K1_ROUTE_GATHER, K1_ROUTE_CAPTURE_VEC4, K1_ROUTE_CAPTURE = 0, 1, 2, 3, 4
K1_ROUTE_SLICE, K1_ROUTE_PIPE = 10, 20
# cvf_metric_route (include/cvf.h): kernel families of cvf_metric_apply[_stats]
METRIC_IDENTITY, METRIC_FACTORED, METRIC_FEATURES, METRIC_ALIGN, METRIC_PURE, METRIC_ROWS = range(6)
# cvf_align_feature_deriv_route (include/cvf.h): the call asked about, and the kernel families of the answer
DERIV_VJP, DERIV_VJP_ROWS, DERIV_JVP, DERIV_HVP, DERIV_FEATURES_FWD, DERIV_FEATURES_METRIC = range(6)
DERIV_IDENTITY, DERIV_FEATURES, DERIV_SMALL, DERIV_LARGE = range(4)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcvf_hip.so")


class PPDesc(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_coord", C.c_int32), ("n_align", C.c_int32), ("n_rec", C.c_int32),
                ("d_r", C.c_int32), ("use_angle_value", C.c_int32), ("has_position", C.c_int32), ("flags", C.c_int32),
                ("align_idx", C.c_void_p), ("ref_c", C.c_void_p), ("rec", C.c_void_p),
                ("atom_align", C.c_void_p), ("atom_slot", C.c_void_p), ("rec_slot", C.c_void_p), ("slot_atom", C.c_void_p), ("n_slot", C.c_int32),
                ("n_rec_slot", C.c_int32), ("align_w", C.c_void_p), ("mrec", C.c_void_p), ("slot_row", C.c_void_p),
                ("n_mrec", C.c_int32), ("n_ref", C.c_int32)]


class MetricPlan(C.Structure):
    _fields_ = [("family", C.c_int32), ("F", C.c_int32), ("waves", C.c_int32), ("geo_pre", C.c_int32), ("multi", C.c_int32),
                ("npb", C.c_int32), ("nets_per_wg", C.c_int32), ("fused", C.c_int32), ("fused_rows", C.c_int32),
                ("reserved", C.c_int32), ("lds_bytes", C.c_int64), ("grid", C.c_int64)]


class DerivPlan(C.Structure):
    _fields_ = [("family", C.c_int32), ("tables_lds", C.c_int32), ("q_lds", C.c_int32), ("u_lds", C.c_int32), ("weighted", C.c_int32),
                ("vec4", C.c_int32), ("lg", C.c_int32), ("rows_per_launch", C.c_int32), ("launches", C.c_int32),
                ("reserved", C.c_int32), ("lds_bytes", C.c_int64), ("grid", C.c_int64)]


class MLPDesc(C.Structure):
    _fields_ = [("n_nets", C.c_int32), ("n_layers", C.c_int32), ("dims", C.c_int32 * (MAX_LAYERS + 1)),
                ("act", C.c_int32 * MAX_LAYERS), ("w_off", (C.c_int32 * MAX_LAYERS) * MAX_NETS),
                ("b_off", (C.c_int32 * MAX_LAYERS) * MAX_NETS), ("n_params", C.c_int32)]


class EFCfg(C.Structure):
    _fields_ = [("k", C.c_int32), ("lag_idx", C.c_int32), ("sort_eigvals", C.c_int32), ("iso_metric", C.c_int32),
                ("alpha", C.c_double), ("beta", C.c_double), ("dt", C.c_double), ("eig_w", C.c_double * MAX_NETS)]


class AdamArgs(C.Structure):
    _fields_ = [("theta", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("step_count", C.c_void_p), ("mlp", C.POINTER(MLPDesc)),
                ("packed", C.c_void_p), ("lr_dev", C.c_void_p)]


_SIGNATURES = {
    "cvf_version": (C.c_int, []),
    "cvf_last_error": (C.c_char_p, []),
    "cvf_ef_nstats": (C.c_int, [C.c_int, C.c_int]),
    "cvf_align_feature_scratch_bytes": (C.c_int64, [C.POINTER(PPDesc), C.c_int64]),
    "cvf_align_feature_fwd": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "cvf_align_feature_route": (C.c_int, [C.POINTER(PPDesc), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "cvf_align_feature_vjp": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cvf_align_feature_vjp_rows": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "cvf_align_feature_jvp": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cvf_align_feature_hvp": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "cvf_align_feature_deriv_route": (C.c_int, [C.POINTER(PPDesc), C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(DerivPlan)]),
    "cvf_metric_gram": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_metric_apply": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_metric_route": (C.c_int, [C.POINTER(PPDesc), C.c_int64, C.c_int, C.c_int, C.POINTER(MetricPlan)]),
    "cvf_metric_stats_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int]),
    "cvf_metric_apply_stats": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EFCfg), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_metric_dense_doubles": (C.c_int64, [C.POINTER(PPDesc)]),
    "cvf_metric_dense_tensors": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_pack_floats": (C.c_int64, [C.POINTER(MLPDesc)]),
    "cvf_ef_pack": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_mlp_fwd": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "cvf_ef_saved_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64]),
    "cvf_ef_fwd_metric_supported": (C.c_int, [C.POINTER(MLPDesc), C.POINTER(PPDesc)]),
    "cvf_ef_fused_stats_rows": (C.c_int64, [C.POINTER(MLPDesc), C.POINTER(PPDesc), C.c_int64, C.c_int]),
    "cvf_ef_stats_finish_rows": (C.c_int, [C.POINTER(EFCfg), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_align_fwd_metric_supported": (C.c_int, [C.POINTER(MLPDesc), C.POINTER(PPDesc)]),
    "cvf_ef_align_fwd_metric_stats": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p,
                                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(EFCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "cvf_ef_fwd_metric_stats": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(EFCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_supported": (C.c_int, [C.POINTER(MLPDesc), C.POINTER(PPDesc)]),
    "cvf_ef16_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int]),
    "cvf_ef16_saved_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64]),
    "cvf_ef16_rows": (C.c_int64, [C.c_int64]),
    "cvf_ef16_finish": (C.c_int, [C.POINTER(EFCfg), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_front": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EFCfg), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_align_rows_floats": (C.c_int64, [C.c_int64]),
    "cvf_ef16_align_rows": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "cvf_ef16_align_rows_tile": (C.c_int, [C.POINTER(PPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_front_rows": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EFCfg), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_backward": (C.c_int, [C.POINTER(EFCfg), C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "cvf_ef16_front_transfer": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_transfer_rows": (C.c_int64, [C.c_int64, C.c_int]),
    "cvf_ef16_front_transfer_rows": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p,
                                               C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef16_backward_transfer": (C.c_int, [C.POINTER(EFCfg), C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "cvf_comm_unique_id_bytes": (C.c_int, []),
    "cvf_comm_unique_id": (C.c_int, [C.c_void_p]),
    "cvf_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]),
    "cvf_comm_allreduce_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cvf_comm_allreduce_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cvf_comm_destroy": (C.c_int, [C.c_void_p]),
    "cvf_p2p_handle_bytes": (C.c_int, []),
    "cvf_p2p_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "cvf_p2p_connect": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cvf_p2p_allreduce_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cvf_p2p_allreduce_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cvf_p2p_error": (C.c_int, [C.c_void_p]),
    "cvf_p2p_destroy": (C.c_int, [C.c_void_p]),
    "cvf_ef16_finish_dp": (C.c_int, [C.POINTER(EFCfg), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_stats_dp": (C.c_int, [C.POINTER(EFCfg), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_loss_dp": (C.c_int, [C.POINTER(EFCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_probe_stream_out_floats": (C.c_int64, [C.c_int, C.c_int64]),
    "cvf_probe_stream": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cvf_p2p_exchange_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cvf_slab_reduce_dp": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(AdamArgs), C.c_void_p, C.c_void_p]),
    "cvf_ef_stats_scratch_doubles": (C.c_int64, [C.c_int, C.c_int]),
    "cvf_ef_stats": (C.c_int, [C.POINTER(EFCfg), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_loss": (C.c_int, [C.POINTER(EFCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_backward_slab_rows": (C.c_int64, [C.c_int64]),
    "cvf_ef_backward": (C.c_int, [C.POINTER(EFCfg), C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "cvf_ef_general_supported": (C.c_int, [C.POINTER(MLPDesc)]),
    "cvf_ef_general_slab_rows": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64]),
    "cvf_ef_general_saved_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64, C.c_int]),
    "cvf_ef_general_fwd": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "cvf_ef_general_backward": (C.c_int, [C.POINTER(EFCfg), C.POINTER(MLPDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "cvf_ef_general_shared_supported": (C.c_int, [C.POINTER(MLPDesc), C.c_int]),
    "cvf_ef_general_shared_slab_rows": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64, C.c_int]),
    "cvf_ef_general_shared_saved_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64, C.c_int]),
    "cvf_ef_general_shared_fwd": (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "cvf_ef_general_shared_backward": (C.c_int, [C.POINTER(EFCfg), C.POINTER(MLPDesc), C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "cvf_ef_general_shared_transfer_supported": (C.c_int, [C.POINTER(MLPDesc), C.c_int]),
    "cvf_ef_general_shared_transfer_slab_rows": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64, C.c_int]),
    "cvf_ef_general_shared_transfer_saved_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64, C.c_int]),
    "cvf_ef_general_shared_transfer_fwd": (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]),
    "cvf_ef_general_shared_transfer_backward": (C.c_int, [C.POINTER(EFCfg), C.POINTER(MLPDesc), C.c_int, C.c_void_p, C.c_int64,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_ef_align_fwd": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PPDesc), C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_slab_reduce": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(AdamArgs), C.c_void_p]),
    "cvf_ae_scratch_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64]),
    "cvf_ae_step": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamArgs), C.c_void_p]),
    "cvf_ae_step_route": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "cvf_ae_general_supported": (C.c_int, [C.POINTER(MLPDesc)]),
    "cvf_ae_general_scratch_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64]),
    "cvf_ae_general_step": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamArgs), C.c_void_p]),
    "cvf_regae_scratch_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int64]),
    "cvf_regae_forward": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_regae_backward": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamArgs),
                                     C.c_void_p]),
    "cvf_regae_forward_keep": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_regae_backward_reuse": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamArgs),
                                     C.c_void_p]),
    "cvf_regae_enc_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_regae_loss_row": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_double,
                                     C.c_double, C.c_void_p, C.c_void_p]),
    "cvf_mlp_eval_rows": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cvf_cv_nets_supported": (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.c_int]),
    "cvf_cv_nets_scratch_floats": (C.c_int64, [C.POINTER(MLPDesc), C.c_int, C.c_int64, C.c_int]),
    "cvf_cv_nets_eval": (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cvf_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_double,
                                C.c_double, C.c_double, C.c_void_p, C.POINTER(MLPDesc), C.c_void_p, C.c_void_p]),
    "cvf_sgd_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.POINTER(MLPDesc), C.c_void_p,
                               C.c_void_p]),
}

# the per-layer route of RegAutoEncoderTask takes the argument lists of the fused calls
_SIGNATURES["cvf_regae_route"] = (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.POINTER(C.c_int64)])
_SIGNATURES["cvf_regae_general_supported"] = (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.c_int])
_SIGNATURES["cvf_regae_general_scratch_floats"] = _SIGNATURES["cvf_regae_scratch_floats"]
_SIGNATURES["cvf_regae_general_forward"] = _SIGNATURES["cvf_regae_forward"]
_SIGNATURES["cvf_regae_general_backward"] = _SIGNATURES["cvf_regae_backward"]
_SIGNATURES["cvf_regae_general_backward_reuse"] = _SIGNATURES["cvf_regae_backward"]
# ... and its twin for decoder / regulariser nets of different depths adds (n_dec_layers, n_reg_layers) behind n_enc_layers


def _with_depths(sig):
    res, args = sig
    at = max(i for i, a in enumerate(args) if a is C.c_int) + 1       # n_enc_layers is the last int of these lists
    return res, args[:at] + [C.c_int, C.c_int] + args[at:]


_SIGNATURES["cvf_regae_ragged_supported"] = _with_depths(_SIGNATURES["cvf_regae_general_supported"])
_SIGNATURES["cvf_regae_ragged_scratch_floats"] = (C.c_int64, [C.POINTER(MLPDesc), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int])
_SIGNATURES["cvf_regae_ragged_forward"] = _with_depths(_SIGNATURES["cvf_regae_forward"])
_SIGNATURES["cvf_regae_ragged_backward"] = _with_depths(_SIGNATURES["cvf_regae_backward"])
_SIGNATURES["cvf_regae_ragged_backward_reuse"] = _with_depths(_SIGNATURES["cvf_regae_backward"])
# the isotropic-metric forms of the two front calls take the arguments of their general twins
_SIGNATURES["cvf_ef16_front_iso"] = _SIGNATURES["cvf_ef16_front"]
_SIGNATURES["cvf_ef16_front_rows_iso"] = _SIGNATURES["cvf_ef16_front_rows"]


class CVModel(C.Structure):
    """``cvf_cv_model`` (include/cvf.h): what ``cvf_cv_file_bind`` fills - both descriptors and theta over one device buffer."""
    _fields_ = [("mlp", MLPDesc), ("pp", PPDesc), ("theta", C.c_void_p), ("upto_layer", C.c_int32), ("k", C.c_int32)]


# xi and d xi / d x per frame in one launch (csrc/cv_frame.hip), and the self-contained model file (csrc/cv_file.hip)
_SIGNATURES["cvf_cv_frame_supported"] = (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.POINTER(PPDesc)])
_SIGNATURES["cvf_cv_frame_eval"] = (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_int, C.POINTER(PPDesc), C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_SIGNATURES["cvf_cv_file_device_bytes"] = (C.c_int64, [C.c_char_p, C.c_int64])
_SIGNATURES["cvf_cv_file_bind"] = (C.c_int, [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(CVModel), C.c_void_p])
# the same in one launch for frames of any size, one workgroup per frame (csrc/cv_frame_large.hip)
_SIGNATURES["cvf_cv_frame_large_supported"] = (C.c_int, [C.POINTER(MLPDesc), C.c_int, C.POINTER(PPDesc)])
_SIGNATURES["cvf_cv_frame_large_lds_bytes"] = (C.c_int64, [C.POINTER(MLPDesc), C.c_int, C.POINTER(PPDesc), C.POINTER(C.c_int32)])
_SIGNATURES["cvf_cv_frame_large_eval"] = _SIGNATURES["cvf_cv_frame_eval"]
# form C, k scalar chains on one trunk: the argument lists of the namesakes, n_shared for upto_layer
_SIGNATURES["cvf_cv_nets_shared_supported"] = _SIGNATURES["cvf_cv_nets_supported"]
_SIGNATURES["cvf_cv_nets_shared_scratch_floats"] = _SIGNATURES["cvf_cv_nets_scratch_floats"]
_SIGNATURES["cvf_cv_nets_shared_eval"] = _SIGNATURES["cvf_cv_nets_eval"]
_SIGNATURES["cvf_cv_frame_shared_supported"] = _SIGNATURES["cvf_cv_frame_supported"]
_SIGNATURES["cvf_cv_frame_shared_eval"] = _SIGNATURES["cvf_cv_frame_eval"]
_SIGNATURES["cvf_cv_frame_large_shared_supported"] = _SIGNATURES["cvf_cv_frame_large_supported"]
_SIGNATURES["cvf_cv_frame_large_shared_lds_bytes"] = _SIGNATURES["cvf_cv_frame_large_lds_bytes"]
_SIGNATURES["cvf_cv_frame_large_shared_eval"] = _SIGNATURES["cvf_cv_frame_large_eval"]
_SIGNATURES["cvf_cv_file_n_shared"] = (C.c_int, [C.c_char_p, C.c_int64])

# bias energy and forces along the CV in one launch, in the MD engine's arrays (csrc/cv_bias.hip)
BIAS_MAX_TERMS = 16
BIAS_HARMONIC, BIAS_UPPER_WALL, BIAS_LOWER_WALL, BIAS_LINEAR, BIAS_TABLE = range(5)
BIAS_KINDS = {"harmonic": BIAS_HARMONIC, "upper_wall": BIAS_UPPER_WALL, "lower_wall": BIAS_LOWER_WALL, "linear": BIAS_LINEAR,
              "table": BIAS_TABLE}


class BiasTerm(C.Structure):
    """``cvf_bias_term`` (include/cvf.h)."""
    _fields_ = [("kind", C.c_int32), ("cv", C.c_int32), ("kappa", C.c_float), ("center", C.c_float), ("tab_off", C.c_int32),
                ("n_nodes", C.c_int32), ("lo", C.c_float), ("inv_h", C.c_float),
                # a joint grid on (cv, cv2) where n_nodes2 >= 2; n_nodes2 == 0: the 1-D table
                ("cv2", C.c_int32), ("n_nodes2", C.c_int32), ("lo2", C.c_float), ("inv_h2", C.c_float)]


class BiasDesc(C.Structure):
    """``cvf_bias_desc`` (include/cvf.h): ``table`` is a device pointer to ``n_table`` floats, read at launch time."""
    _fields_ = [("n_terms", C.c_int32), ("n_table", C.c_int32), ("term", BiasTerm * BIAS_MAX_TERMS), ("table", C.c_void_p)]


class MDLayout(C.Structure):
    """``cvf_md_layout`` (include/cvf.h): where the CV's atoms lie in the engine's position and force arrays."""
    _fields_ = [("atom_index", C.c_void_p), ("atom_stride", C.c_int32), ("reserved", C.c_int32), ("x_frame_stride", C.c_int64),
                ("f_frame_stride", C.c_int64)]


_SIGNATURES["cvf_cv_bias_check"] = (C.c_int, [C.POINTER(BiasDesc), C.c_int])
_SIGNATURES["cvf_cv_frame_bias_supported"] = _SIGNATURES["cvf_cv_frame_supported"]
_SIGNATURES["cvf_cv_frame_bias_eval"] = (C.c_int, [C.POINTER(MLPDesc), C.c_void_p, C.c_int, C.POINTER(PPDesc), C.POINTER(BiasDesc),
                                                   C.POINTER(MDLayout), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p])
_SIGNATURES["cvf_cv_frame_bias_shared_supported"] = _SIGNATURES["cvf_cv_frame_supported"]
_SIGNATURES["cvf_cv_frame_bias_shared_eval"] = _SIGNATURES["cvf_cv_frame_bias_eval"]
_SIGNATURES["cvf_cv_frame_large_bias_supported"] = _SIGNATURES["cvf_cv_frame_supported"]
_SIGNATURES["cvf_cv_frame_large_bias_eval"] = _SIGNATURES["cvf_cv_frame_bias_eval"]
_SIGNATURES["cvf_cv_frame_large_bias_shared_supported"] = _SIGNATURES["cvf_cv_frame_supported"]
_SIGNATURES["cvf_cv_frame_large_bias_shared_eval"] = _SIGNATURES["cvf_cv_frame_bias_eval"]


# periodic cells in the bias launches: whole molecules and the virial (csrc/cv_bias.hip, csrc/cvf_cell.hpp)
class MDCell(C.Structure):
    """``cvf_md_cell`` (include/cvf.h): ``cell`` is a device pointer to 9 floats per frame (lower-triangular rows), read at launch
    time; ``virial_rows`` a device pointer to ``[B][9]`` floats; either may be NULL, not both."""
    _fields_ = [("cell", C.c_void_p), ("cell_frame_stride", C.c_int64), ("virial_rows", C.c_void_p)]


for _name in ("cvf_cv_frame_bias", "cvf_cv_frame_bias_shared", "cvf_cv_frame_large_bias", "cvf_cv_frame_large_bias_shared"):
    _SIGNATURES[_name + "_cell_supported"] = _SIGNATURES["cvf_cv_frame_supported"]
    _SIGNATURES[_name + "_cell_eval"] = (C.c_int, _SIGNATURES["cvf_cv_frame_bias_eval"][1] + [C.POINTER(MDCell)])
_SIGNATURES["cvf_md_make_whole"] = (C.c_int, [C.POINTER(MDLayout), C.POINTER(MDCell), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                              C.c_void_p])

# hill deposition into a table term on the device (csrc/cv_bias_hills.hip)
HILL_CHUNK = 64   # CVF_HILL_CHUNK: the hills a node launch stages through LDS at a time


class HillDesc(C.Structure):
    """``cvf_hill_desc`` (include/cvf.h)."""
    _fields_ = [("term", C.c_int32), ("reserved", C.c_int32), ("height", C.c_float), ("sigma", C.c_float), ("sigma2", C.c_float),
                ("inv_kdt", C.c_float)]


_SIGNATURES["cvf_cv_bias_deposit"] = (C.c_int, [C.POINTER(BiasDesc), C.c_int, C.POINTER(HillDesc), C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_void_p])
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib():
    """The loaded shared library; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"colvarsfinder: HIP extension not built ({LIB_PATH} missing). Run `python __graft_entry__.py` "
                "or `make -C colvars-finder_amd/csrc`. There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().cvf_last_error().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "HIP path needs contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def align_scratch(desc, B, device):
    """Scratch buffer cvf_align_feature_fwd needs for B frames (None for small molecules)."""
    n = lib().cvf_align_feature_scratch_bytes(desc, B)
    return torch.empty((n + 7) // 8, device=device, dtype=torch.float64) if n > 0 else None


def ntiles(B):
    return (B + TILE - 1) // TILE


def require_gpu(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(
            "colvarsfinder (MI355X build) computes on the GPU only: pass device=torch.device('cuda'). "
            "There is no CPU path in this package.")
    if not torch.cuda.is_available():
        raise RuntimeError("colvarsfinder: no HIP device visible")
    lib()
    return device


def upload_f32(a, device, chunk_bytes=64 << 20):
    """Host array -> contiguous fp32 device tensor (trajectory ingestion into the HBM-resident shard).

    A pageable ``tensor.to(device)`` stages through the driver's own bounce buffer.  Here an fp32 C-contiguous source is
    page-locked in place (``hipHostRegister``) and copied by one DMA; anything else (fp64 text trajectories, strided
    arrays) is converted chunk by chunk into two pinned staging buffers whose copies run on a side stream while the
    next chunk is converted.  Small arrays take the plain path."""
    t = torch.as_tensor(a)
    if t.is_cuda:
        return t.to(device=device, dtype=torch.float32).contiguous()
    n = t.numel()
    if n * 4 <= (8 << 20) or not torch.cuda.is_available():
        return t.to(dtype=torch.float32).contiguous().to(device)
    out = torch.empty(tuple(t.shape), device=device, dtype=torch.float32)
    if t.dtype == torch.float32 and t.is_contiguous():
        rt = torch.cuda.cudart()
        if int(rt.cudaHostRegister(t.data_ptr(), n * 4, 0)) == 0:
            try:
                out.copy_(t, non_blocking=True)
                torch.cuda.current_stream(device).synchronize()
            finally:
                rt.cudaHostUnregister(t.data_ptr())
            return out
    src, dst = t.reshape(-1), out.reshape(-1)
    ce = max(1, chunk_bytes // 4)
    bufs = [torch.empty(ce, dtype=torch.float32).pin_memory() for _ in range(2)]
    done = [None, None]
    side = torch.cuda.Stream(device)
    # `out` came from the caching allocator on the current stream: work queued there may still use the block it recycled
    side.wait_stream(torch.cuda.current_stream(device))
    for i, s0 in enumerate(range(0, n, ce)):
        e0, b = min(s0 + ce, n), bufs[i % 2]
        if done[i % 2] is not None:
            done[i % 2].synchronize()            # the copy that last used this staging buffer has finished
        b[:e0 - s0].copy_(src[s0:e0])            # host side: gather / convert into page-locked memory
        with torch.cuda.stream(side):
            dst[s0:e0].copy_(b[:e0 - s0], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
            done[i % 2] = ev
    torch.cuda.current_stream(device).wait_stream(side)
    side.synchronize()
    return out
