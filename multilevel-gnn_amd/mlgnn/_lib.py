"""ctypes binding of the C ABI in include/mlgnn.h.  Fails loudly when the library is missing."""
import atexit
import ctypes
import os
import sys

import torch

# (MLGNN_LIB: a development override for same-box A/B runs of kernel variants, tools/build_variant.py)
LIB = os.environ.get("MLGNN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmlgnn.so")

_c = ctypes
_P = _c.c_void_p
_I64 = _c.c_int64
_INT = _c.c_int
_F = _c.c_float

# name -> (restype, argtypes); mirrors include/mlgnn.h one to one (tests/test_abi.py compares names and types)
SIGNATURES = {
    "mlgnn_version": (_INT, []),
    "mlgnn_csr_aggregate_bwd_workspace_floats": (_I64, [_I64, _I64, _INT, _INT, _INT, _INT]),
    "mlgnn_csr_aggregate_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                       _I64, _I64, _INT, _INT, _INT, _INT, _INT, _F, _F, _P, _P, _F, _INT, _P, _P]),
    "mlgnn_csr_aggregate_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                       _P, _P, _P, _P, _I64,
                                       _I64, _I64, _INT, _INT, _INT, _INT, _INT, _INT, _F, _F, _P, _P, _F, _INT, _INT, _P,
                                       _P, _P, _P]),
    "mlgnn_power_bwd_prologue_workspace_floats": (_I64, []),
    "mlgnn_power_bwd_prologue": (_INT, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_embedding_bwd": (_INT, [_P, _P, _P, _P, _I64, _I64, _INT, _P]),
    "mlgnn_max_table_grad_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_max_table_grad_workspace_floats": (_I64, [_I64, _I64, _I64]),
    "mlgnn_max_table_grad": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_max_table_grad_by_type": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_csr_aggregate_bwd_slots_offset_floats": (_I64, [_I64, _I64, _INT]),
    "mlgnn_max_sparse_supported": (_INT, [_I64, _I64]),
    "mlgnn_max_sparse_records": (_I64, [_I64, _I64, _I64]),
    "mlgnn_max_winners": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _P]),
    "mlgnn_max_sparse_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _I64, _I64, _P]),
    "mlgnn_max_sparse_table_grad": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_segment_project_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_segment_project_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                         _I64, _I64, _I64, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_layernorm_bwd_workspace_floats": (_I64, [_I64, _I64, _INT]),
    "mlgnn_layernorm_act_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _I64, _I64, _F, _INT, _INT, _P]),
    "mlgnn_layernorm_act_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _F, _I64, _I64, _INT, _INT, _P]),
    "mlgnn_linear_wgrad_workspace_floats": (_I64, [_I64, _I64, _I64, _INT]),
    "mlgnn_tallgemm_bf16_shift_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_tallgemm_bf16_shift": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_linear_bwd_supported": (_INT, [_I64, _I64, _I64, _INT]),
    "mlgnn_linear_bwd_workspace_floats": (_I64, [_I64, _I64, _I64, _INT]),
    "mlgnn_linear_bwd": (_INT, [_P, _P, _P, _P, _INT, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64,
                                _I64, _I64, _I64, _P]),
    "mlgnn_linear_wgrad": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_diffpool_fwd_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_diffpool_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _P]),
    "mlgnn_coo_to_csr_workspace_bytes": (_I64, [_I64, _I64]),
    "mlgnn_coo_to_csr": (_INT, [_P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "mlgnn_msgnorm_bwd_workspace_floats": (_I64, [_I64, _I64]),
    "mlgnn_msgnorm_add_fwd": (_INT, [_P, _P, _P, _P, _I64, _I64, _INT, _P]),
    "mlgnn_msgnorm_add_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_diffpool_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _P]),
    "mlgnn_edge_table_to_csr": (_INT, [_P, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P]),
    "mlgnn_dense_sage_supported": (_INT, [_I64, _I64, _I64, _INT]),
    "mlgnn_dense_sage_bwd_workspace_floats": (_I64, [_I64, _I64, _I64]),
    "mlgnn_dense_sage_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P]),
    "mlgnn_dense_sage_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64,
                                    _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P]),
    "mlgnn_segment_pool_workspace_bytes": (_I64, [_I64, _I64]),
    "mlgnn_segment_pool_fwd": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _INT, _P]),
    "mlgnn_tallgemm_supported": (_INT, [_I64, _I64, _I64, _INT]),
    "mlgnn_tallgemm_workspace_bytes": (_I64, [_I64, _I64, _INT]),
    "mlgnn_tallgemm_nt": (_INT, [_P, _P, _INT, _P, _P, _P, _INT, _P, _P, _F, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_tallgemm_nt_shift_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_tallgemm_nt_shift": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_tallgemm_lnin_postln_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_tallgemm_lnin_postln": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _INT, _P, _P, _P, _P, _P, _I64,
                                          _I64, _I64, _I64, _P]),
    "mlgnn_tallgemm_lnbwd_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_tallgemm_lnbwd_workspace_bytes": (_I64, [_I64, _I64]),
    "mlgnn_tallgemm_lnbwd": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_csr_replicate": (_INT, [_P] * 14 + [_I64, _I64, _I64, _P]),
    "mlgnn_sage_rewrite": (_INT, [_P, _P, _I64, _I64, _I64, _P, _P, _P]),
    "mlgnn_tallgemm_dual_supported": (_INT, [_I64, _I64, _I64, _I64]),
    "mlgnn_tallgemm_dual": (_INT, [_P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_transpose_batched": (_INT, [_P, _P, _I64, _I64, _I64, _P]),
    "mlgnn_sage_fold_fwd": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _INT, _P]),
    "mlgnn_sage_fold_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _I64, _I64, _INT, _P]),
    "mlgnn_leaky_relu_bwd": (_INT, [_P, _P, _P, _F, _P, _P, _I64, _I64, _P]),
    "mlgnn_node_embed_fwd": (_INT, [_P, _P, _P, _P, _I64, _I64, _I64, _P]),
    "mlgnn_node_embed_bwd": (_INT, [_P, _P, _P, _I64, _I64, _I64, _P]),
    "mlgnn_narrow_linear_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_narrow_linear_bwd_workspace_floats": (_I64, [_I64, _I64]),
    "mlgnn_narrow_linear_fwd": (_INT, [_P, _P, _P, _P, _I64, _I64, _I64, _P]),
    "mlgnn_narrow_linear_bwd": (_INT, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_skinny_linear_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_skinny_linear_fwd_workspace_floats": (_I64, [_I64, _I64, _I64]),
    "mlgnn_skinny_linear_fwd": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_skinny_linear_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _P]),
    "mlgnn_gat_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_gat_scores": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _P]),
    "mlgnn_gat_aggregate_fwd": (_INT, [_P] * 9 + [_I64, _I64, _I64, _I64, _F, _F, _P]),
    "mlgnn_gat_bwd_workspace_floats": (_I64, [_I64, _I64, _I64, _I64]),
    "mlgnn_gat_aggregate_bwd": (_INT, [_P] * 18 + [_I64, _I64, _I64, _I64, _I64, _F, _F, _P]),
    "mlgnn_mha_supported": (_INT, [_I64, _I64, _I64, _I64]),
    "mlgnn_mha_fwd": (_INT, [_P, _P, _F, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_mha_bwd_workspace_floats": (_I64, [_I64, _I64, _I64, _I64]),
    "mlgnn_mha_bwd": (_INT, [_P, _P, _P, _P, _P, _F, _P, _P, _I64, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_conv2d_supported": (_INT, [_I64] * 6),
    "mlgnn_conv2d_fwd": (_INT, [_P, _P, _P, _P, _INT] + [_I64] * 6 + [_P]),
    "mlgnn_conv2d_bwd_workspace_floats": (_I64, [_I64] * 6),
    "mlgnn_conv2d_bwd": (_INT, [_P, _P, _P, _P, _INT, _P, _P, _P, _P, _I64] + [_I64] * 6 + [_P]),
    "mlgnn_pool_flatten_supported": (_INT, [_I64] * 6),
    "mlgnn_pool_flatten_fwd": (_INT, [_P, _P, _F, _P, _P, _P] + [_I64] * 6 + [_P]),
    "mlgnn_pool_flatten_bwd": (_INT, [_P, _P, _F, _P, _P, _I64] + [_I64] * 6 + [_P]),
    "mlgnn_mmd_supported": (_INT, [_I64] * 3),
    "mlgnn_mmd_fwd": (_INT, [_P, _P, _P, _P, _INT, _F, _F] + [_I64] * 3 + [_P]),
    "mlgnn_mmd_bwd": (_INT, [_P, _P, _P, _P, _INT, _F, _F] + [_I64] * 3 + [_P]),
    "mlgnn_pathway_decoder_supported": (_INT, [_I64] * 6),
    "mlgnn_pathway_decoder_fwd": (_INT, [_P] * 9 + [_I64] * 6 + [_P]),
    "mlgnn_pathway_decoder_bwd": (_INT, [_P] * 13 + [_I64] * 6 + [_P]),
    "mlgnn_vq_supported": (_INT, [_I64] * 3),
    "mlgnn_vq_fwd": (_INT, [_P] * 6 + [_F] + [_I64] * 3 + [_P]),
    "mlgnn_vq_bwd": (_INT, [_P] * 7 + [_F] + [_I64] * 3 + [_P]),
    "mlgnn_vae_latent_supported": (_INT, [_I64] * 3),
    "mlgnn_vae_latent_fwd": (_INT, [_P] * 10 + [_I64] * 3 + [_P]),
    "mlgnn_vae_latent_bwd": (_INT, [_P] * 16 + [_I64] * 4 + [_P]),
    "mlgnn_criterion_supported": (_INT, [_I64] * 2),
    "mlgnn_criterion_workspace": (_I64, [_I64] * 2),
    "mlgnn_criterion_fwd": (_INT, [_P, _P, _P, _I64, _P, _F, _INT, _P, _I64, _P, _P, _P, _I64, _I64, _P]),
    "mlgnn_criterion_bwd": (_INT, [_P, _P, _P, _I64, _P, _P, _P, _P, _F, _INT, _P, _P, _I64, _I64, _P]),
    "mlgnn_mutual_info_supported": (_INT, [_I64, _I64, _INT, _INT]),
    "mlgnn_mutual_info_cd": (_INT, [_P, _P, _P, _c.c_double, _P, _P, _I64, _I64, _INT, _INT, _P]),
    "mlgnn_mutual_info_cc_supported": (_INT, [_I64, _I64, _INT]),
    "mlgnn_mutual_info_cc": (_INT, [_P, _P, _P, _c.c_double, _P, _P, _P, _I64, _I64, _INT, _P]),
    "mlgnn_edge_mi_supported": (_INT, [_I64, _I64, _I64, _INT, _INT, _INT]),
    "mlgnn_edge_mi": (_INT, [_P, _P, _P, _P, _P, _c.c_double, _P, _P, _P, _I64, _I64, _I64, _INT, _INT, _P]),
    "mlgnn_edge_mi_cc_supported": (_INT, [_I64, _I64, _I64, _INT, _INT]),
    "mlgnn_edge_mi_cc": (_INT, [_P, _P, _P, _P, _P, _c.c_double, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_kraskov_mi_supported": (_INT, [_I64, _I64, _I64, _INT, _INT]),
    "mlgnn_kraskov_mi": (_INT, [_P, _P, _P, _P, _c.c_double, _P, _P, _P, _P, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_pathway_pca_supported": (_INT, [_I64] * 4 + [_INT]),
    "mlgnn_pathway_pca_workspace_bytes": (_I64, [_I64] * 4),
    "mlgnn_pathway_pca": (_INT, [_P] * 10 + [_I64] * 6 + [_INT, _P]),
    "mlgnn_pathway_order_supported": (_INT, [_I64] * 3),
    "mlgnn_pathway_order_workspace_bytes": (_I64, [_I64] * 3),
    "mlgnn_pathway_order": (_INT, [_P] + [_I64] * 5 + [_P] * 4 + [_I64, _P]),
    "mlgnn_eval_metrics_supported": (_INT, [_I64] * 4),
    "mlgnn_eval_metrics_workspace_bytes": (_I64, [_I64] * 4),
    "mlgnn_eval_metrics": (_INT, [_P] * 5 + [_I64] * 4 + [_P] * 3 + [_I64, _P]),
    "mlgnn_survival_screen_supported": (_INT, [_I64] * 3 + [_INT]),
    "mlgnn_survival_screen_workspace_bytes": (_I64, [_I64] * 3 + [_INT]),
    "mlgnn_survival_screen": (_INT, [_P, _INT, _I64, _I64] + [_P] * 5 + [_I64] * 3 + [_INT] + [_P] * 4 + [_I64, _P]),
    "mlgnn_pathway_conv_supported": (_INT, [_I64] * 3),
    "mlgnn_pathway_conv_fwd": (_INT, [_P] * 9 + [_I64] * 4 + [_INT, _F, _P, _P]),
    "mlgnn_pathway_conv_bwd_workspace_floats": (_I64, [_I64] * 4 + [_INT]),
    "mlgnn_pathway_conv_bwd": (_INT, [_P] * 15 + [_I64] * 5 + [_INT, _F, _P, _INT, _P]),
    "mlgnn_stream_copy": (_INT, [_P, _P, _I64, _INT, _P]),
    "mlgnn_gemm_bf16_nt_workgroups": (_INT, [_I64, _I64, _INT]),
    "mlgnn_gemm_bf16_nt": (_INT, [_c.POINTER(_P), _c.POINTER(_P), _c.POINTER(_I64), _c.POINTER(_I64), _c.POINTER(_I64),
                                  _INT, _I64, _I64, _INT, _P, _P, _I64, _INT, _P, _I64, _P, _I64, _INT, _F,
                                  _P, _I64, _P, _P]),
    "mlgnn_diffpool_large_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_diffpool_large_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mlgnn_diffpool_large_saved_bytes": (_I64, [_I64, _I64, _I64]),
    "mlgnn_diffpool_large_fwd": (_INT, [_P, _P, _P, _INT, _P, _P, _P, _P, _INT, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_diffpool_large_bwd_workspace_bytes": (_I64, [_I64, _I64, _I64, _INT]),
    "mlgnn_diffpool_large_bwd": (_INT, [_P, _P, _P, _INT, _P, _P, _P, _P, _INT, _P, _P, _INT, _P, _P, _P, _P, _INT, _P, _I64,
                                        _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_diffpool_large_f32_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mlgnn_diffpool_large_f32_saved_bytes": (_I64, [_I64, _I64, _I64]),
    "mlgnn_diffpool_large_f32_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _P]),
    "mlgnn_diffpool_large_f32_bwd_workspace_bytes": (_I64, [_I64, _I64, _I64, _INT]),
    "mlgnn_diffpool_large_f32_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _INT, _P, _I64, _I64, _I64, _I64,
                                            _I64, _INT, _P]),
    "mlgnn_linear_f32x3_supported": (_INT, [_I64, _I64, _I64]),
    "mlgnn_linear_f32x3_padded_rows": (_I64, [_I64]),
    "mlgnn_linear_f32x3_fwd_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mlgnn_linear_f32x3_fwd": (_INT, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_linear_f32x3_bwd_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mlgnn_linear_f32x3_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mlgnn_adam_workspace_floats": (_I64, []),
    "mlgnn_adam_step": (_INT, [_P, _P, _P, _P, _I64, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _P, _P]),
    "mlgnn_hub_capacity": (_I64, [_I64, _INT]),
    "mlgnn_hub_scratch_bytes": (_I64, [_I64, _I64]),
    "mlgnn_hub_rows": (_INT, [_P, _I64, _INT, _I64, _P, _P, _P, _P]),
    "mlgnn_canary_malloc": (_P, [_I64, _INT, _P]),
    "mlgnn_canary_free": (None, [_P, _I64, _INT, _P]),
    "mlgnn_canary_check": (_I64, [_c.c_char_p, _I64]),
    "mlgnn_canary_stats": (_I64, [_c.POINTER(_I64)]),
}


class HubStruct(_c.Structure):
    """``mlgnn_hub_t`` (include/mlgnn.h)."""
    _fields_ = [("cap", _c.c_int32), ("capacity", _c.c_int32), ("vrows", _P), ("hubs", _P), ("counts", _P),
                ("tmp", _P), ("tmp_bytes", _I64)]


ERRORS = {-1: "MLGNN_E_NULL", -2: "MLGNN_E_SHAPE", -3: "MLGNN_E_MODE", -4: "MLGNN_E_DTYPE",
          -5: "MLGNN_E_WORKSPACE", -6: "MLGNN_E_ALIGN"}


class MlgnnError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB):
        raise ImportError(
            "libmlgnn.so is not built (%s). Build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB)
    lib = ctypes.CDLL(LIB)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError if the export is missing
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()

# MLGNN_CANARY=1 (debug; tests/README): every device allocation of the process gets guard bands (csrc/canary.hip
# becomes torch's allocator -- this must happen before the first device allocation) and every C-ABI call is followed by
# a device synchronise + a comparison of all bands; an out-of-bounds write is reported at the call that made it.
CANARY = os.environ.get("MLGNN_CANARY", "0") == "1"
CANARY_CALLS = 0


def canary_check(what):
    """Synchronise and compare every guard band; raises :class:`MlgnnError` naming ``what`` on damage."""
    buf = ctypes.create_string_buffer(512)
    rc = lib.mlgnn_canary_check(buf, 512)
    if rc != 0:
        raise MlgnnError("MLGNN_CANARY: after %s: %s" % (what, buf.value.decode(errors="replace") or "check failed (%d)" % rc))


def canary_stats():
    out = (_I64 * 4)()
    lib.mlgnn_canary_stats(out)
    return dict(live=out[0], device_allocations=out[1], reuses=out[2], checks=out[3], guarded_calls=CANARY_CALLS)


class _CanaryLib:
    """``lib`` with a guard-band check behind every call that takes a stream (the ones that launch kernels)."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if name.startswith("mlgnn_canary") or name not in SIGNATURES or not SIGNATURES[name][1] \
                or SIGNATURES[name][0] is not _INT or name.endswith("_supported") or name.endswith("_workgroups"):
            return fn

        def guarded(*args):
            global CANARY_CALLS
            rc = fn(*args)
            CANARY_CALLS += 1
            canary_check(name)
            return rc
        setattr(self, name, guarded)
        return guarded


def _install_canary():
    alloc = torch.cuda.memory.CUDAPluggableAllocator(LIB, "mlgnn_canary_malloc", "mlgnn_canary_free")
    torch.cuda.memory.change_current_allocator(alloc)       # raises if the process has allocated device memory already
    return alloc


if CANARY:
    _CANARY_ALLOCATOR = _install_canary()
    lib = _CanaryLib(lib)


def check(code, what):
    if code == 0:
        return
    if code < 0:
        raise MlgnnError("%s: argument error %s" % (what, ERRORS.get(code, code)))
    raise MlgnnError("%s: HIP error %d" % (what, code))


def ptr(t):
    """Device address of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    """Raw handle of torch's current stream."""
    return torch.cuda.current_stream().cuda_stream


def aligned(t):
    """``t`` (``None`` stays ``None``) as a kernel operand: contiguous and on a 16-byte boundary.  :func:`call` passes
    ``data_ptr()`` and nothing else, and the kernels read their operands with 16-byte loads; most entry points answer
    ``MLGNN_E_ALIGN`` for anything else.  A contiguous tensor on a boundary -- every fresh allocation, every slot of
    mlgnn.optim.FlatAdam -- is returned as it is (one ``data_ptr()`` on the host); a strided view is copied by
    ``contiguous()``, a contiguous view at an odd offset of somebody's flat buffer (``flat[1:1 + n].view(...)``) is
    cloned once."""
    if t is None:
        return None
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def call(name, *args):
    """Launch the status-returning entry point ``name``: every tensor goes in as its address (``None`` as NULL), anything
    else unchanged; a non-zero status raises :class:`MlgnnError`.  A tensor a kernel cannot read (neither on the device nor
    in pinned host memory) is refused here, before its host address reaches a kernel.  ``name`` is looked up on ``lib`` at
    call time (MLGNN_CANARY and the tests replace attributes of it)."""
    argv = list(args)
    for i, a in enumerate(argv):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda and not a.is_pinned():
                raise TypeError("%s: argument %d is a %s tensor in pageable host memory; the kernels read device (or "
                                "pinned) memory only" % (name, i, a.device))
            argv[i] = a.data_ptr()
    check(getattr(lib, name)(*argv), name)


def size(name, *dims, or_none=False):
    """The count the size query ``name`` (looked up on ``lib`` at call time, as in :func:`call`) answers for ``dims``.  A
    negative status -- a shape it does not take -- raises :class:`MlgnnError`; ``or_none`` (predicates): ``None`` instead."""
    n = int(getattr(lib, name)(*dims))
    if n < 0 and or_none:
        return None
    check(min(n, 0), name)
    return n


def workspace(name, *dims, device, times=1, unit=None):
    """``(scratch tensor, n)``, ``n = times * size(name, *dims)`` being the size the entry point is told (``times``: one
    workspace per graph of a batch).  The element type comes from the query's name -- ``*_floats`` / ``*_bytes`` -- or from
    ``unit`` where the name has no such suffix.  The tensor has ``max(n, 1)`` elements, so it is never NULL: no entry point
    refuses a non-NULL workspace of size 0 (csrc/: they compare ``workspace_floats < need`` or test ``!workspace``)."""
    dtype = {"floats": torch.float32, "bytes": torch.uint8}.get(unit or name.rsplit("_", 1)[-1])
    if dtype is None:
        raise ValueError("%s: the name says neither _floats nor _bytes; pass unit=" % name)
    n = times * size(name, *dims)
    return torch.empty(max(n, 1), dtype=dtype, device=device), n


def require_gpu(t, who):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("%s has no CPU path (the kernels are HIP only); move the tensors to the GPU" % who)


_STATS = []      # (name, counters, suffix) of every stats() dict, in import order


def stats(name, suffix="", **counters):
    """The counters dict of one op (which path its calls took; models and tests read and bump it), registered for the
    MLGNN_PRINT_STATS=1 report at exit."""
    _STATS.append((name, counters, suffix))
    return counters


if os.environ.get("MLGNN_PRINT_STATS", "0") == "1":          # development: which paths a run took
    atexit.register(lambda: print("".join("mlgnn stats: %s %r%s\n" % s for s in _STATS), end="", file=sys.stderr))
