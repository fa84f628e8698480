"""ctypes binding of libhrec.so (the C-ABI declared in include/hrec.h).

Every wrapper takes torch tensors that already live on the current HIP
device and launches on torch's current stream; nothing here computes on the
host. If the library is missing the wrappers raise HrecError — there is no
CPU fallback on the product path.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HREC_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libhrec.so")

_c_i32 = ctypes.c_int
_c_i64 = ctypes.c_int64
_c_u64 = ctypes.c_uint64
_c_dbl = ctypes.c_double
_c_sz = ctypes.c_size_t
_vp = ctypes.c_void_p

# name -> (restype, argtypes)
_SIGNATURES = {
    "hrec_abi_version": (_c_i32, []),
    "hrec_last_error": (ctypes.c_char_p, []),
    "hrec_synth_row_counts": (_c_i32, [_c_u64, _c_u64, _c_i64, _c_i64, _c_i64, _c_i32, _vp, _vp]),
    "hrec_synth_fill": (_c_i32, [_c_u64, _c_u64, _c_u64, _c_i64, _c_i64, _c_i64, _c_i32, _c_i32,
                                 _vp, _vp, _vp, _vp]),
    "hrec_scan_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_exclusive_scan_i64": (_c_i32, [_vp, _c_i64, _vp, _vp, _c_sz, _vp]),
    "hrec_encode_ids_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_encode_ids": (_c_i32, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_encode_ids_ex": (_c_i32, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_minmax_i64_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_minmax_i64": (_c_i32, [_vp, _c_i64, _vp, _vp, _c_sz, _vp]),
    "hrec_coo_to_csr_workspace_bytes": (_c_sz, [_c_i64, _c_i64]),
    "hrec_coo_to_csr": (_c_i32, [_vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_remap_i32": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _vp]),
    "hrec_rows_descending_pairs": (_c_i32, [_vp, _c_i64, _vp, _vp]),
    "hrec_coo_to_csr_sorted": (_c_i32, [_vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "hrec_als_init_factors": (_c_i32, [_c_u64, _c_i64, _c_i64, _c_i32, _c_i32, _vp, _vp]),
    "hrec_als_half_sweep_src64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _c_dbl, _vp, _vp]),
    "hrec_als_half_sweep_kernel": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i32, _c_i64, _c_i32, _c_i32, _c_dbl, _c_i32,
                                            _vp, _vp]),
    "hrec_f32_to_f64": (_c_i32, [_vp, _c_i64, _vp, _vp]),
    "hrec_als_gramian_workspace_bytes": (_c_sz, [_c_i64, _c_i32]),
    "hrec_als_gramian": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_sz, _vp]),
    "hrec_als_half_sweep_implicit": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _c_dbl, _c_dbl,
                                              _vp, _vp, _vp]),
    "hrec_als_half_sweep_nonneg": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _c_dbl, _c_i32,
                                            _c_dbl, _vp, _vp, _vp, _vp]),
    "hrec_als_half_sweep": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _c_dbl,
                                     _c_i32, _vp, _vp]),
    "hrec_transpose_f32": (_c_i32, [_vp, _c_i64, _c_i64, _vp, _c_i64, _vp]),
    "hrec_als_score": (_c_i32, [_vp, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp,
                                _vp]),
    "hrec_als_predict_pairs": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _vp, _vp]),
    "hrec_als_pair_metrics_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_als_pair_metrics": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp,
                                       _vp, _c_sz, _vp]),
    "hrec_ranking_metrics_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_ranking_metrics": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _c_sz, _vp]),
    "hrec_als_score_topk_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32]),
    "hrec_als_score_topk": (_c_i32, [_vp, _vp, _c_i32, _vp, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _vp, _vp, _vp,
                                     _vp, _c_sz, _vp]),
    "hrec_als_score_topk_excluding_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32]),
    "hrec_als_score_topk_excluding": (_c_i32, [_vp, _vp, _c_i32, _vp, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _vp,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_mask_rows_f32": (_c_i32, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, ctypes.c_float, _vp, _vp]),
    "hrec_als_items_bf16_bytes": (_c_sz, [_c_i64, _c_i32]),
    "hrec_als_items_bf16": (_c_i32, [_vp, _c_i64, _c_i64, _c_i32, _vp, _c_sz, _vp]),
    "hrec_als_score_topk_pruned_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32, _c_i32]),
    "hrec_als_score_topk_pruned": (_c_i32, [_vp, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_i32,
                                            _c_i32, _c_i32, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_als_score_topk_pruned_counts": (_c_i32, [_vp, _c_i32, _c_i64, _c_i32, _c_i32, _vp, _vp]),
    "hrec_als_score_topk_pruned_excluding_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32, _c_i32]),
    "hrec_als_score_topk_pruned_excluding": (_c_i32, [_vp, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_i32,
                                                      _c_i32, _c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_topk_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i32, _c_i32]),
    "hrec_topk_f32": (_c_i32, [_vp, _c_i64, _c_i64, _c_i64, _c_i32, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_topk_f64": (_c_i32, [_vp, _c_i64, _c_i64, _c_i64, _c_i32, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_cosine_sim": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _vp, _vp]),
    "hrec_cold_fallback_workspace_bytes": (_c_sz, [_c_i64, _c_i32]),
    "hrec_cold_fallback": (_c_i32, [_vp, _vp, _c_i64, _c_i32, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_rows_minmax_f32": (_c_i32, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp]),
    "hrec_fuse_rows_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i32]),
    "hrec_fuse_rows_topk": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i32, _c_i32, _c_i64, _vp, _vp,
                                     _vp, _c_sz, _vp]),
    "hrec_topk_f64_keyed": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i32, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_lists_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i32, _c_i32]),
    "hrec_hybrid_lists": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _c_i32, _c_i32, _c_i32, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_lists_rowwise": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i32, _c_i32, _vp, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_model_f1_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i32, _c_i32]),
    "hrec_hybrid_model_f1": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _c_i32, _c_i32, _vp, _vp, _vp, _vp,
                                      _c_i32, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_user_metrics_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_user_metrics": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _c_i64, _vp, _c_i32, _c_i32, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_rank_positions_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_rank_positions": (_c_i32, [_c_i64, _c_i64, _c_i32, _vp, _vp, _c_i64] + [_vp] * 15 + [_c_sz, _vp]),
    "hrec_row_inv_norms": (_c_i32, [_vp, _c_i64, _c_i32, _c_i64, _vp, _vp]),
    "hrec_list_quality_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_list_quality": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _c_i64, _vp, _c_i32, _c_i64, _vp, _vp, _vp, _vp,
                                   _vp, _c_i32, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_mmr_rerank": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _c_i32, _c_i64, _c_i64, _c_i64, _vp, _c_i32, _c_i64, _vp,
                                 _c_dbl, _c_i32, _vp, _vp, _vp, _vp]),
    "hrec_als_explain": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32,
                                  _c_dbl, _c_i32, _c_dbl, _vp, _c_i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hrec_cosine_items_bytes": (_c_sz, [_c_i64, _c_i32]),
    "hrec_cosine_items": (_c_i32, [_vp, _c_i64, _c_i32, _c_i64, _vp, _vp, _vp]),
    "hrec_cosine_topk_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32, _c_i32, _c_i32]),
    "hrec_cosine_topk": (_c_i32, [_vp, _c_i64, _c_i32, _c_i64, _vp, _vp, _c_i32, _c_i32, _c_i32, _c_dbl, _c_i32, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_cosine_topk_counts": (_c_i32, [_vp, _c_i32, _c_i64, _c_i32, _c_i32, _vp, _vp]),
    "hrec_fuse_workspace_bytes": (_c_sz, [_c_i64, _c_i32]),
    "hrec_fuse_topk": (_c_i32, [_vp, _vp, _c_i32, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _vp, _vp,
                                _c_sz, _vp]),
}



class TTParams(ctypes.Structure):
    """hrec_tt_params (include/hrec.h)."""
    _fields_ = [("d", ctypes.c_int32), ("reserved", ctypes.c_int32)] + [
        (name, _vp) for name in ("user_emb", "item_emb", "man_emb", "cat_emb", "w1", "b1", "w2", "b2",
                                 "ln_user_gamma", "ln_user_beta", "ln_item_gamma", "ln_item_beta")]


class SparseTable(ctypes.Structure):
    """hrec_sparse_table (include/hrec.h)."""
    _fields_ = [("var", _vp), ("m", _vp), ("v", _vp), ("n_rows", ctypes.c_int64), ("dim", ctypes.c_int32),
                ("batch", ctypes.c_int32), ("indices", _vp), ("grad_rows", _vp), ("mark", _vp), ("gsum", _vp)]


MAX_SPARSE_TABLES = 8
_PP = ctypes.POINTER(TTParams)
_SIGNATURES.update({
    "hrec_tt_item_forward": (_c_i32, [_PP, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp]),
    "hrec_tt_user_forward": (_c_i32, [_PP, _vp, _c_i64, _vp, _vp]),
    "hrec_tt_score": (_c_i32, [_vp, _c_i32, _vp, _c_i64, _c_i32, _vp, _vp]),
    "hrec_tt_pair_score": (_c_i32, [_vp, _vp, _c_i64, _c_i32, _vp, _vp]),
    "hrec_tt_predict_pairs": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp]),
    "hrec_tt_pair_metrics_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_tt_pair_metrics": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_sz,
                                      _vp]),
    "hrec_tt_fold_in_users": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i32, _vp] +
                              [ctypes.c_float] * 5 + [_vp, _vp]),
    "hrec_tt_item_inputs_workspace_bytes": (_c_sz, [_c_i64]),
    "hrec_tt_item_inputs": (_c_i32, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_tt_train_workspace_bytes": (_c_sz, [_c_i32, _c_i64]),
    "hrec_tt_grad_len": (_c_sz, [_c_i32]),
    "hrec_tt_forward_backward": (_c_i32, [_PP, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _c_sz, _vp]),
    "hrec_adam_dense": (_c_i32, [_vp, _vp, _vp, _vp, _c_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                 ctypes.c_float, _vp]),
    "hrec_f32_to_bf16": (_c_i32, [_vp, _c_i64, _vp, _vp]),
    "hrec_dot_scores": (_c_i32, [_vp, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _vp, _c_i64, _vp]),
    "hrec_dot_topk_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32]),
    "hrec_dot_topk": (_c_i32, [_vp, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _c_i32, _vp, _c_i64, _vp, _vp, _vp, _vp,
                               _c_sz, _vp]),
    "hrec_dot_topk_excluding_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32]),
    "hrec_dot_topk_excluding": (_c_i32, [_vp, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _c_i32, _vp, _c_i64, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_dot_filter": (_c_i32, [_vp, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _vp, _c_i32, _c_i64, _c_i32, _vp, _vp,
                                 _vp, _vp]),
    "hrec_hybrid_scores_workspace_bytes": (_c_sz, [_c_i32, _c_i64]),
    "hrec_hybrid_scores": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _c_i32,
                                    _vp, _vp, _c_i64, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_prune_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32, _c_i32]),
    "hrec_hybrid_prune_minmax": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp,
                                          _c_i64, _c_i32, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_prune_topk": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp,
                                        _c_i64, _c_i32, _vp, _vp, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_prune_local": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp,
                                         _c_i64, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_sz,
                                         _vp]),
    "hrec_hybrid_prune_fallback_taken": (_c_i32, [_vp, _c_i32, _c_i64, _c_i32, _c_i32, _vp, _vp]),
    "hrec_hybrid_prune_survivors": (_c_i32, [_vp, _c_i32, _c_i64, _c_i32, _c_i32, _vp, _vp]),
    "hrec_comm_get_unique_id": (_c_i32, [_vp]),
    "hrec_comm_init": (_c_i32, [_c_i32, _c_i32, _vp, ctypes.POINTER(_vp)]),
    "hrec_comm_destroy": (_c_i32, [_vp]),
    "hrec_allgather": (_c_i32, [_vp, _vp, _vp, _c_sz, _c_i32, _vp]),
    "hrec_allreduce_minmax": (_c_i32, [_vp, _vp, _c_i32, _c_i64, _vp]),
    "hrec_adam_sparse": (_c_i32, [_vp, _vp, _vp, _c_i64, _c_i32, _vp, _vp, _c_i32, _vp, _vp] +
                         [ctypes.c_float] * 6 + [_vp]),
    "hrec_adam_sparse_tables": (_c_i32, [ctypes.POINTER(SparseTable), _c_i32] + [ctypes.c_float] * 6 + [_vp]),
    "hrec_adam_sparse_tables_phase": (_c_i32, [ctypes.POINTER(SparseTable), _c_i32, _c_i32] + [ctypes.c_float] * 6
                                      + [_vp]),
})

class HybridBatch(ctypes.Structure):
    """hrec_hybrid_batch (include/hrec.h)."""
    _fields_ = [("als_users", _vp), ("als_rows", _vp), ("tt_users", _vp), ("als_items_t", _vp), ("tt_items", _vp),
                ("tt_items_t", _vp), ("prepared", _vp), ("als_ld", _c_i64), ("n_als_rows", _c_i64),
                ("tt_ld", _c_i64), ("als_items_ld", _c_i64), ("tt_items_ld", _c_i64), ("tt_items_t_ld", _c_i64),
                ("n_items", _c_i64), ("als_width", _c_i32), ("tt_width", _c_i32), ("n_users", _c_i32),
                ("dk", _c_i32)]


_HBP = ctypes.POINTER(HybridBatch)
_SIGNATURES.update({
    "hrec_hybrid_exact_items_bytes": (_c_sz, [_c_i64, _c_i32]),
    "hrec_hybrid_exact_prepare": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _c_i32, _c_i64, _c_i32, _vp, _vp]),
    "hrec_hybrid_exact_workspace_bytes": (_c_sz, [_c_i32, _c_i64, _c_i32]),
    "hrec_hybrid_exact_minmax": (_c_i32, [_HBP, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_exact_topk": (_c_i32, [_HBP, _vp, _vp, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_exact_local": (_c_i32, [_HBP, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "hrec_hybrid_exact_counts": (_c_i32, [_vp, _c_i32, _c_i64, _c_i32, _vp, _vp]),
})

ABI_VERSION = 7
_LIB = None


class HrecError(RuntimeError):
    """A libhrec call failed (or the library is not built)."""


def lib():
    """Load libhrec.so once. torch is imported first so the library binds to
    the HIP runtime torch already loaded (same soname libamdhip64.so.7)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HrecError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                " (no CPU fallback exists for the HIP hot path)")
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.hrec_abi_version() != ABI_VERSION:
            raise HrecError("libhrec ABI version mismatch; rebuild the library")
        _LIB = handle
    return _LIB


def exported_symbols():
    return list(_SIGNATURES)


def _check(name, rc):
    if rc != 0:
        msg = lib().hrec_last_error().decode(errors="replace")
        raise HrecError(f"{name} failed ({rc}): {msg}")


def _stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HrecError(f"{name}: expected a device tensor")
    if t.dtype != dtype:
        raise HrecError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise HrecError(f"{name}: tensor must be contiguous")
    return _vp(t.data_ptr())


def require_device():
    if not torch.cuda.is_available():
        raise HrecError("no HIP device visible: the MI355X hot path needs a GPU")


# ------------------------------------------------------------------ synth
def synth_row_counts(seed, threshold, row_begin, n_rows, n_cols, transposed, counts):
    _check("hrec_synth_row_counts", lib().hrec_synth_row_counts(
        seed, threshold, row_begin, n_rows, n_cols, int(transposed),
        _dev(counts, torch.int64, "counts"), _stream()))


def synth_fill(seed, seed2, threshold, row_begin, n_rows, n_cols, transposed, n_levels, indptr,
               indices, values):
    _check("hrec_synth_fill", lib().hrec_synth_fill(
        seed, seed2, threshold, row_begin, n_rows, n_cols, int(transposed), n_levels,
        _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
        _dev(values, torch.float32, "values"), _stream()))


def exclusive_scan(counts):
    """indptr[n+1] from counts[n] on the device."""
    n = counts.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=counts.device)
    ws_bytes = int(lib().hrec_scan_workspace_bytes(n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=counts.device)
    _check("hrec_exclusive_scan_i64", lib().hrec_exclusive_scan_i64(
        _dev(counts, torch.int64, "counts"), n, _dev(out, torch.int64, "out"),
        _dev(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return out


# ----------------------------------------------------------------- ingest
def minmax_i64(x):
    """(min, max) of a non-empty int64 device tensor (host ints)."""
    n = x.numel()
    out = torch.empty(2, dtype=torch.int64, device=x.device)
    ws = torch.empty(max(int(lib().hrec_minmax_i64_workspace_bytes(n)), 16), dtype=torch.uint8, device=x.device)
    _check("hrec_minmax_i64", lib().hrec_minmax_i64(
        _dev(x, torch.int64, "x"), n, _dev(out, torch.int64, "out"), _dev(ws, torch.uint8, "ws"), ws.numel(),
        _stream()))
    lo, hi = out.tolist()
    return lo, hi


def encode_ids(ids, id_range=None, order=False):
    """numpy.unique(ids, return_inverse=True) on the device: ids int64[n] ->
    (sorted distinct ids int64[m], codes int32[n]). id_range = (lo, hi) with
    lo <= ids <= hi if known; else it is measured on the device first.
    order=True appends whether ids (hence codes) are non-decreasing and, when
    they are, the row pointer of rows = codes (int64[m + 1]; else None) — both
    read by the marking / code passes (hrec_encode_ids_ex), for coo_to_csr's
    rows_in_order / indptr."""
    n = ids.numel()
    dev = ids.device
    uniq = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    codes = torch.empty(n, dtype=torch.int32, device=dev)
    n_uniq = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return (uniq[:0], codes, True, torch.zeros(1, dtype=torch.int64, device=dev)) if order else (uniq[:0], codes)
    lo, hi = minmax_i64(ids) if id_range is None else (int(id_range[0]), int(id_range[1]))
    ws = torch.empty(max(int(lib().hrec_encode_ids_workspace_bytes(n)), 16), dtype=torch.uint8, device=dev)
    desc = starts = None
    if order:
        desc = torch.zeros(1, dtype=torch.int32, device=dev)
        starts = torch.empty(min(n, hi - lo + 1) + 1, dtype=torch.int64, device=dev)
    _check("hrec_encode_ids_ex", lib().hrec_encode_ids_ex(
        _dev(ids, torch.int64, "ids"), n, lo, hi, _dev(uniq, torch.int64, "uniq"),
        _dev(n_uniq, torch.int64, "n_uniq"), _dev(codes, torch.int32, "codes"),
        _dev(desc, torch.int32, "descending") if order else None,
        _dev(starts, torch.int64, "starts") if order else None, _dev(ws, torch.uint8, "ws"),
        ws.numel(), _stream()))
    if order:
        m, d = torch.cat([n_uniq, desc.to(torch.int64)]).tolist()  # one host read
        return uniq[:m], codes, d == 0, (starts[: m + 1] if d == 0 else None)
    return uniq[: int(n_uniq.item())], codes


def coo_to_csr(rows, cols, vals, n_rows, alias=False, rows_in_order=None, indptr=None):
    """(indptr int64[n_rows+1], indices int32[nnz], values f32[nnz]) of the COO
    (rows, cols, vals), rows ascending, a row's entries in input order.
    alias=True: when rows are already in order the returned indices / values
    ARE cols / vals (no copy) — for callers that do not modify either after.
    rows_in_order: whether rows is non-decreasing, when the caller knows it
    (encode_ids(..., order=True)); None checks on the device. indptr: the
    row pointer encode_ids(..., order=True) returned for rows in order (with
    alias=True nothing runs on the device)."""
    nnz = rows.numel()
    dev = rows.device
    if cols.numel() != nnz or vals.numel() != nnz:
        raise HrecError("coo_to_csr: rows, cols and vals must have the same length")
    if indptr is not None and rows_in_order and alias:
        if indptr.numel() > n_rows + 1:
            raise HrecError("coo_to_csr: indptr has more than n_rows + 1 entries")
        if indptr.numel() < n_rows + 1:  # rows past the last code: empty (they end at nnz)
            indptr = torch.cat([indptr, torch.full((n_rows + 1 - indptr.numel(),), nnz, dtype=torch.int64,
                                                   device=dev)])
        return indptr, cols, vals
    indptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    # rows already in order (e.g. ratings grouped by user): no sort needed
    if rows_in_order is None:
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        _check("hrec_rows_descending_pairs", lib().hrec_rows_descending_pairs(
            _dev(rows, torch.int32, "rows"), nnz, _dev(flag, torch.int32, "out"), _stream()))
        in_order = int(flag.item()) == 0
    else:
        in_order = bool(rows_in_order)
    if in_order and alias:
        indices, values = cols, vals
    else:
        indices = torch.empty(nnz, dtype=torch.int32, device=dev)
        values = torch.empty(nnz, dtype=torch.float32, device=dev)
    if in_order:
        _check("hrec_coo_to_csr_sorted", lib().hrec_coo_to_csr_sorted(
            _dev(rows, torch.int32, "rows"), _dev(cols, torch.int32, "cols"), _dev(vals, torch.float32, "vals"),
            nnz, n_rows, _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
            _dev(values, torch.float32, "values"), _stream()))
        return indptr, indices, values
    ws = torch.empty(max(int(lib().hrec_coo_to_csr_workspace_bytes(nnz, n_rows)), 16), dtype=torch.uint8,
                     device=dev)
    _check("hrec_coo_to_csr", lib().hrec_coo_to_csr(
        _dev(rows, torch.int32, "rows"), _dev(cols, torch.int32, "cols"), _dev(vals, torch.float32, "vals"),
        nnz, n_rows, _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
        _dev(values, torch.float32, "values"), _dev(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return indptr, indices, values


def remap_i32(x, table):
    """x[i] = table[x[i]] in place on the device (ids outside the table -> -1)."""
    _check("hrec_remap_i32", lib().hrec_remap_i32(
        _dev(x, torch.int32, "x"), x.numel(), _dev(table, torch.int32, "table"), table.numel(), _stream()))
    return x


# -------------------------------------------------------------------- ALS
def als_init_factors(seed, row_begin, n_rows, k, kp, out):
    _check("hrec_als_init_factors", lib().hrec_als_init_factors(
        seed, row_begin, n_rows, k, kp, _dev(out, torch.float32, "out"), _stream()))


def als_half_sweep(indptr, indices, values, src_factors, k, reg_param, dst_factors, accum_mode=0, src64=None,
                   kernel=None):
    """K1. src64 (optional): the source factors already converted to f64
    (f32_to_f64 of src_factors) — same results, no conversion per gathered
    row (hrec_als_half_sweep_src64; kp 64, accum_mode 0).
    kernel (optional; kp 64, accum_mode 0): 0 = one wave per row, 1 = pooled
    (hrec_als_half_sweep_kernel); None leaves the choice to the library.
    Same bits either way."""
    n_rows = indptr.numel() - 1
    kp = dst_factors.shape[1]
    if src_factors.shape[1] != kp or dst_factors.shape[0] < n_rows:
        raise HrecError("als_half_sweep: factor shapes do not match")
    if kernel is not None:
        if accum_mode != 0 or kp != 64:
            raise HrecError("als_half_sweep: an explicit kernel needs kp 64 and accum_mode 0")
        if src64 is not None and src64.shape != src_factors.shape:
            raise HrecError("als_half_sweep: src64 needs the source factors' shape")
        src = _dev(src_factors, torch.float32, "src_factors") if src64 is None else _dev(src64, torch.float64, "src64")
        _check("hrec_als_half_sweep_kernel", lib().hrec_als_half_sweep_kernel(
            _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
            _dev(values, torch.float32, "values"), n_rows, src, 0 if src64 is None else 1, src_factors.shape[0], k,
            kp, float(reg_param), int(kernel), _dev(dst_factors, torch.float32, "dst_factors"), _stream()))
        return
    if src64 is not None:
        if accum_mode != 0 or src64.shape != src_factors.shape:
            raise HrecError("als_half_sweep: src64 needs accum_mode 0 and the source factors' shape")
        _check("hrec_als_half_sweep_src64", lib().hrec_als_half_sweep_src64(
            _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
            _dev(values, torch.float32, "values"), n_rows, _dev(src64, torch.float64, "src64"),
            src64.shape[0], k, kp, float(reg_param), _dev(dst_factors, torch.float32, "dst_factors"), _stream()))
        return
    _check("hrec_als_half_sweep", lib().hrec_als_half_sweep(
        _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
        _dev(values, torch.float32, "values"), n_rows,
        _dev(src_factors, torch.float32, "src_factors"), src_factors.shape[0], k, kp,
        float(reg_param), int(accum_mode), _dev(dst_factors, torch.float32, "dst_factors"),
        _stream()))


def als_gramian(src_factors, k):
    """YtY of the implicit-feedback half-sweep (hrec_als_gramian): f64
    [kp, kp] = sum over the rows of src_factors [n_src, kp] f32 of y y^T;
    rows and columns >= k are zero. The same bits for the same buffer."""
    n_src, kp = src_factors.shape
    dev = src_factors.device
    out = torch.empty((kp, kp), dtype=torch.float64, device=dev)
    need = int(lib().hrec_als_gramian_workspace_bytes(n_src, kp))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _check("hrec_als_gramian", lib().hrec_als_gramian(
        _dev(src_factors, torch.float32, "src_factors"), n_src, int(k), kp, _dev(out, torch.float64, "yty"),
        _dev(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return out


def als_half_sweep_implicit(indptr, indices, values, src_factors, k, reg_param, alpha, yty, dst_factors):
    """The implicit-feedback half-sweep (hrec_als_half_sweep_implicit): yty =
    als_gramian(src_factors, k); kp 16, 32 or 64."""
    n_rows = indptr.numel() - 1
    kp = dst_factors.shape[1]
    if src_factors.shape[1] != kp or dst_factors.shape[0] < n_rows or tuple(yty.shape) != (kp, kp):
        raise HrecError("als_half_sweep_implicit: factor / Gramian shapes do not match")
    _check("hrec_als_half_sweep_implicit", lib().hrec_als_half_sweep_implicit(
        _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
        _dev(values, torch.float32, "values"), n_rows, _dev(src_factors, torch.float32, "src_factors"),
        src_factors.shape[0], int(k), kp, float(reg_param), float(alpha), _dev(yty, torch.float64, "yty"),
        _dev(dst_factors, torch.float32, "dst_factors"), _stream()))


def als_half_sweep_nonneg(indptr, indices, values, src_factors, k, reg_param, dst_factors, implicit=False, alpha=0.0,
                          yty=None, iters=None):
    """The non-negative half-sweep (hrec_als_half_sweep_nonneg, Spark's
    nonnegative=True): the explicit normal equations, or with implicit=True
    the implicit ones (alpha, yty = als_gramian(src_factors, k)), solved by
    NNLS; kp 16, 32 or 64. iters (optional int32 [>= n_rows]) receives each
    row's iteration count."""
    n_rows = indptr.numel() - 1
    kp = dst_factors.shape[1]
    if src_factors.shape[1] != kp or dst_factors.shape[0] < n_rows:
        raise HrecError("als_half_sweep_nonneg: factor shapes do not match")
    if implicit and (yty is None or tuple(yty.shape) != (kp, kp)):
        raise HrecError("als_half_sweep_nonneg: implicit=True needs the [kp, kp] Gramian yty")
    if iters is not None and iters.numel() < n_rows:
        raise HrecError("als_half_sweep_nonneg: iters is shorter than the rows")
    _check("hrec_als_half_sweep_nonneg", lib().hrec_als_half_sweep_nonneg(
        _dev(indptr, torch.int64, "indptr"), _dev(indices, torch.int32, "indices"),
        _dev(values, torch.float32, "values"), n_rows, _dev(src_factors, torch.float32, "src_factors"),
        src_factors.shape[0], int(k), kp, float(reg_param), 1 if implicit else 0, float(alpha),
        _dev(yty, torch.float64, "yty") if implicit else None, _dev(dst_factors, torch.float32, "dst_factors"),
        _dev(iters, torch.int32, "iters"), _stream()))


def f32_to_f64(x, out=None):
    """Exact f32 -> f64 copy on the device (hrec_f32_to_f64)."""
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    if out.numel() != x.numel():
        raise HrecError("f32_to_f64: size mismatch")
    _check("hrec_f32_to_f64", lib().hrec_f32_to_f64(_dev(x, torch.float32, "in"), x.numel(),
                                                    _dev(out, torch.float64, "out"), _stream()))
    return out


def transpose(x, pad=4):
    """[rows, cols] -> [cols, ld] with ld = rows rounded up to `pad` (the
    padding columns are zero) so vector loads along rows stay aligned."""
    rows, cols = x.shape
    ld = -(-rows // pad) * pad
    out = torch.zeros((cols, ld), dtype=torch.float32, device=x.device)
    _check("hrec_transpose_f32", lib().hrec_transpose_f32(
        _dev(x, torch.float32, "in"), rows, cols, _dev(out, torch.float32, "out"), ld, _stream()))
    return out


def als_score(user_factors, user_rows, item_factors_t, item_rows, n_items, k, out=None):
    kp = user_factors.shape[1]
    n_users = user_rows.numel()
    if out is None:
        out = torch.empty((n_users, n_items), dtype=torch.float32, device=user_factors.device)
    _check("hrec_als_score", lib().hrec_als_score(
        _dev(user_factors, torch.float32, "user_factors"), _dev(user_rows, torch.int64, "user_rows"),
        n_users, _dev(item_factors_t, torch.float32, "item_factors_t"), item_factors_t.shape[1],
        _dev(item_rows, torch.int64, "item_rows"), n_items, k, kp,
        _dev(out, torch.float32, "out"), _stream()))
    return out


# slots of als_pair_metrics' sums (HREC_PAIR_* of include/hrec.h)
PAIR_SUMS = ("n_ok", "n_nan", "sum_e", "sum_abs_e", "sum_e2", "sum_y", "sum_y2", "sum_p", "sum_p2", "sum_yp")


def _pair_args(name, user_factors, item_factors, user_rows, item_rows):
    kp = user_factors.shape[1]
    n = user_rows.numel()
    if item_factors.shape[1] != kp or item_rows.numel() != n:
        raise HrecError(f"{name}: factor widths or row list lengths do not match")
    return kp, n, (_dev(user_factors, torch.float32, "user_factors"), user_factors.shape[0],
                   _dev(item_factors, torch.float32, "item_factors"), item_factors.shape[0])


def als_predict_pairs(user_factors, item_factors, user_rows, item_rows, k, out=None):
    """f32 [n]: the JVM-exact ALS prediction of every (user_rows[p],
    item_rows[p]) pair (hrec_als_predict_pairs); both factor matrices
    row-major [rows, kp]. NaN where either row is outside its matrix (-1)."""
    kp, n, fac = _pair_args("als_predict_pairs", user_factors, item_factors, user_rows, item_rows)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=user_factors.device)
    elif out.numel() != n:
        raise HrecError("als_predict_pairs: out must have one entry per pair")
    _check("hrec_als_predict_pairs", lib().hrec_als_predict_pairs(
        *fac, int(k), kp, _dev(user_rows, torch.int64, "user_rows"), _dev(item_rows, torch.int64, "item_rows"), n,
        _dev(out, torch.float32, "out"), _stream()))
    return out


def als_pair_metrics(user_factors, item_factors, user_rows, item_rows, k, labels, pred_out=None):
    """f64 device [len(PAIR_SUMS)]: the counts and sums of
    hrec_als_pair_metrics over the pairs' predictions against labels (f64
    [n]); pred_out (f32 [n], optional) also receives the predictions. One
    scoring launch + a fixed-order reduction: the same bits on every call."""
    kp, n, fac = _pair_args("als_pair_metrics", user_factors, item_factors, user_rows, item_rows)
    if labels.numel() != n or (pred_out is not None and pred_out.numel() != n):
        raise HrecError("als_pair_metrics: labels / pred_out must have one entry per pair")
    dev = user_factors.device
    sums = torch.empty(len(PAIR_SUMS), dtype=torch.float64, device=dev)
    need = int(lib().hrec_als_pair_metrics_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_als_pair_metrics", lib().hrec_als_pair_metrics(
        *fac, int(k), kp, _dev(user_rows, torch.int64, "user_rows"), _dev(item_rows, torch.int64, "item_rows"), n,
        _dev(labels, torch.float64, "labels"), _dev(pred_out, torch.float32, "pred_out"),
        _dev(sums, torch.float64, "sums"), _dev(ws, torch.uint8, "ws"), need, _stream()))
    return sums


# slots of ranking_metrics' sums (HREC_RANK_* of include/hrec.h)
RANK_SUMS = ("n_rows", "n_empty", "hits", "sum_precision", "sum_recall", "sum_ap", "sum_ap_k", "sum_ndcg")
RANK_MAX = 1024  # largest k and list length of hrec_ranking_metrics


def rank_tables(k):
    """The host tables hrec_ranking_metrics reads (numpy f64): gain[i] = 1 /
    ln(i + 2), i < k, and idcg[j] = gain[0] + ... + gain[j - 1], j <= k,
    added in that order (cumsum is sequential)."""
    gain = 1.0 / np.log(np.arange(int(k), dtype=np.float64) + 2.0)
    return gain, np.concatenate([np.zeros(1), np.cumsum(gain)])


def ranking_metrics(pred, label_indptr, labels, k, pred_len=None, pred_len_max=None, want_per_row=False):
    """Spark's RankingMetrics sums over ranked id lists on the device
    (hrec_ranking_metrics). pred: int64 [n_rows, ld], row r's list best first
    in its first pred_len[r] (int32 [n_rows]; None: pred_len_max, default ld)
    entries; labels[label_indptr[r] : label_indptr[r + 1]] (int64, ascending)
    its ground truth. Returns (sums f64 [len(RANK_SUMS)], unsorted int32 [1],
    per_row f64 [n_rows, 5] or None), all on the device; the sums mean nothing
    when unsorted is 1. The same bits on every call."""
    n_rows = label_indptr.numel() - 1
    k = int(k)
    if pred.dim() != 2 or pred.shape[0] != n_rows or n_rows < 0:
        raise HrecError("ranking_metrics: pred must be [n_rows, ld] with n_rows = len(label_indptr) - 1")
    if pred_len is not None and pred_len.numel() != n_rows:
        raise HrecError("ranking_metrics: pred_len must have one entry per row")
    dev = label_indptr.device
    ld = int(pred.shape[1])
    len_max = ld if pred_len_max is None else int(pred_len_max)
    if n_rows > 0 and pred.numel() == 0:  # no list entries at all: a stand-in column, never read
        pred, ld = torch.zeros((n_rows, 1), dtype=torch.int64, device=dev), 1
    if labels.numel() == 0:
        labels = torch.zeros(1, dtype=torch.int64, device=dev)
    gain_h, idcg_h = rank_tables(k) if 1 <= k <= RANK_MAX else (np.zeros(1), np.zeros(2))  # the library rejects k
    gain, idcg = torch.as_tensor(gain_h, device=dev), torch.as_tensor(idcg_h, device=dev)
    sums = torch.empty(len(RANK_SUMS), dtype=torch.float64, device=dev)
    unsorted = torch.empty(1, dtype=torch.int32, device=dev)
    per_row = torch.empty((n_rows, 5), dtype=torch.float64, device=dev) if want_per_row and n_rows > 0 else None
    need = int(lib().hrec_ranking_metrics_workspace_bytes(n_rows))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_ranking_metrics", lib().hrec_ranking_metrics(
        _dev(pred, torch.int64, "pred"), ld, len_max, _dev(pred_len, torch.int32, "pred_len"),
        _dev(label_indptr, torch.int64, "label_indptr"), _dev(labels, torch.int64, "labels"), n_rows, k,
        _dev(gain, torch.float64, "gain"), _dev(idcg, torch.float64, "idcg"), _dev(per_row, torch.float64, "per_row"),
        _dev(sums, torch.float64, "sums"), _dev(unsorted, torch.int32, "unsorted"), _dev(ws, torch.uint8, "ws"), need,
        _stream()))
    if want_per_row and per_row is None:
        per_row = torch.empty((0, 5), dtype=torch.float64, device=dev)
    return sums, unsorted, per_row


def _excl_args(name, excl_indptr, excl_cols):
    """The exclusion CSR's two pointers (an empty column list: a stand-in entry, never read)."""
    if excl_cols.numel() == 0:
        excl_cols = torch.zeros(1, dtype=torch.int32, device=excl_indptr.device)
    return _dev(excl_indptr, torch.int64, f"{name}: excl_indptr"), _dev(excl_cols, torch.int32, f"{name}: excl_cols")


def _als_topk(user_factors, user_rows, item_factors_t, n_items, k, top_k, pruned=None, excl=None,
              check_overflow=False, overflow_out=None, workspace=None, out=None):
    """The body of the four als_score_topk* wrappers: entry hrec_als_score_topk
    + "_pruned" with pruned = (item_factors, items_bf16) + "_excluding" with
    excl = (excl_indptr, excl_cols). Checks the shapes and `out`, allocates
    what the caller did not pass, calls the entry; check_overflow reads the
    flag and answers a set one from the full score matrix (the pruned entries
    resolve top_k <= 8 on the device: no read there)."""
    entry = "hrec_als_score_topk" + ("_pruned" if pruned else "") + ("_excluding" if excl else "")
    name = entry[5:]
    kp = user_factors.shape[1]
    B = user_rows.numel()
    kk = min(int(top_k), int(n_items))
    dev = user_factors.device
    if pruned and (pruned[0].stride(1) != 1 or pruned[0].shape[0] < n_items):
        raise HrecError(f"{name}: item_factors must be row-major with >= n_items rows")
    if excl and excl[0].numel() != user_factors.shape[0] + 1:
        raise HrecError(f"{name}: excl_indptr must have one entry per factor row + 1")
    if out is None:
        out = (torch.empty((B, kk), dtype=torch.int64, device=dev),
               torch.empty((B, kk), dtype=torch.float32, device=dev))
        if excl:
            out += (torch.empty(B, dtype=torch.int32, device=dev),)
    elif (tuple(out[0].shape) != (B, kk) or tuple(out[1].shape) != (B, kk) or check_overflow
          or (excl and out[2].numel() != B)):
        raise HrecError(f"{name}: out must be two [B, kk] tensors"
                        + (" and one [B]" if excl else ", with check_overflow=False"))
    # zeroed by the library on the stream
    flag = overflow_out if overflow_out is not None else torch.empty(1, dtype=torch.int32, device=dev)
    query = getattr(lib(), entry + "_workspace_bytes")
    need = int(query(B, n_items, kk, int(k)) if pruned else query(B, n_items, kk))
    ws = workspace if workspace is not None and workspace.numel() >= need else \
        torch.empty(need, dtype=torch.uint8, device=dev)
    args = [_dev(user_factors, torch.float32, "user_factors"), _dev(user_rows, torch.int64, "user_rows"), B,
            _dev(item_factors_t, torch.float32, "item_factors_t"), item_factors_t.shape[1]]
    if pruned:
        args += [_dev(pruned[0], torch.float32, "item_factors"), pruned[0].stride(0),
                 _dev(pruned[1], torch.uint8, "items_bf16")]
    args += [n_items, int(k), kp, kk]
    if excl:
        args += _excl_args(name, *excl)
    args += [_dev(out[0], torch.int64, "out_idx"), _dev(out[1], torch.float32, "out_val")]
    if excl:
        args.append(_dev(out[2], torch.int32, "out_len"))
    args += [_dev(flag, torch.int32, "overflow"), _dev(ws, torch.uint8, "ws"), ws.numel(), _stream()]
    _check(entry, getattr(lib(), entry)(*args))
    if check_overflow and (kk > 8 or not pruned) and int(flag.item()) != 0:
        scores = als_score(user_factors, user_rows, item_factors_t, None, n_items, k)
        return topk(scores, kk)
    return out


def als_score_topk(user_factors, user_rows, item_factors_t, n_items, k, top_k, check_overflow=True,
                   overflow_out=None):
    """Top-k of the JVM-exact ALS scores over items [0, n_items) for each
    (known) user, without materialising the score matrix. Falls back to the
    full score matrix + top-k when a user's survivor list overflowed.
    overflow_out (device int32 [1], optional) receives the library's overflow
    flag (with check_overflow=False the caller resolves it later)."""
    return _als_topk(user_factors, user_rows, item_factors_t, n_items, k, top_k, check_overflow=check_overflow,
                     overflow_out=overflow_out)


def als_score_topk_excluding(user_factors, user_rows, item_factors_t, n_items, k, top_k, excl_indptr, excl_cols,
                             overflow_out=None, workspace=None, out=None):
    """als_score_topk over the items outside each query's exclusion set
    (hrec_als_score_topk_excluding): (ids int64 [B, kk], scores f32 [B, kk],
    lens int32 [B]), a list's entries past its length unspecified.
    excl_indptr (int64) / excl_cols (int32, ascending per row): a CSR over the
    rows of user_factors. The overflow flag (overflow_out, device int32 [1])
    is the caller's to resolve: a set flag means als_score + mask_rows (NaN) +
    topk. workspace (uint8 device, optional) is reused when large enough; out
    (optional): the contiguous ([B, kk], [B, kk], [B]) tensors to write."""
    return _als_topk(user_factors, user_rows, item_factors_t, n_items, k, top_k, excl=(excl_indptr, excl_cols),
                     overflow_out=overflow_out, workspace=workspace, out=out)


def mask_rows(vals, row_ids, excl_indptr, excl_cols, fill=float("nan")):
    """vals[i, c] = fill (in place) for every column c of the exclusion set
    of factor row row_ids[i] (hrec_mask_rows_f32; the CSR of
    als_score_topk_excluding). vals: f32 [n_rows, n], unit column stride.
    Returns int32 [n_rows]: n - the row's distinct in-range excluded columns."""
    if vals.dtype != torch.float32 or not vals.is_cuda:
        raise HrecError("mask_rows: vals must be an f32 device tensor")
    if vals.dim() != 2 or vals.stride(1) != 1 or row_ids.numel() != vals.shape[0]:
        raise HrecError("mask_rows: vals must be [n_rows, n] with one row id per row")
    n_rows, n = vals.shape
    kept = torch.empty(n_rows, dtype=torch.int32, device=vals.device)
    _check("hrec_mask_rows_f32", lib().hrec_mask_rows_f32(
        _vp(vals.data_ptr()), n_rows, n, max(int(vals.stride(0)), n),  # a one-row view may carry any stride
        _dev(row_ids, torch.int64, "row_ids"), *_excl_args("mask_rows", excl_indptr, excl_cols),
        ctypes.c_float(fill), _dev(kept, torch.int32, "kept_out"), _stream()))
    return kept


def als_items_bf16(item_factors, k):
    """The pruned ALS top-k's item operand (hrec_als_items_bf16): bf16 rows
    [N][dk] + the largest row norm, one uint8 device buffer (once per item
    matrix; item_factors row-major f32 [N, >= k])."""
    n = int(item_factors.shape[0])
    need = int(lib().hrec_als_items_bf16_bytes(n, int(k)))
    out = torch.empty(need, dtype=torch.uint8, device=item_factors.device)
    _check("hrec_als_items_bf16", lib().hrec_als_items_bf16(
        _dev(item_factors, torch.float32, "item_factors"), item_factors.stride(0), n, int(k),
        _vp(out.data_ptr()), need, _stream()))
    return out


def als_score_topk_pruned(user_factors, user_rows, item_factors_t, item_factors, items_bf16, n_items, k, top_k,
                          check_overflow=True, overflow_out=None, workspace=None, out=None):
    """als_score_topk with the bf16 matrix-core bound in front of the exact
    chain (hrec_als_score_topk_pruned): the same (ids, scores). item_factors
    is the row-major copy of item_factors_t, items_bf16 from als_items_bf16.
    workspace (uint8 device, optional) is reused when large enough. For
    top_k <= 8 an overflow is resolved on the device inside the call (no
    host read); above, the overflow flag falls back to the full score matrix
    + top-k as als_score_topk does (check_overflow). out (optional): the
    contiguous (int64 [B, kk], f32 [B, kk]) tensors to write, e.g. the row
    slices of a larger result (with check_overflow=False)."""
    return _als_topk(user_factors, user_rows, item_factors_t, n_items, k, top_k, pruned=(item_factors, items_bf16),
                     check_overflow=check_overflow, overflow_out=overflow_out, workspace=workspace, out=out)


def als_score_topk_pruned_excluding(user_factors, user_rows, item_factors_t, item_factors, items_bf16, n_items, k,
                                    top_k, excl_indptr, excl_cols, overflow_out=None, workspace=None, out=None):
    """als_score_topk_excluding with the bf16 matrix-core bound in front of
    the exact chain (hrec_als_score_topk_pruned_excluding): the same (ids int64
    [B, kk], scores f32 [B, kk], lens int32 [B]), a list's entries past its
    length unspecified. The operands are als_score_topk_pruned's, the
    exclusion CSR als_score_topk_excluding's. The overflow flag (overflow_out,
    device int32 [1]) is the caller's to resolve at every top_k: a set flag
    means the answer is incomplete and als_score_topk_excluding answers the
    call. workspace (uint8 device, optional) is reused when large enough; out
    (optional): the contiguous ([B, kk], [B, kk], [B]) tensors to write."""
    return _als_topk(user_factors, user_rows, item_factors_t, n_items, k, top_k, pruned=(item_factors, items_bf16),
                     excl=(excl_indptr, excl_cols), overflow_out=overflow_out, workspace=workspace, out=out)


def als_topk_pruned_counts(ws, B, n_items, top_k, k):
    """Diagnostics of the last als_score_topk_pruned(_excluding) call on workspace ws:
    (pairs the bf16 bound kept per user, candidates per user), int32 [B]
    each (hrec_als_score_topk_pruned_counts)."""
    out = torch.zeros(2 * B, dtype=torch.int32, device=ws.device)
    _check("hrec_als_score_topk_pruned_counts", lib().hrec_als_score_topk_pruned_counts(
        _dev(ws, torch.uint8, "ws"), int(B), int(n_items), int(top_k), int(k), _dev(out, torch.int32, "out"),
        _stream()))
    return out[:B].clone(), out[B:].clone()


# ------------------------------------------------------------------ top-k
def topk(vals, top_k):
    """Stable descending top-k of each row of a 2-D f32/f64 device tensor."""
    if vals.dim() == 1:
        vals = vals.unsqueeze(0)
    n_rows, n = vals.shape
    kk = min(int(top_k), n)
    dev = vals.device
    is64 = vals.dtype == torch.float64
    out_i = torch.empty((n_rows, kk), dtype=torch.int64, device=dev)
    out_v = torch.empty((n_rows, kk), dtype=vals.dtype, device=dev)
    if kk == 0:
        return out_i, out_v
    ws_bytes = int(lib().hrec_topk_workspace_bytes(n_rows, n, kk, int(is64)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    fn = lib().hrec_topk_f64 if is64 else lib().hrec_topk_f32
    _check("hrec_topk", fn(_dev(vals, vals.dtype, "vals"), n_rows, n, vals.stride(0), kk,
                           _dev(out_i, torch.int64, "out_idx"), _dev(out_v, vals.dtype, "out_val"),
                           _dev(ws, torch.uint8, "ws"), ws_bytes, _stream()))
    return out_i, out_v


def topk_materialised(score, lo, hi, n_cols, kk, max_bytes, out_i, out_v, lens=None, excl=None, idx_offset=0):
    """The last resort of every ranked-list path: rows [lo, hi) of out_i /
    out_v (and lens) from materialised scores. score(s, e) gives the f32
    [e - s, n_cols] scores of rows s .. e; they go through hrec_topk_f32 in
    sub-batches whose score matrix stays under max_bytes. excl (optional):
    (row_ids, excl_indptr, excl_cols) — row r's excluded columns are NaN-ed
    first (mask_rows with row_ids[r]) and lens[r] = min(kk, columns kept).
    idx_offset is added to the indices."""
    sub = max(1, max_bytes // (4 * n_cols))
    for s in range(lo, hi, sub):
        e = min(s + sub, hi)
        scores = score(s, e)
        if excl is not None:
            lens[s:e] = mask_rows(scores, excl[0][s:e], excl[1], excl[2]).clamp_(max=kk)
        idx, val = topk(scores, kk)
        out_i[s:e] = idx + int(idx_offset) if idx_offset else idx
        out_v[s:e] = val
        del scores


# ----------------------------------------------------------------- fusion
def fuse_topk(als, tt, als_wins, top_k, want_fused=True, minmax=None):
    """als: f64 [n]; tt: f32 or f64 [n] (device). Returns (idx, score, fused).
    minmax (optional f64 [4] device tensor) receives (als min, als max, tt min, tt max)."""
    n = als.numel()
    dev = als.device
    tt_f32 = tt.dtype == torch.float32
    kk = min(int(top_k), n)
    out_i = torch.empty(max(kk, 1), dtype=torch.int64, device=dev)
    out_s = torch.empty(max(kk, 1), dtype=torch.float64, device=dev)
    fused = torch.empty(n, dtype=torch.float64, device=dev) if want_fused else None
    ws_bytes = int(lib().hrec_fuse_workspace_bytes(n, kk))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _check("hrec_fuse_topk", lib().hrec_fuse_topk(
        _dev(als, torch.float64, "als"), _dev(tt, tt.dtype, "tt"), int(tt_f32), n, int(bool(als_wins)),
        kk, _dev(out_i, torch.int64, "out_idx"), _dev(out_s, torch.float64, "out_score"),
        _dev(fused, torch.float64, "out_fused"), _dev(minmax, torch.float64, "out_minmax"),
        _dev(ws, torch.uint8, "ws"), ws_bytes, _stream()))
    return out_i[:kk], out_s[:kk], fused


# ------------------------------------------------------------ cold start
def cosine_sim(feats, query_rows):
    """[n_query, n_items] f64 cosine similarities (self = -inf), sklearn's
    normalise-then-dot: a row norm below 10 * eps counts as 1."""
    n_items, dim = feats.shape
    out = torch.empty((query_rows.numel(), n_items), dtype=torch.float64, device=feats.device)
    _check("hrec_cosine_sim", lib().hrec_cosine_sim(
        _dev(feats, torch.float64, "feats"), n_items, dim, _dev(query_rows, torch.int64, "query_rows"),
        query_rows.numel(), _dev(out, torch.float64, "out"), _stream()))
    return out


COLD_MAX_DIM = 16  # hrec_cold_fallback's feature width limit


def cold_fallback(feats, ratings, want_idx=False):
    """The cold-start fallback of every item at once (hrec_cold_fallback,
    src/als_model.py:78-86,93-104): feats [n, dim] f64 (dim <= 16), ratings
    [n] f64 (the items' 'rating'), both device. Returns (mean f64 [n]: the
    mean rating of the <= 3 most similar other items with cosine > 0.5
    (cosine_sim's values: a row norm below 10 * eps counts as 1), 0 where
    there is none; count int32 [n]; idx int32 [n, 3] of those items'
    rows, -1 padded, when want_idx)."""
    n, dim = feats.shape
    dev = feats.device
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    idx = torch.empty((n, 3), dtype=torch.int32, device=dev) if want_idx else None
    need = int(lib().hrec_cold_fallback_workspace_bytes(n, dim))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_cold_fallback", lib().hrec_cold_fallback(
        _dev(feats, torch.float64, "feats"), _dev(ratings, torch.float64, "ratings"), n, dim,
        _dev(mean, torch.float64, "out_mean"), _dev(cnt, torch.int32, "out_count"),
        _dev(idx, torch.int32, "out_idx") if idx is not None else None, _dev(ws, torch.uint8, "ws"), need,
        _stream()))
    return mean, cnt, idx


# -------------------------------------------------------------- two-tower
def tt_params(d, tensors):
    """Build the hrec_tt_params block from a dict of device f32 tensors (the
    caller keeps the tensors alive)."""
    p = TTParams()
    p.d = int(d)
    for name, _ in TTParams._fields_[2:]:
        setattr(p, name, _dev(tensors[name], torch.float32, name).value)
    return p


def tt_item_forward(params, item, man, cat, numeric, out=None):
    n = item.numel()
    if out is None:
        out = torch.empty((n, params.d), dtype=torch.float32, device=item.device)
    elif tuple(out.shape) != (n, params.d):
        raise HrecError(f"tt_item_forward: out must be [{n}, {params.d}], got {tuple(out.shape)}")
    _check("hrec_tt_item_forward", lib().hrec_tt_item_forward(
        ctypes.byref(params), _dev(item, torch.int32, "item"), _dev(man, torch.int32, "manufacturer"),
        _dev(cat, torch.int32, "category"), _dev(numeric, torch.float32, "numeric"), n,
        _dev(out, torch.float32, "item_vec"), _stream()))
    return out


def tt_user_forward(params, user):
    n = user.numel()
    out = torch.empty((n, params.d), dtype=torch.float32, device=user.device)
    _check("hrec_tt_user_forward", lib().hrec_tt_user_forward(
        ctypes.byref(params), _dev(user, torch.int32, "user"), n, _dev(out, torch.float32, "user_vec"),
        _stream()))
    return out


def tt_score(user_vec, item_vec):
    B, d = user_vec.shape
    N = item_vec.shape[0]
    out = torch.empty((B, N), dtype=torch.float32, device=user_vec.device)
    _check("hrec_tt_score", lib().hrec_tt_score(
        _dev(user_vec, torch.float32, "user_vec"), B, _dev(item_vec, torch.float32, "item_vec"), N, d,
        _dev(out, torch.float32, "out"), _stream()))
    return out


# ------------------------------------------------- matrix-core dot + top-k
DOT_DK = (32, 64, 128, 256)


def dot_dk(d):
    """Row width the dot kernels read (d zero-padded up to 32/64/128/256)."""
    for dk in DOT_DK:
        if d <= dk:
            return dk
    raise HrecError(f"dot: vector width {d} > 256 is not supported")


def to_bf16(x):
    """f32 device tensor -> bfloat16 tensor (round to nearest even, on the device)."""
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _check("hrec_f32_to_bf16", lib().hrec_f32_to_bf16(
        _dev(x, torch.float32, "in"), x.numel(), _vp(out.data_ptr()), _stream()))
    return out


def dot_operand(x, dtype=torch.float32, dk=None):
    """[n, d] f32 vectors -> the kernels' operand: rows of dot_dk(d) (or dk)
    elements, zero-padded, in f32 or bf16 (16-B aligned, contiguous)."""
    n, d = x.shape
    dk = dot_dk(d) if dk is None else int(dk)
    if dk < d:
        raise HrecError(f"dot_operand: dk {dk} < width {d}")
    if d != dk or not x.is_contiguous():
        padded = torch.zeros((n, dk), dtype=x.dtype, device=x.device)
        padded[:, :d] = x
        x = padded
    if dtype == torch.bfloat16:
        return x if x.dtype == torch.bfloat16 else to_bf16(x)
    if x.dtype != torch.float32:
        raise HrecError(f"dot_operand: expected float32, got {x.dtype}")
    return x


def _dot_args(U, V):
    if U.dtype != V.dtype or U.dtype not in (torch.float32, torch.bfloat16):
        raise HrecError("dot: operands must both be float32 or both bfloat16 (see dot_operand)")
    if U.shape[1] != V.shape[1] or U.shape[1] not in DOT_DK:
        raise HrecError(f"dot: operand widths {U.shape[1]} / {V.shape[1]} must match and be one of {DOT_DK}")
    for t, name in ((U, "user_vec"), (V, "item_vec")):
        if not t.is_cuda or not t.is_contiguous():
            raise HrecError(f"dot: {name} must be a contiguous device tensor")
    return U.shape[1], int(U.dtype == torch.bfloat16)


def dot_scores(U, V):
    """out[b, j] = <U[b], V[j]> on the matrix cores (f32 accumulation).
    U, V: operands from dot_operand (same dtype and width)."""
    dk, bf = _dot_args(U, V)
    B, N = U.shape[0], V.shape[0]
    out = torch.empty((B, N), dtype=torch.float32, device=U.device)
    _check("hrec_dot_scores", lib().hrec_dot_scores(
        _vp(U.data_ptr()), B, _vp(V.data_ptr()), N, dk, bf, _dev(out, torch.float32, "out"), N, _stream()))
    return out


DOT_USER_CHUNK = 4096


def dot_topk(U, V, top_k, idx_offset=0, max_rounds=2):
    """Stable top-k of <U[b], V[j]> over all j, never materialising the score
    matrix (hrec_dot_topk). Ties -> smaller j. Returns (idx int64 [B, kk]
    (+ idx_offset), val f32 [B, kk]), kk = min(top_k, N). When a user's
    survivor list overflows, the k-th best of the survivors (a valid, higher
    lower bound) seeds another round; after max_rounds the exact chunked path
    (scores + top-k per chunk + keyed merge) answers."""
    return _dot_topk(U, V, top_k, idx_offset, max_rounds)[:2]


def _dot_topk(U, V, top_k, idx_offset, max_rounds, excl=None):
    """dot_topk's and, with excl = (excl_rows, excl_indptr, excl_cols),
    dot_topk_excluding's loop over user chunks and refinement rounds:
    (idx, val, lens or None)."""
    name = "hrec_dot_topk" + ("_excluding" if excl else "")
    dk, bf = _dot_args(U, V)
    B, N = U.shape[0], V.shape[0]
    kk = min(int(top_k), int(N))
    dev = U.device
    if excl and excl[0].numel() != B:
        raise HrecError("dot_topk_excluding: excl_rows must have one entry per query")
    out_i = torch.empty((B, kk), dtype=torch.int64, device=dev)
    out_v = torch.empty((B, kk), dtype=torch.float32, device=dev)
    out_n = torch.zeros(B, dtype=torch.int32, device=dev) if excl else None
    if B == 0 or kk == 0:
        return out_i, out_v, out_n
    p_excl = _excl_args("dot_topk_excluding", excl[1], excl[2]) if excl else None
    entry, query = getattr(lib(), name), getattr(lib(), name + "_workspace_bytes")
    for b0 in range(0, B, DOT_USER_CHUNK):
        b1 = min(B, b0 + DOT_USER_CHUNK)
        Ub = U[b0:b1]
        nb = b1 - b0
        need = int(query(nb, N, kk))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        oi, ov = out_i[b0:b1], out_v[b0:b1]
        p_in, p_out = (), (_dev(oi, torch.int64, "out_idx"), _dev(ov, torch.float32, "out_val"))
        if excl:
            rows, on = excl[0][b0:b1], out_n[b0:b1]
            p_in = (_dev(rows, torch.int64, "excl_rows"), *p_excl)
            p_out += (_dev(on, torch.int32, "out_len"),)
        thr = None
        for _ in range(max_rounds):
            _check(name, entry(
                _vp(Ub.data_ptr()), nb, _vp(V.data_ptr()), N, dk, bf, kk,
                None if thr is None else _dev(thr, torch.float32, "thr"), int(idx_offset),
                *p_in, *p_out, _dev(flag, torch.int32, "overflow"), _dev(ws, torch.uint8, "ws"), need, _stream()))
            if int(flag.item()) == 0:
                break
            thr = ov[:, kk - 1].contiguous()
        else:
            if excl:
                del ws
                topk_materialised(lambda s, e: dot_scores(Ub[s:e], V), 0, nb, N, kk, DOT_FALLBACK_BYTES, oi, ov, on,
                                  (rows, excl[1], excl[2]), idx_offset)
            else:
                ci, cv = _dot_topk_chunked(Ub, V, kk, idx_offset)
                oi.copy_(ci)
                ov.copy_(cv)
    return out_i, out_v, out_n


DOT_FALLBACK_BYTES = 1 << 30  # dot_topk_excluding's materialised fallback keeps its score matrix under this


def dot_topk_excluding(U, V, top_k, excl_rows, excl_indptr, excl_cols, idx_offset=0, max_rounds=2):
    """dot_topk over the items outside each query's exclusion set
    (hrec_dot_topk_excluding): (idx int64 [B, kk] (+ idx_offset), val f32
    [B, kk], lens int32 [B]), kk = min(top_k, N); a list's entries past its
    length are unspecified. Query b's set is excl_cols[excl_indptr[r] :
    excl_indptr[r + 1]] with r = excl_rows[b] (int64 [B]; negative: empty);
    columns int32, local item indices, ascending per row. Users go in chunks
    of DOT_USER_CHUNK; an overflowed chunk is refined as in dot_topk (the
    k-th best of the truncated ranking seeds the next round), and after
    max_rounds the materialised chain answers it: hrec_dot_scores ->
    hrec_mask_rows_f32 (NaN) -> hrec_topk_f32, in user sub-batches whose
    score matrix stays under DOT_FALLBACK_BYTES."""
    return _dot_topk(U, V, top_k, idx_offset, max_rounds, (excl_rows, excl_indptr, excl_cols))


def dot_filter(U, V, thr, thr_per=0, cap=8192):
    """Survivors of <U[b], V[j]> >= thr[b, j // thr_per] (thr [B] or [B, G]
    f32; thr_per = 0: one bound per user) — hrec_dot_filter. Returns (val f32
    [B, cap], idx int64 [B, cap], count int32 [B]); count > cap = overflow,
    list order unspecified."""
    dk, bf = _dot_args(U, V)
    B, N = U.shape[0], V.shape[0]
    dev = U.device
    thr = thr.to(device=dev, dtype=torch.float32)
    thr = thr.reshape(B, -1).contiguous()
    cv = torch.empty((B, cap), dtype=torch.float32, device=dev)
    ci = torch.empty((B, cap), dtype=torch.int64, device=dev)
    cn = torch.zeros(B, dtype=torch.int32, device=dev)
    _check("hrec_dot_filter", lib().hrec_dot_filter(
        _vp(U.data_ptr()), B, _vp(V.data_ptr()), N, dk, bf, _dev(thr, torch.float32, "thr"), thr.shape[1],
        int(thr_per), int(cap), _vp(cv.data_ptr()), _vp(ci.data_ptr()), _vp(cn.data_ptr()), _stream()))
    return cv, ci, cn


def hybrid_scores(als_users, als_rows, tt_users, als_item, tt_item):
    """Both bf16 score matrices of a hybrid batch and their per-row min/max
    in one launch (hrec_hybrid_scores): als_users [n, ka] f32 ALS factors
    (rows als_rows [B] int64 are used), tt_users [B, kt] f32 two-tower user
    vectors, als_item / tt_item bf16 [N, dk] item operands (dot_operand).
    Returns (als [B, N] f32, tt [B, N] f32, als_mm [2, B], tt_mm [2, B]) —
    dot_scores of the bf16 user operands and rows_minmax of each. A row of
    als_rows outside [0, als_users.shape[0]) gives a NaN ALS score row (as
    als_score does for an unknown user)."""
    dk = _hyb_args(als_item, tt_item)
    B, N = int(als_rows.shape[0]), int(als_item.shape[0])
    if tt_item.shape[0] != N or tt_users.shape[0] != B:
        raise HrecError("hybrid_scores: item counts / batch sizes differ")
    for t, name in ((als_users, "als_users"), (tt_users, "tt_users")):
        if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise HrecError(f"hybrid_scores: {name} must be a row-major float32 device matrix")
        if t.shape[1] > dk:
            raise HrecError(f"hybrid_scores: {name} width {t.shape[1]} > operand width {dk}")
    rows = als_rows.to(torch.int64).contiguous()
    dev = als_item.device
    als = torch.empty((B, N), dtype=torch.float32, device=dev)
    tt = torch.empty((B, N), dtype=torch.float32, device=dev)
    a_mm = torch.empty((2, B), dtype=torch.float32, device=dev)
    t_mm = torch.empty((2, B), dtype=torch.float32, device=dev)
    need = int(lib().hrec_hybrid_scores_workspace_bytes(B, N))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_hybrid_scores", lib().hrec_hybrid_scores(
        _vp(als_users.data_ptr()), als_users.stride(0), _vp(rows.data_ptr()), als_users.shape[0], als_users.shape[1],
        _vp(tt_users.data_ptr()), tt_users.stride(0), tt_users.shape[1], B, _vp(als_item.data_ptr()),
        _vp(tt_item.data_ptr()), N, dk, _vp(als.data_ptr()), _vp(tt.data_ptr()), N, _vp(a_mm.data_ptr()),
        _vp(t_mm.data_ptr()), _vp(ws.data_ptr()), need, _stream()))
    return als, tt, a_mm, t_mm


PRUNE_MAX_K = 8


class HybridPrune:
    """The pruned bf16 hybrid top-k (hrec_hybrid_prune_*) for one batch
    shape: minmax() -> (als_mm, tt_mm) [2, B] (all-reduce them across item
    shards), then topk(als_mm, tt_mm, als_wins, top_k, idx_offset) -> (ids
    [B, kk] int64, fused f64 [B, kk]). Same user / item arguments as
    hybrid_scores; the workspace carries phase 1 into phase 2."""

    def __init__(self, als_users, als_rows, tt_users, als_item, tt_item, top_k):
        self.dk = _hyb_args(als_item, tt_item)
        self.B, self.N = int(als_rows.shape[0]), int(als_item.shape[0])
        if tt_item.shape[0] != self.N or tt_users.shape[0] != self.B:
            raise HrecError("hybrid_prune: item counts / batch sizes differ")
        for t, name in ((als_users, "als_users"), (tt_users, "tt_users")):
            if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
                raise HrecError(f"hybrid_prune: {name} must be a row-major float32 device matrix")
            if t.shape[1] > self.dk:
                raise HrecError(f"hybrid_prune: {name} width {t.shape[1]} > operand width {self.dk}")
        if not 1 <= int(top_k) <= PRUNE_MAX_K:
            raise HrecError(f"hybrid_prune: top_k must be in [1, {PRUNE_MAX_K}]")
        self.top_k = int(top_k)
        self.kk = min(self.top_k, self.N)
        self.U, self.rows, self.T = als_users, als_rows.to(torch.int64).contiguous(), tt_users
        self.Va, self.Vt = als_item, tt_item
        dev = als_item.device
        self.need = int(lib().hrec_hybrid_prune_workspace_bytes(self.B, self.N, self.dk, self.top_k))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev)

    def rebind(self, als_rows, tt_users):
        """The same batch shape with other users (the workspace is reused)."""
        if int(als_rows.shape[0]) != self.B or tuple(tt_users.shape) != tuple(self.T.shape) or \
                tt_users.dtype != torch.float32 or tt_users.stride(1) != 1 or not tt_users.is_cuda:
            raise HrecError("hybrid_prune.rebind: batch shape differs from the one the workspace was sized for")
        self.rows = als_rows if als_rows.dtype == torch.int64 and als_rows.is_contiguous() else \
            als_rows.to(torch.int64).contiguous()
        self.T = tt_users
        return self

    def _users(self):
        return (_vp(self.U.data_ptr()), self.U.stride(0), _vp(self.rows.data_ptr()), self.U.shape[0], self.U.shape[1],
                _vp(self.T.data_ptr()), self.T.stride(0), self.T.shape[1], self.B, _vp(self.Va.data_ptr()),
                _vp(self.Vt.data_ptr()), self.N, self.dk)

    def minmax(self):
        dev = self.Va.device
        a_mm = torch.empty((2, self.B), dtype=torch.float32, device=dev)
        t_mm = torch.empty((2, self.B), dtype=torch.float32, device=dev)
        _check("hrec_hybrid_prune_minmax", lib().hrec_hybrid_prune_minmax(
            *self._users(), _vp(a_mm.data_ptr()), _vp(t_mm.data_ptr()), _vp(self.ws.data_ptr()), self.need,
            _stream()))
        return a_mm, t_mm

    def topk(self, als_mm, tt_mm, als_wins, idx_offset=0):
        dev = self.Va.device
        out_i = torch.empty((self.B, self.kk), dtype=torch.int64, device=dev)
        out_v = torch.empty((self.B, self.kk), dtype=torch.float64, device=dev)
        _check("hrec_hybrid_prune_topk", lib().hrec_hybrid_prune_topk(
            *self._users(), _dev(als_mm, torch.float32, "als_mm"), _dev(tt_mm, torch.float32, "tt_mm"),
            int(bool(als_wins)), self.top_k, int(idx_offset), _vp(out_i.data_ptr()), _vp(out_v.data_ptr()),
            _vp(self.ws.data_ptr()), self.need, _stream()))
        return out_i, out_v

    def local(self, als_wins, idx_offset=0):
        """Both phases for ONE item shard (hrec_hybrid_prune_local): the same
        (ids, fused) as minmax() + topk() with one launch fewer; returns
        (ids, fused, als_mm, tt_mm)."""
        dev = self.Va.device
        a_mm = torch.empty((2, self.B), dtype=torch.float32, device=dev)
        t_mm = torch.empty((2, self.B), dtype=torch.float32, device=dev)
        out_i = torch.empty((self.B, self.kk), dtype=torch.int64, device=dev)
        out_v = torch.empty((self.B, self.kk), dtype=torch.float64, device=dev)
        _check("hrec_hybrid_prune_local", lib().hrec_hybrid_prune_local(
            *self._users(), int(bool(als_wins)), self.top_k, int(idx_offset), _vp(a_mm.data_ptr()),
            _vp(t_mm.data_ptr()), _vp(out_i.data_ptr()), _vp(out_v.data_ptr()), _vp(self.ws.data_ptr()), self.need,
            _stream()))
        return out_i, out_v, a_mm, t_mm

    def survivors(self):
        """Survivors of the last topk()'s heavy-model filter per user (int32 [B])."""
        out = torch.empty(self.B, dtype=torch.int32, device=self.Va.device)
        _check("hrec_hybrid_prune_survivors", lib().hrec_hybrid_prune_survivors(
            _vp(self.ws.data_ptr()), self.B, self.N, self.dk, self.top_k, _vp(out.data_ptr()), _stream()))
        return out

    def fallback_taken(self):
        """Whether the last topk() took the exact unfused path (device flag)."""
        out = torch.empty(1, dtype=torch.int32, device=self.Va.device)
        _check("hrec_hybrid_prune_fallback_taken", lib().hrec_hybrid_prune_fallback_taken(
            _vp(self.ws.data_ptr()), self.B, self.N, self.dk, self.top_k, _vp(out.data_ptr()), _stream()))
        return bool(int(out.item()))


EXACT_MAX_K = 8
EXACT_TT_WIDTHS = (32, 64, 128)


def exact_dk(als_width, tt_width):
    """The bf16 operand width of the exact pruned hybrid (64 or 128), or None
    when the shapes are outside it (the materialised path answers)."""
    if tt_width not in EXACT_TT_WIDTHS or not 1 <= als_width <= 128:
        return None
    return 64 if max(als_width, tt_width) <= 64 else 128


class HybridExactItems:
    """One item shard prepared for the exact pruned hybrid
    (hrec_hybrid_exact_prepare): the ALS item factors TRANSPOSED as
    hrec_als_score takes them (Vt [>= k, ld], ld >= n), the two-tower item
    vectors [n, d] (d in 32/64/128, row stride a multiple of 4) and their
    transpose, and the split-bf16 operands + norm bounds of both."""

    def __init__(self, Vt, n_items, k, tt_items):
        self.k, self.d, self.N = int(k), int(tt_items.shape[1]), int(n_items)
        self.dk = exact_dk(self.k, self.d)
        if self.dk is None:
            raise HrecError(f"hybrid_exact: widths (k={self.k}, d={self.d}) outside the exact pruned path")
        for t, name in ((Vt, "Vt"), (tt_items, "tt_items")):
            if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
                raise HrecError(f"hybrid_exact: {name} must be a row-major float32 device matrix")
        if Vt.shape[0] < self.k or Vt.stride(0) < self.N or tt_items.shape[0] != self.N:
            raise HrecError("hybrid_exact: Vt must be [>= k, >= n_items] and tt_items [n_items, d]")
        if tt_items.stride(0) % 4 or tt_items.data_ptr() % 16:
            raise HrecError("hybrid_exact: tt_items rows must be 16-B aligned (row stride a multiple of 4)")
        self.Vat, self.Vt = Vt, tt_items
        self.Vtt = transpose(tt_items.contiguous())  # [d, ld]
        self.buf = torch.empty(int(lib().hrec_hybrid_exact_items_bytes(self.N, self.dk)), dtype=torch.uint8,
                               device=tt_items.device)
        _check("hrec_hybrid_exact_prepare", lib().hrec_hybrid_exact_prepare(
            _vp(Vt.data_ptr()), Vt.stride(0), self.k, _vp(tt_items.data_ptr()), tt_items.stride(0), self.d, self.N,
            self.dk, _vp(self.buf.data_ptr()), _stream()))


class HybridExact:
    """The exact pruned hybrid top-k (hrec_hybrid_exact_*) for one batch shape:
    minmax() -> (als_mm, tt_mm) [2, B] (all-reduce them across item shards),
    then topk(als_mm, tt_mm, als_wins, idx_offset) -> (ids [B, kk] int64,
    fused f64 [B, kk]); local() does both for one shard. Bit for bit
    als_score + tt_score + rows_minmax + fuse_rows_topk (batches of >= 8
    users). als_users [n, >= k] f32 (rows als_rows [B] int64 used), tt_users
    [B, d] f32; items: a HybridExactItems."""

    def __init__(self, als_users, als_rows, tt_users, items, top_k):
        if not 1 <= int(top_k) <= EXACT_MAX_K:
            raise HrecError(f"hybrid_exact: top_k must be in [1, {EXACT_MAX_K}]")
        for t, name in ((als_users, "als_users"), (tt_users, "tt_users")):
            if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
                raise HrecError(f"hybrid_exact: {name} must be a row-major float32 device matrix")
        if als_users.shape[1] < items.k or tt_users.shape[1] != items.d:
            raise HrecError("hybrid_exact: user widths differ from the prepared items'")
        self.items = items
        self.B, self.N, self.dk = int(als_rows.shape[0]), items.N, items.dk
        if tt_users.shape[0] != self.B:
            raise HrecError("hybrid_exact: batch sizes differ")
        self.top_k = int(top_k)
        self.kk = min(self.top_k, self.N)
        self.U = als_users
        self.need = int(lib().hrec_hybrid_exact_workspace_bytes(self.B, self.N, self.dk))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=tt_users.device)
        self.rebind(als_rows, tt_users)

    def rebind(self, als_rows, tt_users):
        """The same batch shape with other users (the workspace is reused)."""
        if int(als_rows.shape[0]) != self.B or tuple(tt_users.shape) != (self.B, self.items.d) or \
                tt_users.dtype != torch.float32 or tt_users.stride(1) != 1 or not tt_users.is_cuda:
            raise HrecError("hybrid_exact.rebind: batch shape differs from the one the workspace was sized for")
        self.rows = als_rows if als_rows.dtype == torch.int64 and als_rows.is_contiguous() else \
            als_rows.to(torch.int64).contiguous()
        self.T = tt_users
        it = self.items
        self.arg = HybridBatch(_vp(self.U.data_ptr()), _vp(self.rows.data_ptr()), _vp(self.T.data_ptr()),
                               _vp(it.Vat.data_ptr()), _vp(it.Vt.data_ptr()), _vp(it.Vtt.data_ptr()),
                               _vp(it.buf.data_ptr()), self.U.stride(0), self.U.shape[0], self.T.stride(0),
                               it.Vat.stride(0), it.Vt.stride(0), it.Vtt.stride(0), self.N, it.k, it.d, self.B,
                               self.dk)
        return self

    def _mm(self):
        dev = self.ws.device
        return (torch.empty((2, self.B), dtype=torch.float32, device=dev),
                torch.empty((2, self.B), dtype=torch.float32, device=dev))

    def _out(self):
        dev = self.ws.device
        return (torch.empty((self.B, self.kk), dtype=torch.int64, device=dev),
                torch.empty((self.B, self.kk), dtype=torch.float64, device=dev))

    def minmax(self):
        a_mm, t_mm = self._mm()
        _check("hrec_hybrid_exact_minmax", lib().hrec_hybrid_exact_minmax(
            ctypes.byref(self.arg), _vp(a_mm.data_ptr()), _vp(t_mm.data_ptr()), _vp(self.ws.data_ptr()), self.need,
            _stream()))
        return a_mm, t_mm

    def topk(self, als_mm, tt_mm, als_wins, idx_offset=0):
        out_i, out_v = self._out()
        _check("hrec_hybrid_exact_topk", lib().hrec_hybrid_exact_topk(
            ctypes.byref(self.arg), _dev(als_mm, torch.float32, "als_mm"), _dev(tt_mm, torch.float32, "tt_mm"),
            int(bool(als_wins)), self.top_k, int(idx_offset), _vp(out_i.data_ptr()), _vp(out_v.data_ptr()),
            _vp(self.ws.data_ptr()), self.need, _stream()))
        return out_i, out_v

    def local(self, als_wins, idx_offset=0):
        """Both phases for ONE item shard: (ids, fused, als_mm, tt_mm)."""
        a_mm, t_mm = self._mm()
        out_i, out_v = self._out()
        _check("hrec_hybrid_exact_local", lib().hrec_hybrid_exact_local(
            ctypes.byref(self.arg), int(bool(als_wins)), self.top_k, int(idx_offset), _vp(a_mm.data_ptr()),
            _vp(t_mm.data_ptr()), _vp(out_i.data_ptr()), _vp(out_v.data_ptr()), _vp(self.ws.data_ptr()), self.need,
            _stream()))
        return out_i, out_v, a_mm, t_mm

    def counts(self):
        """(groups rescored per user for the extremes [B], for the top-k [B],
        whether some user rescored every group) of the last call."""
        out = torch.empty(2 * self.B + 1, dtype=torch.int32, device=self.ws.device)
        _check("hrec_hybrid_exact_counts", lib().hrec_hybrid_exact_counts(
            _vp(self.ws.data_ptr()), self.B, self.N, self.dk, _vp(out.data_ptr()), _stream()))
        return out[: self.B], out[self.B: 2 * self.B], bool(int(out[2 * self.B].item()))


def _hyb_args(*ops):
    dk = ops[0].shape[1]
    for t in ops:
        if t.dtype != torch.bfloat16 or t.shape[1] != dk or not t.is_cuda or not t.is_contiguous():
            raise HrecError("hybrid: operands must be contiguous bfloat16 device tensors of one width")
    if dk not in (64, 128, 256):
        raise HrecError(f"hybrid: width {dk} must be 64, 128 or 256")
    return dk


def _dot_topk_chunked(U, V, kk, idx_offset, chunk=1 << 20):
    """Exact fallback: dot_scores per item chunk, per-chunk stable top-k with
    global ids, keyed merge (ties -> smaller id)."""
    cand_i, cand_v = [], []
    for j0 in range(0, V.shape[0], chunk):
        s = dot_scores(U, V[j0:j0 + chunk])
        i, v = topk(s, kk)
        cand_i.append(i + (j0 + idx_offset))
        cand_v.append(v.double())
    ci = torch.cat(cand_i, 1).contiguous()
    cv = torch.cat(cand_v, 1).contiguous()
    i, v = topk_keyed(cv, ci, kk)
    return i, v.float()


def tt_pair_score(user_vec, item_vec):
    n, d = user_vec.shape
    out = torch.empty(n, dtype=torch.float32, device=user_vec.device)
    _check("hrec_tt_pair_score", lib().hrec_tt_pair_score(
        _dev(user_vec, torch.float32, "user_vec"), _dev(item_vec, torch.float32, "item_vec"), n, d,
        _dev(out, torch.float32, "out"), _stream()))
    return out


def _tt_pair_args(name, user_vec, user_rows, item_vec, item_rows):
    d = user_vec.shape[1]
    n = user_rows.numel()
    if item_vec.shape[1] != d or item_rows.numel() != n:
        raise HrecError(f"{name}: vector widths or row list lengths do not match")
    return d, n, (_dev(user_vec, torch.float32, "user_vec"), user_vec.shape[0],
                  _dev(item_vec, torch.float32, "item_vec"), item_vec.shape[0], d,
                  _dev(user_rows, torch.int64, "user_rows"), _dev(item_rows, torch.int64, "item_rows"), n)


def tt_predict_pairs(user_vec, user_rows, item_vec, item_rows, out=None):
    """f32 [n]: the two-tower score of every (user_vec[user_rows[p]],
    item_vec[item_rows[p]]) pair (hrec_tt_predict_pairs), with the bits
    tt_pair_score / tt_score give that pair; both matrices row-major [rows,
    d], 1 <= d <= 256. NaN where either row is outside its matrix."""
    d, n, args = _tt_pair_args("tt_predict_pairs", user_vec, user_rows, item_vec, item_rows)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=user_vec.device)
    elif out.numel() != n:
        raise HrecError("tt_predict_pairs: out must have one entry per pair")
    _check("hrec_tt_predict_pairs", lib().hrec_tt_predict_pairs(*args, _dev(out, torch.float32, "out"), _stream()))
    return out


def tt_pair_sums(user_vec, user_rows, item_vec, item_rows, labels, pred_out=None):
    """f64 device [len(PAIR_SUMS)]: the counts and sums of
    hrec_tt_pair_metrics over the pairs' scores against labels (f64 [n]);
    pred_out (f32 [n], optional) also receives the scores. One scoring launch
    + a fixed-order reduction: the same bits on every call."""
    d, n, args = _tt_pair_args("tt_pair_sums", user_vec, user_rows, item_vec, item_rows)
    if labels.numel() != n or (pred_out is not None and pred_out.numel() != n):
        raise HrecError("tt_pair_sums: labels / pred_out must have one entry per pair")
    dev = user_vec.device
    sums = torch.empty(len(PAIR_SUMS), dtype=torch.float64, device=dev)
    need = int(lib().hrec_tt_pair_metrics_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_tt_pair_metrics", lib().hrec_tt_pair_metrics(
        *args, _dev(labels, torch.float64, "labels"), _dev(pred_out, torch.float32, "pred_out"),
        _dev(sums, torch.float64, "sums"), _dev(ws, torch.uint8, "ws"), need, _stream()))
    return sums


def tt_fold_in_users(emb, ln_gamma, ln_beta, item_vec, indptr, item_rows, ratings, step_lr, beta1, omb1, beta2, omb2,
                     eps, want_loss=True):
    """hrec_tt_fold_in_users: the first indptr.numel() - 1 rows of emb (f32
    [>= n_rows, d], updated in place) fitted to their histories - CSR (indptr
    int64 [n_rows + 1], item_rows int64 rows of item_vec [n_items, d], ratings
    f32) - for step_lr.numel() steps (step_lr: f32 device, the sparse Adam step
    size of each step), everything else frozen. Returns the f32 [n_rows, 2]
    mean squared error of each row before and after (None without want_loss).
    An item row outside item_vec is skipped; a row without a usable entry
    keeps its bits and gets NaN losses. 1 <= d <= 256.
    Precondition (not checked: indptr lives on the device): indptr is
    non-decreasing from indptr[0] >= 0 to indptr[-1] <= item_rows.numel();
    anything else makes the kernel read past item_rows and ratings."""
    n_rows = indptr.numel() - 1
    d = emb.shape[1]
    if n_rows < 0 or emb.shape[0] < n_rows or item_vec.shape[1] != d or ln_gamma.numel() != d or ln_beta.numel() != d:
        raise HrecError("tt_fold_in_users: emb / item_vec / LayerNorm shapes do not match")
    if item_rows.numel() != ratings.numel():
        raise HrecError("tt_fold_in_users: item_rows and ratings must have the same length")
    dev = emb.device
    loss = torch.empty((n_rows, 2), dtype=torch.float32, device=dev) if want_loss else None
    if n_rows == 0:
        return loss
    if item_rows.numel() == 0:  # an empty tensor has no address; no entry is read
        item_rows, ratings = item_rows.new_zeros(1), ratings.new_zeros(1)
    steps = int(step_lr.numel())
    _check("hrec_tt_fold_in_users", lib().hrec_tt_fold_in_users(
        _dev(emb, torch.float32, "emb"), n_rows, d, _dev(ln_gamma, torch.float32, "ln_gamma"),
        _dev(ln_beta, torch.float32, "ln_beta"), _dev(item_vec, torch.float32, "item_vec") if item_vec.shape[0] else None,
        item_vec.shape[0], _dev(indptr, torch.int64, "indptr"), _dev(item_rows, torch.int64, "item_rows"),
        _dev(ratings, torch.float32, "ratings"), steps, _dev(step_lr, torch.float32, "step_lr") if steps else None,
        float(beta1), float(omb1), float(beta2), float(omb2), float(eps), _dev(loss, torch.float32, "loss"), _stream()))
    return loss


TT_INPUTS_IDS, TT_INPUTS_INF, TT_INPUTS_DUP = 1, 2, 4


def tt_item_inputs(item, man, cat, price, rating, tables, scale, min_, ws=None):
    """hrec_tt_item_inputs: device int64 id columns + f64 numeric columns ->
    (item, man, cat int32 [n], numeric f32 [n, 2], flags int32 [1] device).
    tables = (n_item, n_man, n_cat); scale / min_: the scaler's 2 doubles.
    flags != 0: an id outside its table (or >= 2^24), an infinite numeric
    value or a repeated item id — the outputs are then not the model's
    inputs. ws: a reusable uint8 workspace of
    hrec_tt_item_inputs_workspace_bytes(n_item) bytes."""
    n = item.numel()
    dev = item.device
    need = int(lib().hrec_tt_item_inputs_workspace_bytes(int(tables[0])))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    outs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)]
    num = torch.empty((n, 2), dtype=torch.float32, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    sc = (ctypes.c_double * 2)(float(scale[0]), float(scale[1]))
    mn = (ctypes.c_double * 2)(float(min_[0]), float(min_[1]))
    _check("hrec_tt_item_inputs", lib().hrec_tt_item_inputs(
        _dev(item, torch.int64, "item"), _dev(man, torch.int64, "man"), _dev(cat, torch.int64, "cat"),
        _dev(price, torch.float64, "price"), _dev(rating, torch.float64, "rating"), n, int(tables[0]),
        int(tables[1]), int(tables[2]), ctypes.cast(sc, _vp), ctypes.cast(mn, _vp), _vp(outs[0].data_ptr()),
        _vp(outs[1].data_ptr()), _vp(outs[2].data_ptr()), _vp(num.data_ptr()), _vp(flags.data_ptr()),
        _vp(ws.data_ptr()), ws.numel(), _stream()))
    return outs[0], outs[1], outs[2], num, flags, ws


def tt_grad_len(d):
    return int(lib().hrec_tt_grad_len(int(d)))


def tt_forward_backward(params, user, item, man, cat, numeric, y, ws=None):
    """Returns (grad_dense [grad_len], g_user, g_item, g_man, g_cat)."""
    B = user.numel()
    d = params.d
    dev = user.device
    need = int(lib().hrec_tt_train_workspace_bytes(d, B))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    gd = torch.empty(tt_grad_len(d), dtype=torch.float32, device=dev)
    gu = torch.empty((B, d), dtype=torch.float32, device=dev)
    gi = torch.empty((B, d), dtype=torch.float32, device=dev)
    gm = torch.empty((B, 8), dtype=torch.float32, device=dev)
    gc = torch.empty((B, 8), dtype=torch.float32, device=dev)
    _check("hrec_tt_forward_backward", lib().hrec_tt_forward_backward(
        ctypes.byref(params), _dev(user, torch.int32, "user"), _dev(item, torch.int32, "item"),
        _dev(man, torch.int32, "manufacturer"), _dev(cat, torch.int32, "category"),
        _dev(numeric, torch.float32, "numeric"), _dev(y, torch.float32, "y"), B,
        _dev(gd, torch.float32, "grad_dense"), _dev(gu, torch.float32, "g_user"),
        _dev(gi, torch.float32, "g_item"), _dev(gm, torch.float32, "g_man"), _dev(gc, torch.float32, "g_cat"),
        _dev(ws, torch.uint8, "workspace"), ws.numel(), _stream()))
    return gd, gu, gi, gm, gc


def adam_dense(var, m, v, grad, alpha, beta1, beta2, eps):
    _check("hrec_adam_dense", lib().hrec_adam_dense(
        _dev(var, torch.float32, "var"), _dev(m, torch.float32, "m"), _dev(v, torch.float32, "v"),
        _dev(grad, torch.float32, "grad"), var.numel(), float(alpha), float(beta1), float(beta2), float(eps),
        _stream()))


def adam_sparse(var, m, v, indices, grad_rows, mark, gsum, lr, beta1, omb1, beta2, omb2, eps):
    n_rows, dim = var.shape
    _check("hrec_adam_sparse", lib().hrec_adam_sparse(
        _dev(var, torch.float32, "var"), _dev(m, torch.float32, "m"), _dev(v, torch.float32, "v"), n_rows, dim,
        _dev(indices, torch.int32, "indices"), _dev(grad_rows, torch.float32, "grad_rows"), indices.numel(),
        _dev(mark, torch.int32, "mark"), _dev(gsum, torch.float32, "gsum"), float(lr), float(beta1),
        float(omb1), float(beta2), float(omb2), float(eps), _stream()))


def adam_sparse_tables(tables, lr, beta1, omb1, beta2, omb2, eps):
    """hrec_adam_sparse over several tables in 3 launches. tables: list of
    (var, m, v, indices, grad_rows, mark, gsum) tuples, as adam_sparse takes."""
    if len(tables) > MAX_SPARSE_TABLES:
        raise HrecError(f"adam_sparse_tables: at most {MAX_SPARSE_TABLES} tables")
    arr = (SparseTable * max(1, len(tables)))()
    for j, (var, m, v, indices, grad_rows, mark, gsum) in enumerate(tables):
        n_rows, dim = var.shape
        arr[j] = SparseTable(_dev(var, torch.float32, "var"), _dev(m, torch.float32, "m"),
                             _dev(v, torch.float32, "v"), n_rows, dim, indices.numel(),
                             _dev(indices, torch.int32, "indices"), _dev(grad_rows, torch.float32, "grad_rows"),
                             _dev(mark, torch.int32, "mark"), _dev(gsum, torch.float32, "gsum"))
    _check("hrec_adam_sparse_tables", lib().hrec_adam_sparse_tables(
        arr, len(tables), float(lr), float(beta1), float(omb1), float(beta2), float(omb2), float(eps), _stream()))


SPARSE_MARK, SPARSE_SWEEP_UNTOUCHED, SPARSE_TOUCHED, SPARSE_UNMARK = 0, 1, 2, 3


def sparse_tables_arg(tables):
    """ctypes array of hrec_sparse_table for the phased sparse Adam: tables is
    a list of (var, m, v, indices, grad_rows, mark) (no gsum: phase 2 sums
    the gradients in registers). Build once per step, pass to every phase."""
    if len(tables) > MAX_SPARSE_TABLES:
        raise HrecError(f"adam_sparse_tables_phase: at most {MAX_SPARSE_TABLES} tables")
    arr = (SparseTable * max(1, len(tables)))()
    for j, (var, m, v, indices, grad_rows, mark) in enumerate(tables):
        n_rows, dim = var.shape
        arr[j] = SparseTable(_dev(var, torch.float32, "var"), _dev(m, torch.float32, "m"),
                             _dev(v, torch.float32, "v"), n_rows, dim, indices.numel(),
                             _dev(indices, torch.int32, "indices"), _dev(grad_rows, torch.float32, "grad_rows"),
                             _dev(mark, torch.int32, "mark"), None)
    return arr, len(tables)


def adam_sparse_tables_phase(arg, phase, lr=0.0, beta1=0.0, omb1=0.0, beta2=0.0, omb2=0.0, eps=0.0):
    """One phase of hrec_adam_sparse_tables_phase on the current stream
    (arg from sparse_tables_arg)."""
    arr, n = arg
    _check("hrec_adam_sparse_tables_phase", lib().hrec_adam_sparse_tables_phase(
        arr, n, int(phase), float(lr), float(beta1), float(omb1), float(beta2), float(omb2), float(eps),
        _stream()))


# --------------------------------------------------------- batched fusion
def rows_minmax(x):
    n_rows, n = x.shape
    out = torch.empty((2, n_rows), dtype=torch.float32, device=x.device)  # [mins; maxes]
    _check("hrec_rows_minmax_f32", lib().hrec_rows_minmax_f32(
        _dev(x, torch.float32, "x"), n_rows, n, x.stride(0), _dev(out, torch.float32, "out"), _stream()))
    return out


def fuse_rows_topk(als, tt, als_mm, tt_mm, als_wins, top_k, idx_offset=0):
    n_rows, n = als.shape
    kk = min(int(top_k), n)
    dev = als.device
    out_i = torch.empty((n_rows, kk), dtype=torch.int64, device=dev)
    out_v = torch.empty((n_rows, kk), dtype=torch.float64, device=dev)
    need = int(lib().hrec_fuse_rows_workspace_bytes(n_rows, n, kk))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_fuse_rows_topk", lib().hrec_fuse_rows_topk(
        _dev(als, torch.float32, "als"), _dev(tt, torch.float32, "tt"), n_rows, n, als.stride(0),
        _dev(als_mm, torch.float32, "als_minmax"), _dev(tt_mm, torch.float32, "tt_minmax"), int(bool(als_wins)),
        kk, int(idx_offset), _dev(out_i, torch.int64, "out_idx"), _dev(out_v, torch.float64, "out_val"),
        _dev(ws, torch.uint8, "ws"), need, _stream()))
    return out_i, out_v


def topk_keyed(vals, keys, top_k):
    n_rows, n = vals.shape
    kk = min(int(top_k), n)
    dev = vals.device
    out_i = torch.empty((n_rows, kk), dtype=torch.int64, device=dev)
    out_v = torch.empty((n_rows, kk), dtype=torch.float64, device=dev)
    need = int(lib().hrec_topk_workspace_bytes(n_rows, n, kk, 1))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_topk_f64_keyed", lib().hrec_topk_f64_keyed(
        _dev(vals, torch.float64, "vals"), _dev(keys, torch.int64, "keys"), n_rows, n, kk,
        _dev(out_i, torch.int64, "out_idx"), _dev(out_v, torch.float64, "out_val"), _dev(ws, torch.uint8, "ws"),
        need, _stream()))
    return out_i, out_v


# ----------------------------------------------------- hybrid ranked lists
HYBRID_LISTS_SAMPLE = 4096  # HREC_HYBRID_LISTS_SAMPLE: columns whose kk-th best key bounds a row (mode 0)
HYBRID_LISTS_CAP = 4096     # HREC_HYBRID_LISTS_CAP: entries of a row's list (mode 0)


def _score_pair(name, als, tt, fallback):
    """The checks hybrid_lists and hybrid_model_f1 share: (als, tt, ld) of two
    f32 device matrices with unit column stride and one row stride >= n."""
    for t, what in ((als, "als"), (tt, "tt")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise HrecError(f"{name}: {what} must be a 2-D f32 device tensor")
    n_rows, n = als.shape
    if tuple(tt.shape) != (n_rows, n):
        raise HrecError(f"{name}: als and tt must have the same shape")
    if n_rows > 1:
        ld = int(als.stride(0))
        if als.stride(1) != 1 or tt.stride(1) != 1 or int(tt.stride(0)) != ld or ld < n:
            raise HrecError(f"{name}: als and tt need unit column stride and one row stride >= n")
    else:
        als, tt, ld = als.contiguous(), tt.contiguous(), n
    if fallback is not None and fallback.numel() != n:
        raise HrecError(f"{name}: fallback must hold one value per column")
    return als, tt, ld


def _hybrid_lists(name, als, tt, top_k, wins, fallback, excl, mode, want_minmax):
    """The body of hybrid_lists (wins: a bool) and hybrid_lists_rowwise (wins:
    int32 [n_rows] on the device)."""
    als, tt, ld = _score_pair(name, als, tt, fallback)
    n_rows, n = als.shape
    dev = als.device
    kk = min(int(top_k), n)
    idx = torch.empty((n_rows, kk), dtype=torch.int64, device=dev)
    val = torch.empty((n_rows, kk), dtype=torch.float64, device=dev)
    lens = torch.empty(n_rows, dtype=torch.int32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    minmax = torch.empty((n_rows, 4), dtype=torch.float64, device=dev) if want_minmax else None
    if excl is not None:
        if excl[0].numel() != n_rows:
            raise HrecError(f"{name}: excl_rows must hold one entry per row")
        excl_args = (_dev(excl[0], torch.int64, f"{name}: excl_rows"), *_excl_args(name, excl[1], excl[2]))
    else:
        excl_args = (None, None, None)
    if isinstance(wins, torch.Tensor):
        if wins.numel() != n_rows:
            raise HrecError(f"{name}: row_wins must hold one entry per row")
        wins = _dev(wins, torch.int32, f"{name}: row_wins")
    else:
        wins = int(bool(wins))
    need = int(lib().hrec_hybrid_lists_workspace_bytes(n_rows, n, int(top_k), int(mode)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check(f"hrec_{name}", getattr(lib(), f"hrec_{name}")(
        _vp(als.data_ptr()), _vp(tt.data_ptr()), n_rows, n, ld, _dev(fallback, torch.float64, "fallback"),
        wins, int(top_k), int(mode), *excl_args, _dev(idx, torch.int64, "out_idx"),
        _dev(val, torch.float64, "out_val"), _dev(lens, torch.int32, "out_len"),
        _dev(minmax, torch.float64, "out_minmax"), _dev(overflow, torch.int32, "overflow"),
        _dev(ws, torch.uint8, "ws"), need, _stream()))
    res = (idx, val, lens, overflow)
    return res + (minmax,) if want_minmax else res


def hybrid_lists(als, tt, top_k, als_wins, fallback=None, excl=None, mode=0, want_minmax=False):
    """hrec_hybrid_lists over the f32 device score matrices als / tt [n_rows,
    n] (unit column stride, one shared row stride >= n): per row the stable
    descending ranking of hrec_fuse_topk's fused scores without the row's
    excluded columns, cut to kk = min(top_k, n). fallback (f64 [n] device,
    optional) replaces NaN ALS entries per column; excl (optional) =
    (excl_rows int64 [n_rows], excl_indptr int64, excl_cols int32), the CSR
    of dot_topk_excluding. mode 0: bounded (a set overflow flag means some
    row's list was cut: repeat with mode 1); mode 1: full. Returns (idx int64
    [n_rows, kk], val f64 [n_rows, kk], lens int32 [n_rows], overflow int32
    [1][, minmax f64 [n_rows, 4]]) as device tensors; entries past a row's
    length are unspecified."""
    return _hybrid_lists("hybrid_lists", als, tt, top_k, bool(als_wins), fallback, excl, mode, want_minmax)


def hybrid_lists_rowwise(als, tt, top_k, row_wins, fallback=None, excl=None, mode=0, want_minmax=False):
    """hrec_hybrid_lists_rowwise: hybrid_lists with row r's weights chosen by
    row_wins[r] != 0 (int32 [n_rows] on the device, hybrid_model_f1's wins)."""
    if not isinstance(row_wins, torch.Tensor):
        raise HrecError("hybrid_lists_rowwise: row_wins: expected a device tensor")
    return _hybrid_lists("hybrid_lists_rowwise", als, tt, top_k, row_wins, fallback, excl, mode, want_minmax)


def hybrid_model_f1(als, tt, k, labels=None, default_wins=False, fallback=None, mode=0, want_top=False):
    """hrec_hybrid_model_f1 over hybrid_lists' score matrices: per row each
    model's own stable top-min(k, n) (ALS keys with the fallback substituted,
    in f64; two-tower keys in f32; NaN last) and compute_f1_score's F1 of it
    against the row's labels. labels (optional) = (label_rows int64 [n_rows]
    (-1: no labels), label_indptr int64, label_cols int32 (candidate columns,
    ascending and distinct per row), label_total int32 (one per CSR row: the
    size of the whole ground-truth set)). Returns (f1 f64 [n_rows, 2] (ALS,
    two-tower; NaN for a row without labels), wins int32 [n_rows] (f1_als >
    f1_tt; default_wins for a row without labels), overflow int32 [1][, top
    int64 [n_rows, 2, min(k, n)]]) as device tensors. mode 0: bounded (a set
    overflow flag: repeat with mode 1); mode 1: full."""
    name = "hybrid_model_f1"
    als, tt, ld = _score_pair(name, als, tt, fallback)
    n_rows, n = als.shape
    dev = als.device
    f1 = torch.empty((n_rows, 2), dtype=torch.float64, device=dev)
    wins = torch.empty(n_rows, dtype=torch.int32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    top = torch.empty((n_rows, 2, min(max(int(k), 0), n)), dtype=torch.int64, device=dev) if want_top else None
    if labels is not None:
        rows, indptr, cols, total = labels
        if rows.numel() != n_rows:
            raise HrecError(f"{name}: label_rows must hold one entry per row")
        if total.numel() != indptr.numel() - 1:
            raise HrecError(f"{name}: label_total must hold one entry per label row")
        if total.numel() == 0:
            total = torch.zeros(1, dtype=torch.int32, device=dev)  # a stand-in entry, never read
        label_args = (_dev(rows, torch.int64, f"{name}: label_rows"), *_excl_args(name, indptr, cols),
                      _dev(total, torch.int32, f"{name}: label_total"))
    else:
        label_args = (None, None, None, None)
    need = int(lib().hrec_hybrid_model_f1_workspace_bytes(n_rows, n, int(k), int(mode)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_hybrid_model_f1", lib().hrec_hybrid_model_f1(
        _vp(als.data_ptr()), _vp(tt.data_ptr()), n_rows, n, ld, _dev(fallback, torch.float64, "fallback"), int(k),
        int(mode), *label_args, int(bool(default_wins)), _dev(f1, torch.float64, "out_f1"),
        _dev(wins, torch.int32, "out_wins"), _dev(top, torch.int64, "out_top"), _dev(overflow, torch.int32, "overflow"),
        _dev(ws, torch.uint8, "ws"), need, _stream()))
    res = (f1, wins, overflow)
    return res + (top,) if want_top else res


# ------------------------------------------------ per-user reference metrics
UM_MAX_K = 8       # HREC_UM_MAX_K: k values of one hrec_user_metrics call
UM_LIST_MAX = 1024  # largest k, ndcg_k and list length
UM_SOURCES = {"f64": 0, "f32": 1, "als": 2, "fused": 3}  # HREC_UM_SRC_*
# bit b of user_metrics' status (HREC_UM_* of include/hrec.h)
UM_STATUS = ("ndcg_undefined", "err_undefined", "no_common", "no_relevant", "no_ratings")
UM_NDCG_UNDEFINED, UM_ERR_UNDEFINED, UM_NO_COMMON, UM_NO_RELEVANT, UM_NO_RATINGS = 1, 2, 4, 8, 16


def um_columns(k_values):
    """The columns of user_metrics' per_row, in order (the reference's result keys)."""
    return ([f"Precision@{int(k)}" for k in k_values] + [f"Recall@{int(k)}" for k in k_values]
            + ["NDCG", "MAE", "RMSE"])


def um_sums(k_values):
    """The slots of user_metrics' sums, in order: per column its sum over the rows
    where it is defined, per column the count of those rows, per status bit its rows."""
    cols = um_columns(k_values)
    return tuple([f"sum_{c}" for c in cols] + [f"n_{c}" for c in cols] + [f"n_{s}" for s in UM_STATUS])


def um_discounts(ndcg_k):
    """The host table hrec_user_metrics reads (numpy f64, ndcg_k + 1 entries): 0, then the
    running sums of sklearn's discount 1 / (ln(i + 2) / ln 2), i < ndcg_k, added in
    order (cumsum is sequential)."""
    d = 1.0 / (np.log(np.arange(int(ndcg_k), dtype=np.float64) + 2.0) / np.log(2.0))
    return np.concatenate([np.zeros(1), np.cumsum(d)])


def _rows_matrix(name, what, t, dtype, n_rows):
    """(pointer, row stride) of a 2-D device tensor with unit column stride (a
    view with a larger row stride is taken as it is)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 2:
        raise HrecError(f"{name}: {what} must be a 2-D {dtype} device tensor")
    if t.shape[0] != n_rows:
        raise HrecError(f"{name}: {what} must hold one row per list")
    if t.shape[1] == 0:
        return None, t, 0
    if t.stride(1) != 1 or (n_rows > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return _vp(t.data_ptr()), t, (int(t.stride(0)) if n_rows > 1 else int(t.shape[1]))


def user_metrics(ranked, k_values, actual, scores, source=None, ndcg_k=10, list_len=None, tt=None, fallback=None,
                 minmax=None, row_wins=None):
    """hrec_user_metrics: the reference RecommenderEvaluator's per-user
    Precision@k / Recall@k (each k of k_values, at most UM_MAX_K), NDCG@ndcg_k,
    MAE and RMSE for every row. ranked: int64 [n_rows, L <= 1024] device (a
    view with a row stride is fine), row r's candidate columns best first in
    its first list_len[r] (int32 [n_rows]; None: L) entries. actual = (rows
    int64 [n_rows] (-1: no ratings), indptr int64, cols int32 (each rated
    item's candidate column, ascending, -1 outside the frame), ratings f64
    aligned with cols, frame f64: the ratings in frame order), or None.
    scores [n_rows, n]: f64 (source "f64") or f32 ("f32": np.float32
    semantics; "als": the ALS matrix with `fallback`; "fused": with tt,
    fallback, minmax [n_rows, 4] and row_wins int32 [n_rows] of the lists
    call); source None: by dtype. Returns device (per_row f64 [n_rows,
    2 * n_k + 3] in um_columns' order, status int32 [n_rows], sums f64
    [len(um_sums(k_values))]). The same bits on every call."""
    name = "user_metrics"
    ks = [int(k) for k in k_values]
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise HrecError(f"{name}: scores must be a 2-D device tensor")
    n_rows, n = (int(x) for x in scores.shape)
    dev = scores.device
    if source is None:
        source = "f32" if scores.dtype == torch.float32 else "f64"
    if source not in UM_SOURCES:
        raise HrecError(f"{name}: source must be one of {sorted(UM_SOURCES)}")
    s_ptr, scores, ld = _rows_matrix(name, "scores", scores, torch.float64 if source == "f64" else torch.float32, n_rows)
    r_ptr, ranked, r_ld = _rows_matrix(name, "ranked", ranked, torch.int64, n_rows)
    list_n = int(ranked.shape[1])
    if r_ptr is None:  # empty lists: a stand-in column, never read
        stand_in = torch.zeros((max(n_rows, 1), 1), dtype=torch.int64, device=dev)
        r_ptr, r_ld = _vp(stand_in.data_ptr()), 1
    t_ptr = None
    if source == "fused":
        t_ptr, tt, t_ld = _rows_matrix(name, "tt", tt, torch.float32, n_rows)
        if tuple(tt.shape) != (n_rows, n) or (n_rows > 1 and t_ld != ld):
            raise HrecError(f"{name}: scores and tt need the same shape and row stride")
        if minmax is None or tuple(minmax.shape) != (n_rows, 4) or row_wins is None or row_wins.numel() != n_rows:
            raise HrecError(f"{name}: the fused source needs minmax [n_rows, 4] and row_wins [n_rows]")
    if fallback is not None and fallback.numel() != n:
        raise HrecError(f"{name}: fallback must hold one value per column")
    if list_len is not None and list_len.numel() != n_rows:
        raise HrecError(f"{name}: list_len must have one entry per row")
    if actual is not None:
        rows, indptr, cols, ratings, frame = actual
        if rows.numel() != n_rows:
            raise HrecError(f"{name}: act_rows must hold one entry per row")
        if cols.numel() != ratings.numel() or cols.numel() != frame.numel():
            raise HrecError(f"{name}: act_cols, act_ratings and act_frame must have the same length")
        if cols.numel() == 0:  # stand-in entries, never read
            cols = torch.zeros(1, dtype=torch.int32, device=dev)
            ratings = frame = torch.zeros(1, dtype=torch.float64, device=dev)
        act_args = (_dev(rows, torch.int64, "act_rows"), _dev(indptr, torch.int64, "act_indptr"),
                    _dev(cols, torch.int32, "act_cols"), _dev(ratings, torch.float64, "act_ratings"),
                    _dev(frame, torch.float64, "act_frame"))
    else:
        act_args = (None,) * 5
    n_k = len(ks)
    ncol = 2 * n_k + 3
    k_arr = (ctypes.c_int32 * max(n_k, 1))(*ks)
    cs_h = um_discounts(ndcg_k) if 1 <= int(ndcg_k) <= UM_LIST_MAX else np.zeros(2)  # the library rejects ndcg_k
    cs = torch.as_tensor(cs_h, device=dev)
    per_row = torch.empty((n_rows, ncol), dtype=torch.float64, device=dev)
    status = torch.empty(n_rows, dtype=torch.int32, device=dev)
    sums = torch.zeros(2 * ncol + len(UM_STATUS), dtype=torch.float64, device=dev)
    need = int(lib().hrec_user_metrics_workspace_bytes(n_rows))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_user_metrics", lib().hrec_user_metrics(
        r_ptr, r_ld, list_n, _dev(list_len, torch.int32, "list_len"), n_rows, n, ctypes.cast(k_arr, _vp), n_k,
        int(ndcg_k), _dev(cs, torch.float64, "disc_cs"), *act_args, UM_SOURCES[source], s_ptr, t_ptr, ld,
        _dev(fallback, torch.float64, "fallback"), _dev(minmax, torch.float64, "minmax"),
        _dev(row_wins, torch.int32, "row_wins"), _dev(per_row, torch.float64, "per_row"),
        _dev(status, torch.int32, "status"), _dev(sums, torch.float64, "sums"), _dev(ws, torch.uint8, "ws"), need,
        _stream()))
    return per_row, status, sums


# ------------------------------------------- positions in the full catalogue
RP_CHUNK = 1024  # HREC_RP_CHUNK: label entries of a row keyed and sorted at a time (one pass over the row each)
# the slots of rank_positions' sums (HREC_RP_SUMS of include/hrec.h)
RP_SUMS = ("sum_auc", "sum_reciprocal_rank", "sum_w_pr", "sum_w", "n_auc", "n_reciprocal_rank", "n_w_pr", "n_w",
           "ranked", "unranked")
RP_ROW = ("auc", "reciprocal_rank", "sum_w_pr", "sum_w")
RP_ROW_N = ("live", "ranked", "unranked")


def rank_positions(scores, labels, source=None, weight=None, excl=None, tt=None, fallback=None, minmax=None,
                   row_wins=None, want_rank=True, out_rank=None):
    """hrec_rank_positions: for every label entry its 0-based position among
    ALL live candidates of its row, in the order of every top-k list here
    (larger first, equal values by smaller column, NaN last), and per row the
    AUC, the reciprocal rank and the percentile-rank sums. Ties are resolved
    by the list order, not counted as 1/2: the AUC of the ranking that is
    served. scores [n_rows, n] and source / tt / fallback / minmax / row_wins
    as in user_metrics (a view with a row stride is fine; source None: by
    dtype). labels = (rows int64 [n_rows] (-1: no labels), indptr int64, cols
    int32 (any order, duplicates allowed, -1: not a candidate)), weight f64
    aligned with cols or None; excl (optional) = (excl_rows int64 [n_rows],
    excl_indptr int64, excl_cols int32) of hybrid_lists. Returns device
    (rank int32 aligned with cols (-1: unranked; None unless want_rank; the
    entries of CSR rows that no row of the call reads are left as they are:
    out_rank, when given, is the tensor to write into), row f64 [n_rows, 4] in
    RP_ROW's order, row_n int32 [n_rows, 3] in RP_ROW_N's, sums f64
    [len(RP_SUMS)]). The same bits on every call."""
    name = "rank_positions"
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise HrecError(f"{name}: scores must be a 2-D device tensor")
    n_rows, n = (int(x) for x in scores.shape)
    dev = scores.device
    if source is None:
        source = "f32" if scores.dtype == torch.float32 else "f64"
    if source not in UM_SOURCES:
        raise HrecError(f"{name}: source must be one of {sorted(UM_SOURCES)}")
    s_ptr, scores, ld = _rows_matrix(name, "scores", scores, torch.float64 if source == "f64" else torch.float32, n_rows)
    t_ptr = None
    if source == "fused":
        t_ptr, tt, t_ld = _rows_matrix(name, "tt", tt, torch.float32, n_rows)
        if tuple(tt.shape) != (n_rows, n) or (n_rows > 1 and t_ld != ld):
            raise HrecError(f"{name}: scores and tt need the same shape and row stride")
        if minmax is None or tuple(minmax.shape) != (n_rows, 4) or row_wins is None or row_wins.numel() != n_rows:
            raise HrecError(f"{name}: the fused source needs minmax [n_rows, 4] and row_wins [n_rows]")
    if fallback is not None and fallback.numel() != n:
        raise HrecError(f"{name}: fallback must hold one value per column")
    rows, indptr, cols = labels
    if rows.numel() != n_rows:
        raise HrecError(f"{name}: label_rows must hold one entry per row")
    if weight is not None and weight.numel() != cols.numel():
        raise HrecError(f"{name}: weight must be aligned with the label columns")
    n_lab = int(cols.numel())
    if out_rank is not None:
        if out_rank.numel() != n_lab:
            raise HrecError(f"{name}: out_rank must be aligned with the label columns")
        rank = out_rank
    else:
        rank = torch.empty(n_lab, dtype=torch.int32, device=dev) if want_rank else None
    if n_lab == 0:  # stand-in entries, never read
        cols = torch.zeros(1, dtype=torch.int32, device=dev)
        weight = None
    if excl is not None:
        if excl[0].numel() != n_rows:
            raise HrecError(f"{name}: excl_rows must hold one entry per row")
        excl_args = (_dev(excl[0], torch.int64, f"{name}: excl_rows"), *_excl_args(name, excl[1], excl[2]))
    else:
        excl_args = (None, None, None)
    row = torch.empty((n_rows, len(RP_ROW)), dtype=torch.float64, device=dev)
    row_n = torch.empty((n_rows, len(RP_ROW_N)), dtype=torch.int32, device=dev)
    sums = torch.zeros(len(RP_SUMS), dtype=torch.float64, device=dev)
    need = int(lib().hrec_rank_positions_workspace_bytes(n_rows))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_rank_positions", lib().hrec_rank_positions(
        n_rows, n, UM_SOURCES[source], s_ptr, t_ptr, ld, _dev(fallback, torch.float64, "fallback"),
        _dev(minmax, torch.float64, "minmax"), _dev(row_wins, torch.int32, "row_wins"),
        _dev(rows, torch.int64, "label_rows"), _dev(indptr, torch.int64, "label_indptr"),
        _dev(cols, torch.int32, "label_cols"), _dev(weight, torch.float64, "label_weight"), *excl_args,
        _dev(rank if n_lab else None, torch.int32, "out_rank"), _dev(row, torch.float64, "out_row"),
        _dev(row_n, torch.int32, "out_row_n"), _dev(sums, torch.float64, "sums"), _dev(ws, torch.uint8, "ws"), need,
        _stream()))
    return rank, row, row_n, sums


# ------------------------------------------------------------- list quality
LQ_MAX_TABLES = 4   # HREC_LQ_MAX_TABLES
LQ_LIST_MAX = 1024  # longest list
LQ_MAX_D = 256      # widest item vector


def lq_columns(n_tab):
    """The columns of list_quality's per_row and row_n, in order."""
    return ("intraListDiversity", "unexpectedness") + tuple(f"table{t}" for t in range(int(n_tab)))


def lq_sums(n_tab):
    """The slots of list_quality's sums, in order: per column its sum over the
    rows where it is defined, then per column the count of those rows."""
    cols = lq_columns(n_tab)
    return tuple([f"sum_{c}" for c in cols] + [f"n_{c}" for c in cols])


def _vector_rows(name, vectors, d):
    """(pointer, n, d, ld) of a 2-D f32 device matrix whose first d columns
    (None: all) are the item vectors; a view with a row stride is taken as it is."""
    if not isinstance(vectors, torch.Tensor) or not vectors.is_cuda or vectors.dtype != torch.float32 \
            or vectors.dim() != 2:
        raise HrecError(f"{name}: vectors must be a 2-D float32 device tensor")
    n = int(vectors.shape[0])
    d = int(vectors.shape[1]) if d is None else int(d)
    if d > vectors.shape[1]:
        raise HrecError(f"{name}: d exceeds the vectors' columns")
    if vectors.stride(1) != 1 or (n > 1 and vectors.stride(0) < vectors.shape[1]):
        raise HrecError(f"{name}: vectors must have unit column stride")
    return _vp(vectors.data_ptr()), n, d, (int(vectors.stride(0)) if n > 1 else int(vectors.shape[1]))


def row_inv_norms(vectors, d=None):
    """hrec_row_inv_norms: f64 device [n] = 1 / |row j| over the first d
    columns (None: all) of the f32 device matrix, 0 where the squared norm is
    0 or not finite."""
    ptr, n, d, ld = _vector_rows("row_inv_norms", vectors, d)
    out = torch.empty(n, dtype=torch.float64, device=vectors.device)
    _check("hrec_row_inv_norms", lib().hrec_row_inv_norms(ptr, n, d, ld, _dev(out, torch.float64, "out"), _stream()))
    return out


def list_quality(lists, vectors, inv_norm, list_len=None, history=None, tables=None, exposure=None, sums=None,
                 d=None):
    """hrec_list_quality: per list (row of `lists`: int64 [n_rows, L <= 1024]
    device candidate columns, the first list_len[r] (int32; None: L) entries;
    a view with a row stride is fine) the intra-list diversity, the
    unexpectedness against history = (rows int64 [n_rows] (-1: none), indptr
    int64, cols int32) or None, and the means of tables (f64 [n_tab <= 4, n]
    or None) over the list; every valid entry adds 1 to exposure (int64 [n];
    None: a zeroed one is made) and the call adds onto sums (f64
    [len(lq_sums(n_tab))]; None: zeroed). vectors f32 [n, >= d] with inv_norm
    = row_inv_norms(vectors, d). Returns device (per_row f64 [n_rows, 2 +
    n_tab] in lq_columns' order, row_n int32 of the same shape (m, g, counted
    table entries), exposure, sums). The same bits on every call."""
    name = "list_quality"
    v_ptr, n, d, ld = _vector_rows(name, vectors, d)
    dev = vectors.device
    if not isinstance(lists, torch.Tensor) or lists.dim() != 2:
        raise HrecError(f"{name}: lists must be a 2-D device tensor")
    n_rows = int(lists.shape[0])
    l_ptr, lists, l_ld = _rows_matrix(name, "lists", lists, torch.int64, n_rows)
    list_n = int(lists.shape[1])
    if inv_norm.numel() != n:
        raise HrecError(f"{name}: inv_norm must hold one value per vector")
    if list_len is not None and list_len.numel() != n_rows:
        raise HrecError(f"{name}: list_len must have one entry per row")
    n_tab = 0
    if tables is not None:
        if tables.dim() != 2 or (tables.shape[0] and tables.shape[1] != n):
            raise HrecError(f"{name}: tables must be [n_tab, n]")
        n_tab = int(tables.shape[0])
    if history is not None:
        if history[0].numel() != n_rows:
            raise HrecError(f"{name}: hist_rows must hold one entry per row")
        hist_args = (_dev(history[0], torch.int64, f"{name}: hist_rows"), *_excl_args(name, history[1], history[2]))
    else:
        hist_args = (None, None, None)
    ncol = 2 + n_tab
    if exposure is None:
        exposure = torch.zeros(n, dtype=torch.int64, device=dev)
    elif exposure.numel() != n:
        raise HrecError(f"{name}: exposure must hold one counter per vector")
    if sums is None:
        sums = torch.zeros(2 * ncol, dtype=torch.float64, device=dev)
    elif sums.numel() != 2 * ncol:
        raise HrecError(f"{name}: sums must hold {2 * ncol} slots")
    per_row = torch.empty((n_rows, ncol), dtype=torch.float64, device=dev)
    row_n = torch.empty((n_rows, ncol), dtype=torch.int32, device=dev)
    need = int(lib().hrec_list_quality_workspace_bytes(n_rows))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _check("hrec_list_quality", lib().hrec_list_quality(
        l_ptr, l_ld, list_n, _dev(list_len, torch.int32, "list_len"), n_rows, n, v_ptr, d, ld,
        _dev(inv_norm, torch.float64, "inv_norm"), *hist_args,
        _dev(tables if n_tab else None, torch.float64, "tables"), n_tab, _dev(exposure, torch.int64, "exposure"),
        _dev(per_row, torch.float64, "per_row"), _dev(row_n, torch.int32, "row_n"), _dev(sums, torch.float64, "sums"),
        _dev(ws, torch.uint8, "ws"), need, _stream()))
    return per_row, row_n, exposure, sums


# ------------------------------------------------------------ MMR re-ranking
MMR_POOL_MAX = 1024  # longest pool


def mmr_rerank(pool, scores, vectors, inv_norm, lambda_, top_n, pool_len=None, d=None, want_value=False):
    """hrec_mmr_rerank: greedy Maximal Marginal Relevance over every row of
    `pool` (int64 [n_rows, P <= 1024] device candidate columns, best first, the
    first pool_len[r] (int32; None: P) entries) with the ratings `scores` (f32
    or f64 [n_rows, P]) at the same positions; views with a row stride are
    fine. vectors f32 [n, >= d] with inv_norm = row_inv_norms(vectors, d).
    Returns device (out_pos int32 [n_rows, top_n]: the selected positions in
    the pool row in selection order, -1 past out_len; out_len int32 [n_rows];
    out_value f64 [n_rows, top_n] or None). The same bits on every call."""
    name = "mmr_rerank"
    v_ptr, n, d, ld = _vector_rows(name, vectors, d)
    dev = vectors.device
    if not isinstance(pool, torch.Tensor) or pool.dim() != 2:
        raise HrecError(f"{name}: pool must be a 2-D device tensor")
    n_rows, pool_n = int(pool.shape[0]), int(pool.shape[1])
    if not isinstance(scores, torch.Tensor) or scores.dtype not in (torch.float32, torch.float64) \
            or tuple(scores.shape) != (n_rows, pool_n):
        raise HrecError(f"{name}: scores must be a float32 or float64 device tensor of the pool's shape")
    p_ptr, pool, p_ld = _rows_matrix(name, "pool", pool, torch.int64, n_rows)
    s_ptr, scores, s_ld = _rows_matrix(name, "scores", scores, scores.dtype, n_rows)
    if inv_norm.numel() != n:
        raise HrecError(f"{name}: inv_norm must hold one value per vector")
    if pool_len is not None and pool_len.numel() != n_rows:
        raise HrecError(f"{name}: pool_len must have one entry per row")
    top_n = int(top_n)
    out_pos = torch.empty((n_rows, max(top_n, 0)), dtype=torch.int32, device=dev)
    out_len = torch.empty(n_rows, dtype=torch.int32, device=dev)
    out_value = torch.empty((n_rows, max(top_n, 0)), dtype=torch.float64, device=dev) if want_value else None
    _check("hrec_mmr_rerank", lib().hrec_mmr_rerank(
        p_ptr, p_ld, pool_n, _dev(pool_len, torch.int32, "pool_len"), s_ptr, int(scores.dtype == torch.float64), s_ld,
        n_rows, n, v_ptr, d, ld, _dev(inv_norm, torch.float64, "inv_norm"), float(lambda_), top_n,
        _dev(out_pos, torch.int32, "out_pos"), _dev(out_len, torch.int32, "out_len"),
        _dev(out_value, torch.float64, "out_value"), _stream()))
    return out_pos, out_len, out_value


# ------------------------------------------------- cosine neighbours
COSINE_TOP_MAX = 1024  # largest top_k of cosine_topk
COSINE_MODES = {"auto": 0, "exhaustive": 1, "pruned": 2}
COSINE_AUTO_CUT = 3072  # kCosAutoCut of csrc/cosine_topk.hip: auto ranks smaller matrices exhaustively
COSINE_CAP = 4096  # kCosCap: rows the pruned arm's filter may keep per query


def cosine_items(vectors, inv_norm, d=None):
    """hrec_cosine_items: the bf16 unit-row operand of cosine_topk's pruned
    arm (uint8 device buffer), prepared once per matrix and reused by every
    batch. vectors f32 [n, >= d] with inv_norm = row_inv_norms(vectors, d)."""
    name = "cosine_items"
    v_ptr, n, d, ld = _vector_rows(name, vectors, d)
    if inv_norm.numel() != n:
        raise HrecError(f"{name}: inv_norm must hold one value per vector")
    out = torch.empty(int(lib().hrec_cosine_items_bytes(n, d)), dtype=torch.uint8, device=vectors.device)
    _check("hrec_cosine_items", lib().hrec_cosine_items(v_ptr, n, d, ld, _dev(inv_norm, torch.float64, "inv_norm"),
                                                        _dev(out, torch.uint8, "out"), _stream()))
    return out


def cosine_topk_workspace_bytes(n_q, n, top_k, d, mode=0):
    return int(lib().hrec_cosine_topk_workspace_bytes(int(n_q), int(n), int(top_k), int(d), int(mode)))


def cosine_topk_counts(ws, n_q, n, top_k, d):
    """int32 device [n_q]: the rows the pruned arm's filter kept per query in
    the last mode-2 cosine_topk call on the workspace `ws` (same shape)."""
    out = torch.empty(n_q, dtype=torch.int32, device=ws.device)
    _check("hrec_cosine_topk_counts", lib().hrec_cosine_topk_counts(
        _dev(ws, torch.uint8, "ws"), int(n_q), int(n), int(top_k), int(d), _dev(out, torch.int32, "out"), _stream()))
    return out


def cosine_topk(vectors, inv_norm, query_rows, top_k, skip_self=True, min_sim=float("-inf"), mode=0, items=None,
                d=None, ws=None, want_overflow=False, redo=True):
    """hrec_cosine_topk: per query row (int64 device rows of `vectors`; a row
    outside [0, n) is an unknown query) the stable top-k of the cosines to
    every row: larger first, equal cosines -> the smaller column, the query's
    own column left out when skip_self, cut to the prefix with cosine >
    min_sim. vectors f32 [n, >= d] with inv_norm = row_inv_norms(vectors, d);
    mode 0 auto / 1 exhaustive / 2 pruned (or the names of COSINE_MODES);
    items = cosine_items(vectors, inv_norm, d) for the pruned arm. Returns
    device (out_idx int64 [n_q, top_k], -1 past out_len; out_val f64, NaN past
    out_len; out_len int32 [n_q]). A call whose pruned arm raised its overflow
    flag is redone in the exhaustive arm (want_overflow: the flag of the first
    attempt is returned as a fourth value; redo=False leaves the incomplete
    result and the workspace as the pruned arm left them, for
    cosine_topk_counts). The same bits on every call and in every mode."""
    name = "cosine_topk"
    v_ptr, n, d, ld = _vector_rows(name, vectors, d)
    dev = vectors.device
    mode = COSINE_MODES.get(mode, mode)
    if inv_norm.numel() != n:
        raise HrecError(f"{name}: inv_norm must hold one value per vector")
    if not isinstance(query_rows, torch.Tensor) or query_rows.dim() != 1:
        raise HrecError(f"{name}: query_rows must be a 1-D device tensor")
    n_q, top_k = int(query_rows.numel()), int(top_k)
    out_idx = torch.empty((n_q, max(top_k, 0)), dtype=torch.int64, device=dev)
    out_val = torch.empty((n_q, max(top_k, 0)), dtype=torch.float64, device=dev)
    out_len = torch.empty(n_q, dtype=torch.int32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    raised = False

    def run(m):
        nonlocal ws
        need = cosine_topk_workspace_bytes(n_q, n, top_k, d, m)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _check("hrec_cosine_topk", lib().hrec_cosine_topk(
            v_ptr, n, d, ld, _dev(inv_norm, torch.float64, "inv_norm"), _dev(query_rows, torch.int64, "query_rows"),
            n_q, top_k, int(bool(skip_self)), float(min_sim), int(m), _dev(items, torch.uint8, "items"),
            _dev(out_idx, torch.int64, "out_idx"), _dev(out_val, torch.float64, "out_val"),
            _dev(out_len, torch.int32, "out_len"), _dev(overflow, torch.int32, "overflow"),
            _dev(ws, torch.uint8, "ws"), ws.numel(), _stream()))

    run(mode)
    if n_q and mode != 1 and int(overflow.item()):
        raised = True
        if redo:
            run(1)
    return (out_idx, out_val, out_len, raised) if want_overflow else (out_idx, out_val, out_len)


# ------------------------------------------------- ALS explanations
EXPLAIN_MAX_TOP = 32  # largest top_m (HREC_EXPLAIN_MAX_TOP)
EXPLAIN_LIST_MAX = 1024  # longest list of one kernel row


def als_explain(lists, history, item_factors, k, reg_param, top_m, implicit=False, alpha=0.0, yty=None,
                list_len=None, want_row=True):
    """hrec_als_explain: per row of `lists` (int64 [n_rows, L <= 1024] device
    item-factor rows, the first list_len[r] (int32; None: L) entries; a view
    with a row stride is fine) and per entry i, the prediction y_i . A^-1 b
    split into one term per entry of the row's history = (rows int64 [n_rows]
    (-1: none), indptr int64, cols int32 item-factor rows, vals f32 ratings).
    item_factors f32 [n_items, kp]; implicit needs yty = als_gramian of them.
    Returns device (total f64 [n_rows, L], pos int32 [n_rows, L, top_m]:
    positions within the row's history segment, -1 past len; val f64 of the
    same shape, NaN past len; len int32 [n_rows, L]; row f32 [n_rows, kp]: the
    row's own solve, or None). The same bits on every call."""
    name = "als_explain"
    if not isinstance(lists, torch.Tensor) or lists.dim() != 2:
        raise HrecError(f"{name}: lists must be a 2-D device tensor")
    if not isinstance(item_factors, torch.Tensor) or item_factors.dim() != 2:
        raise HrecError(f"{name}: item_factors must be a 2-D device tensor")
    n_rows, list_n = int(lists.shape[0]), int(lists.shape[1])
    n_items, kp = int(item_factors.shape[0]), int(item_factors.shape[1])
    dev = item_factors.device
    l_ptr, lists, l_ld = _rows_matrix(name, "lists", lists, torch.int64, n_rows)
    if list_len is not None and list_len.numel() != n_rows:
        raise HrecError(f"{name}: list_len must have one entry per row")
    h_rows, h_indptr, h_cols, h_vals = history
    if h_rows.numel() != n_rows:
        raise HrecError(f"{name}: hist_rows must hold one entry per row")
    if h_cols.numel() != h_vals.numel():
        raise HrecError(f"{name}: hist_cols and hist_vals must have one entry per rating")
    if h_cols.numel() == 0:  # stand-in entries, never read
        h_cols = torch.zeros(1, dtype=torch.int32, device=dev)
        h_vals = torch.zeros(1, dtype=torch.float32, device=dev)
    if implicit and (yty is None or tuple(yty.shape) != (kp, kp)):
        raise HrecError(f"{name}: implicit needs yty [kp, kp]")
    top_m = int(top_m)
    tm = max(top_m, 0)
    total = torch.empty((n_rows, list_n), dtype=torch.float64, device=dev)
    pos = torch.empty((n_rows, list_n, tm), dtype=torch.int32, device=dev)
    val = torch.empty((n_rows, list_n, tm), dtype=torch.float64, device=dev)
    length = torch.empty((n_rows, list_n), dtype=torch.int32, device=dev)
    row = torch.empty((n_rows, kp), dtype=torch.float32, device=dev) if want_row else None
    _check("hrec_als_explain", lib().hrec_als_explain(
        l_ptr, l_ld, list_n, _dev(list_len, torch.int32, "list_len"), n_rows,
        _dev(h_rows, torch.int64, "hist_rows"), _dev(h_indptr, torch.int64, "hist_indptr"),
        _dev(h_cols, torch.int32, "hist_cols"), _dev(h_vals, torch.float32, "hist_vals"),
        _dev(item_factors, torch.float32, "item_factors"), n_items, int(k), kp, float(reg_param), int(bool(implicit)),
        float(alpha), _dev(yty if implicit else None, torch.float64, "yty"), top_m,
        _dev(total, torch.float64, "out_total"), _dev(pos, torch.int32, "out_pos"), _dev(val, torch.float64, "out_val"),
        _dev(length, torch.int32, "out_len"), _dev(row, torch.float32, "out_row"), _stream()))
    return total, pos, val, length, row


# ------------------------------------------------------- multi-GPU (C-ABI)
_COMM_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3, torch.uint8: 4}


class Comm:
    """The C-ABI's RCCL communicator (hrec_comm_*), for hosts that drive the
    exchange steps through libhrec instead of torch.distributed: rank 0's
    unique_id() goes to every rank by the host's own channel, then every
    rank constructs Comm(rank, world, uid)."""

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * 128)()
        _check("hrec_comm_get_unique_id", lib().hrec_comm_get_unique_id(ctypes.cast(buf, _vp)))
        return bytes(buf)

    def __init__(self, rank, world, uid):
        if len(uid) != 128:
            raise HrecError("Comm: the unique id has 128 bytes")
        self._id = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        self.h = _vp()
        self.rank, self.world = int(rank), int(world)
        _check("hrec_comm_init", lib().hrec_comm_init(self.rank, self.world, ctypes.cast(self._id, _vp),
                                                      ctypes.byref(self.h)))

    def allgather(self, send, recv=None):
        """recv [world * n] = every rank's send [n] (rank-major)."""
        if send.dtype not in _COMM_DTYPES or not send.is_cuda or not send.is_contiguous():
            raise HrecError("Comm.allgather: a contiguous device tensor of f32/f64/i32/i64/u8")
        if recv is None:
            recv = torch.empty((self.world,) + tuple(send.shape), dtype=send.dtype, device=send.device)
        elif recv.numel() != self.world * send.numel() or recv.device != send.device:
            # hrec_allgather writes world x count elements: a smaller buffer is an out-of-bounds write
            raise HrecError(f"Comm.allgather: recv holds {recv.numel()} elements on {recv.device}, "
                            f"need {self.world} x {send.numel()} on {send.device}")
        _check("hrec_allgather", lib().hrec_allgather(self.h, _vp(send.data_ptr()), _dev(recv, send.dtype, "recv"),
                                                      send.numel(), _COMM_DTYPES[send.dtype], _stream()))
        return recv

    def allreduce_minmax(self, mm):
        """mm [n_rows, 2, B] f32 (each model's [min; max]) -> global extremes, in place."""
        if mm.dim() != 3 or mm.shape[1] != 2:
            raise HrecError("Comm.allreduce_minmax: mm must be [n_rows, 2, B]")
        if not mm.is_cuda or mm.dtype != torch.float32:
            raise HrecError("Comm.allreduce_minmax: mm must be a float32 device tensor")
        _check("hrec_allreduce_minmax", lib().hrec_allreduce_minmax(
            self.h, _dev(mm, torch.float32, "mm"), mm.shape[0], mm.shape[2], _stream()))
        return mm

    def close(self):
        if self.h:
            _check("hrec_comm_destroy", lib().hrec_comm_destroy(self.h))
            self.h = _vp()
