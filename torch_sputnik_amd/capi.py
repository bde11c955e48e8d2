"""ctypes view of the C ABI (include/sputnik_hip.h) for callers that hold raw
device memory: the parity tests and bench.py call the kernels through this, on
torch-allocated HIP buffers, without going through the TORCH_LIBRARY layer.

Every wrapper takes already-valid int32 / float32 contiguous GPU tensors,
passes their pointers plus the current HIP stream, and raises on a nonzero
status.  No shape inference or casting happens here (that is the op layer's
job, csrc/torch_binding.cpp).
"""
import ctypes

import torch

from ._native import kernel_lib

_c_int = ctypes.c_int
_c_i64 = ctypes.c_int64
_c_ptr = ctypes.c_void_p
_c_size = ctypes.c_size_t
_c_float = ctypes.c_float


class PhiloxState(ctypes.Structure):
    """sputnik_hip_philox_state: seed and offset values, or device pointers to them (NULL:
    the values are meant) plus the in-graph offset -- a PhiloxCudaState without torch."""
    _fields_ = [("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("seed_ptr", ctypes.c_void_p), ("offset_ptr", ctypes.c_void_p),
                ("offset_intragraph", ctypes.c_uint64)]


class AttentionPatternArgs(ctypes.Structure):
    """sputnik_hip_attention_pattern_args: the rule of an attention pattern as the kernels take
    it (include/sputnik_hip.h, "Attention patterns"; ops.attention_pattern_csr fills one in)."""
    _fields_ = [("offset", ctypes.c_int64), ("window_left", ctypes.c_int64), ("window_right", ctypes.c_int64),
                ("dilation", ctypes.c_int64), ("block", ctypes.c_int), ("summary_stride", ctypes.c_int),
                ("summary_first", ctypes.c_int), ("random_block", ctypes.c_int),
                ("random_threshold", ctypes.c_uint), ("causal", ctypes.c_int), ("global_rows", ctypes.c_int),
                ("global_flags", ctypes.c_void_p)]


_DROP = [ctypes.c_double, PhiloxState, _c_ptr]   # p, state, rng_state_out

# name -> (restype, argtypes); must list every symbol include/sputnik_hip.h declares.
SIGNATURES = {
    "sputnik_hip_version": (ctypes.c_char_p, []),
    "sputnik_hip_build_id": (ctypes.c_char_p, []),
    "sputnik_hip_spmm_kernel_name": (ctypes.c_char_p, [_c_int] * 5),
    "sputnik_hip_spmm_typed_kernel_name": (ctypes.c_char_p, [_c_int] * 6 + [_c_i64, _c_int]),
    "sputnik_hip_left_spmm_half_tiles_tile_rows": (_c_int, [_c_int] * 3),
    "sputnik_hip_sddmm_kernel_name": (ctypes.c_char_p, [_c_int] * 7),
    "sputnik_hip_sddmm_sum_route": (_c_int, [_c_int] * 8 + [_c_ptr] * 5),
    "sputnik_hip_sddmm_launch_shape": (_c_int, [_c_int] * 10 + [_c_ptr] * 9),
    "sputnik_hip_spmm_launch_shape": (_c_int, [_c_int] * 6 + [_c_ptr]),
    "sputnik_hip_sparse_softmax_route": (_c_int, [_c_int] * 5 + [_c_ptr] * 6),
    "sputnik_hip_reload_options": (None, []),
    "sputnik_hip_spmm": (_c_int, [_c_int] * 4 + [_c_ptr] * 7),
    "sputnik_hip_spmm_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_spmm_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_i64, _c_ptr, _c_ptr,
                                                        _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr,
                                                        _c_size, _c_ptr]),
    "sputnik_hip_spmm_plan": (_c_int, [_c_int] * 4 + [_c_ptr] * 4 + [_c_size, _c_ptr]),
    "sputnik_hip_spmm_batched_planned": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_i64, _c_ptr,
                                                                _c_ptr, _c_ptr, _c_i64, _c_ptr,
                                                                _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sddmm": (_c_int, [_c_int] * 4 + [_c_ptr] * 7),
    "sputnik_hip_sddmm_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_sddmm_many_mask_workspace_bytes": (_c_size, [_c_int] * 5),
    "sputnik_hip_csr_transpose_many_mask_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_sddmm_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64,
                                                         _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr,
                                                         _c_size, _c_ptr]),
    "sputnik_hip_sddmm_plan": (_c_int, [_c_int] * 4 + [_c_ptr] * 4 + [_c_size, _c_ptr]),
    "sputnik_hip_sddmm_batched_planned": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr,
                                                                 _c_i64, _c_ptr, _c_i64, _c_ptr,
                                                                 _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_permute_band_size": (_c_int, []),
    "sputnik_hip_permute_banded_batched": (_c_int, [_c_int, _c_int, _c_ptr, _c_i64, _c_ptr, _c_ptr,
                                                   _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_spmm_permuted_supported": (_c_int, [_c_int] * 4),
    "sputnik_hip_spmm_permuted_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_i64, _c_ptr,
                                                                 _c_ptr, _c_ptr, _c_ptr, _c_i64,
                                                                 _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_spmm_group_supported": (_c_int, [_c_int] * 6),
    "sputnik_hip_spmm_group_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_i64, _c_i64, _c_int, _c_int,
                                                              _c_ptr]),
    "sputnik_hip_spmm_transposed_out_supported": (_c_int, [_c_int] * 5),
    "sputnik_hip_spmm_transposed_out_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_i64, _c_ptr, _c_ptr,
                                                                       _c_ptr, _c_ptr, _c_i64, _c_ptr,
                                                                       _c_int, _c_int, _c_ptr, _c_i64,
                                                                       _c_ptr]),
    "sputnik_hip_sddmm_sum_scratch_bytes": (_c_size, [_c_int] * 5),
    "sputnik_hip_sddmm_sum_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_sddmm_sum_plan": (_c_int, [_c_int] * 4 + [_c_ptr] * 4 + [_c_size, _c_ptr]),
    "sputnik_hip_sddmm_sum_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64,
                                                             _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_size,
                                                             _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sddmm_sum_batched_planned": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr,
                                                                     _c_i64, _c_ptr, _c_i64, _c_ptr,
                                                                     _c_ptr, _c_size, _c_ptr, _c_size,
                                                                     _c_ptr]),
    "sputnik_hip_sparse_softmax": (_c_int, [_c_int] * 3 + [_c_ptr] * 6),
    "sputnik_hip_sparse_softmax_batched": (_c_int, [_c_int] * 4 + [_c_ptr, _c_i64, _c_ptr, _c_ptr,
                                                                  _c_ptr, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_csr_transpose_workspace_bytes": (_c_size, [_c_int] * 3),
    "sputnik_hip_csr_transpose": (_c_int, [_c_int] * 4 + [_c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr,
                                                         _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr,
                                                         _c_size, _c_ptr]),
    "sputnik_hip_csr_transpose_route": (_c_int, [_c_int] * 3 + [_c_ptr] * 7),
    "sputnik_hip_csr_transpose_many_mask_route": (_c_int, [_c_int] * 4 + [_c_i64, _c_int, _c_int, _c_size,
                                                                         _c_ptr, _c_ptr]),
    "sputnik_hip_dense_to_csr_count": (_c_int, [_c_int] * 3 + [_c_ptr, _c_int, _c_int, _c_i64, _c_i64,
                                                              _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    "sputnik_hip_dense_to_csr_fill": (_c_int, [_c_int] * 3 + [_c_ptr, _c_int, _c_int, _c_i64, _c_i64,
                                                             _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    "sputnik_hip_dense_to_csr_launch_shape": (_c_int, [_c_int] * 4 + [_c_ptr] * 4),
    "sputnik_hip_csr_row_order": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr]),
    "sputnik_hip_csr_row_order_route": (_c_int, [_c_int] * 3 + [_c_ptr] * 4),
    "sputnik_hip_topk_to_csr": (_c_int, [_c_int, _c_int, _c_ptr, _c_int, _c_i64, _c_int, _c_i64, _c_ptr, _c_int,
                                         _c_i64, _c_ptr, _c_size] + [_c_ptr] * 5),
    "sputnik_hip_topk_to_csr_workspace_bytes": (_c_size, [_c_int] * 3),
    "sputnik_hip_topk_to_csr_launch_shape": (_c_int, [_c_int] * 4 + [_c_ptr] * 6),
    "sputnik_hip_random_csr": (_c_int, [_c_int] * 3 + [_c_i64, _c_int, _c_float, ctypes.c_uint, PhiloxState, _c_ptr,
                                        _c_ptr, _c_size] + [_c_ptr] * 5),
    "sputnik_hip_random_csr_workspace_bytes": (_c_size, [_c_int] * 3),
    "sputnik_hip_random_csr_launch_shape": (_c_int, [_c_int] * 3 + [_c_ptr] * 7),
    "sputnik_hip_attention_pattern_launch_shape": (_c_int, [_c_int, _c_int, _c_i64] + [_c_ptr] * 6),
    "sputnik_hip_attention_pattern_count": (_c_int, [_c_int, _c_int, ctypes.POINTER(AttentionPatternArgs), PhiloxState]
                                            + [_c_ptr] * 4),
    "sputnik_hip_attention_pattern_fill": (_c_int, [_c_int, _c_int, ctypes.POINTER(AttentionPatternArgs), PhiloxState,
                                                    _c_int] + [_c_ptr] * 4),
    "sputnik_hip_csr_regrow": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr, _c_ptr, _c_int, _c_i64,
                                        ctypes.c_uint, _c_ptr, _c_size] + [_c_ptr] * 4),
    "sputnik_hip_csr_regrow_workspace_bytes": (_c_size, [_c_int] * 3),
    "sputnik_hip_csr_regrow_launch_shape": (_c_int, [_c_int] * 4 + [_c_ptr] * 9),
    "sputnik_hip_csr_regrow_total": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_i64, _c_ptr, _c_int,
                                              _c_i64, ctypes.c_uint, _c_ptr, _c_size] + [_c_ptr] * 6),
    "sputnik_hip_csr_regrow_total_workspace_bytes": (_c_size, [_c_int] * 3),
    "sputnik_hip_csr_regrow_total_launch_shape": (_c_int, [_c_int] * 5 + [_c_ptr] * 14),
    "sputnik_hip_csr_regrow_random": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr, PhiloxState, _c_ptr,
                                               ctypes.c_uint, _c_int, _c_float, _c_ptr, _c_size] + [_c_ptr] * 4),
    "sputnik_hip_csr_regrow_total_random": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_i64, PhiloxState,
                                                     _c_ptr, ctypes.c_uint, _c_int, _c_float, _c_ptr, _c_size]
                                            + [_c_ptr] * 6),
    "sputnik_hip_csr_regrow_random_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_csr_regrow_random_launch_shape": (_c_int, [_c_int] * 5 + [_c_ptr] * 11),
    "sputnik_hip_csr_topk": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_int, _c_i64, _c_ptr, _c_size]
                             + [_c_ptr] * 5 + [_c_i64, _c_ptr]),
    "sputnik_hip_csr_topk_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_csr_topk_launch_shape": (_c_int, [_c_int] * 5 + [_c_ptr] * 8),
    "sputnik_hip_csr_topk_global_select": (_c_int, [_c_int] + [_c_ptr] * 4 + [_c_int, _c_i64, _c_ptr, _c_size]
                                           + [_c_ptr] * 3),
    "sputnik_hip_csr_topk_global_fill": (_c_int, [_c_int] + [_c_ptr] * 5 + [_c_int, _c_ptr, _c_size]
                                         + [_c_ptr] * 7),
    "sputnik_hip_csr_topk_global_workspace_bytes": (_c_size, [_c_int, _c_ptr]),
    "sputnik_hip_csr_topk_global_launch_shape": (_c_int, [_c_int, _c_ptr, _c_ptr, _c_int] + [_c_ptr] * 5),
    "sputnik_hip_csr_transpose_checked": (_c_int, [_c_int] * 4 + [_c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr,
                                                         _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr,
                                                         _c_size, _c_ptr]),
    # extensions
    "sputnik_hip_spmm_bias_batched": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_i64, _c_ptr, _c_ptr,
                                                             _c_ptr, _c_i64, _c_ptr, _c_int, _c_ptr,
                                                             _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_softmax_scaled_batched": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_float, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_sparse_softmax_backward_batched": (_c_int, [_c_int] * 3 + [
        _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_float, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_csr_transpose_typed": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_i64, _c_ptr, _c_ptr,
                                                               _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr,
                                                               _c_ptr, _c_size, _c_int, _c_ptr]),
    "sputnik_hip_spmm_typed_workspace_bytes": (_c_size, [_c_int] * 6 + [_c_i64, _c_int]),
    "sputnik_hip_spmm_typed": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_int, _c_i64, _c_ptr, _c_ptr,
                                                      _c_ptr, _c_int, _c_i64, _c_ptr, _c_int, _c_ptr,
                                                      _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sddmm_typed": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64,
                                                       _c_ptr, _c_i64, _c_int, _c_ptr, _c_i64,
                                                       _c_int, _c_ptr, _c_size, _c_int, _c_ptr]),
    "sputnik_hip_sddmm_sum_typed": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64,
                                                           _c_ptr, _c_i64, _c_int, _c_ptr, _c_ptr,
                                                           _c_size, _c_int, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_left_spmm_half_tiles_workspace_bytes": (_c_size, [_c_int] * 8),
    "sputnik_hip_left_spmm_half_tiles": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr,
                                                                _c_int, _c_i64, _c_int, _c_ptr, _c_int,
                                                                _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_linear_half_supported": (_c_int, [_c_int] * 7),
    "sputnik_hip_sparse_linear_half_image_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_sparse_linear_half_image": (_c_int, [_c_int] * 3 + [_c_ptr, _c_ptr, _c_ptr, _c_int, _c_int,
                                                                    _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_half_planes_bytes": (_c_size, [_c_i64, _c_int]),
    "sputnik_hip_half_planes": (_c_int, [_c_i64, _c_ptr, _c_int, _c_ptr, _c_ptr]),
    "sputnik_hip_sparse_linear_half_forward": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_ptr, _c_int,
                                                                      _c_ptr, _c_int, _c_ptr, _c_ptr]),
    "sputnik_hip_sparse_linear_half_rows_supported": (_c_int, [_c_int] * 7),
    "sputnik_hip_sparse_linear_half_rows_forward": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_ptr, _c_i64, _c_i64,
                                                                           _c_int, _c_ptr, _c_int, _c_i64, _c_i64,
                                                                           _c_ptr]),
    "sputnik_hip_sparse_linear_half_plan_bytes": (_c_size, [_c_int] * 2),
    "sputnik_hip_sparse_linear_half_plan": (_c_int, [_c_int] * 2 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    "sputnik_hip_sparse_linear_half_scratch_bytes": (_c_size, [_c_int] * 7),
    "sputnik_hip_sparse_linear_half_weight_gradient": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_int,
                                                                              _c_ptr, _c_int, _c_ptr, _c_ptr,
                                                                              _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_linear_half_weight_gradient_dense": (_c_int, [_c_int] * 5 + [
        _c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_sparse_linear_dense_weight_gradient_supported": (_c_int, [_c_int] * 8),
    "sputnik_hip_sparse_linear_dense_weight_gradient": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_int, _c_ptr, _c_int, _c_int, _c_int, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_sparse_linear_half_input_gradient": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_ptr, _c_int,
                                                                             _c_int, _c_ptr, _c_int, _c_ptr]),
    "sputnik_hip_sddmm_sum_group_planned": (_c_int, [_c_int] * 5 + [_c_ptr, _c_i64, _c_i64, _c_ptr]),
    "sputnik_hip_sddmm_sum_mixed_scratch_bytes": (_c_size, [_c_int] * 7),
    "sputnik_hip_sddmm_sum_mixed": (_c_int, [_c_int] * 5 + [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_int,
                                                           _c_i64, _c_ptr, _c_int, _c_i64, _c_ptr,
                                                           _c_ptr, _c_size, _c_int, _c_ptr, _c_size,
                                                           _c_ptr]),
    "sputnik_hip_sparse_softmax_typed": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_float, _c_ptr, _c_i64, _c_int, _c_ptr]),
    "sputnik_hip_sparse_softmax_backward_typed": (_c_int, [_c_int] * 3 + [
        _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_float, _c_ptr, _c_i64, _c_int, _c_ptr]),
    "sputnik_hip_sparse_attention_supported": (_c_int, [_c_int] * 4),
    "sputnik_hip_sparse_attention_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_sparse_attention_forward": (_c_int, [_c_int] * 5 + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_plan": (_c_int, [_c_int] * 4 + [_c_ptr] * 4 + [_c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_forward_planned": (_c_int, [_c_int] * 5 + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_supported": (_c_int, [_c_int] * 8 + [_c_ptr, _c_i64, _c_i64, _c_i64] * 4),
    "sputnik_hip_sparse_attention_heads_workspace_bytes": (_c_size, [_c_int] * 4),
    "sputnik_hip_sparse_attention_heads_forward": (_c_int, [_c_int] * 6 + [_c_ptr] * 3 + [_c_int] + [
        _c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [_c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64,
                                               _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_forward_planned": (_c_int, [_c_int] * 6 + [_c_ptr] * 3 + [_c_int] + [
        _c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [_c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64,
                                               _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_many_mask_workspace_bytes": (_c_size, [_c_int] * 5),
    "sputnik_hip_sparse_attention_many_mask_plan": (_c_int, [_c_int] * 4 + [_c_ptr] * 5 + [_c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_many_mask_forward": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int] + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_many_mask_forward_planned": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int] + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_many_mask_forward": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_int] + [
        _c_ptr] * 3 + [_c_int] + [_c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [
        _c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_many_mask_forward_planned": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_int, _c_int] + [_c_ptr] * 3 + [_c_int] + [_c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [
        _c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_dropout_typed": (_c_int, [_c_int] * 4 + [_c_ptr, _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr]),
    "sputnik_hip_sparse_attention_forward_dropout": (_c_int, [_c_int] * 5 + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_forward_planned_dropout": (_c_int, [_c_int] * 5 + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_backward_supported": (_c_int, [_c_int] * 4),
    "sputnik_hip_sparse_attention_backward_workspace_bytes": (_c_size, [_c_int] * 5),
    "sputnik_hip_sparse_attention_backward": (_c_int, [_c_int] * 5 + [_c_ptr] * 7 + [
        _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr, _c_i64, _c_ptr, _c_i64,
        _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64]
        + [ctypes.c_double, PhiloxState] + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_rows_supported": (_c_int, [_c_int] * 4),
    "sputnik_hip_sparse_attention_rows_forward": (_c_int, [_c_int] * 5 + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr]),
    "sputnik_hip_sparse_attention_heads_forward_dropout": (_c_int, [_c_int] * 6 + [_c_ptr] * 3 + [_c_int] + [
        _c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [_c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64]
        + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_forward_planned_dropout": (_c_int, [_c_int] * 6 + [_c_ptr] * 3 + [
        _c_int] + [_c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [
        _c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_many_mask_forward_dropout": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int] + [
        _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float, _c_ptr,
        _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_many_mask_forward_planned_dropout": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_int] + [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_float,
                           _c_ptr, _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_many_mask_forward_dropout": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_int, _c_int] + [_c_ptr] * 3 + [_c_int] + [_c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [
        _c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_attention_heads_many_mask_forward_planned_dropout": (_c_int, [_c_int] * 4 + [
        _c_ptr, _c_int, _c_int] + [_c_ptr] * 3 + [_c_int] + [_c_ptr, _c_i64, _c_i64, _c_i64] * 3 + [
        _c_float, _c_ptr, _c_int, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64] + _DROP + [_c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_spmm_many_mask": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_ptr, _c_ptr, _c_i64,
                                                          _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr,
                                                          _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sddmm_many_mask": (_c_int, [_c_int] * 4 + [_c_ptr, _c_int, _c_ptr, _c_ptr, _c_ptr,
                                                           _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr,
                                                           _c_i64, _c_ptr, _c_size, _c_ptr]),
    "sputnik_hip_sparse_softmax_many_mask": (_c_int, [_c_int] * 2 + [
        _c_ptr, _c_int, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_float, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_sparse_softmax_backward_many_mask": (_c_int, [_c_int] * 2 + [
        _c_ptr, _c_int, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_float, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_transpose_batched": (_c_int, [_c_int] * 3 + [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_permute_last_batched": (_c_int, [_c_int] * 2 + [_c_ptr, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_ptr]),
    "sputnik_hip_transpose_cast_batched": (_c_int, [_c_int] * 3 + [_c_ptr, _c_int, _c_i64, _c_ptr, _c_int,
                                                                  _c_i64, _c_ptr]),
    "sputnik_hip_csr_transpose_many_mask": (_c_int, [_c_int] * 3 + [
        _c_ptr, _c_int, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr,
        _c_ptr, _c_size, _c_ptr]),
}

_bound = None


def lib():
    global _bound
    if _bound is None:
        L = kernel_lib()
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library lacks the symbol
            fn.restype = restype
            fn.argtypes = argtypes
        _bound = L
    return _bound


def version():
    return lib().sputnik_hip_version().decode()


def build_id():
    """Hash of the kernel sources the loaded library was built from."""
    return lib().sputnik_hip_build_id().decode()


def spmm_kernel_name(m, k, n, nonzeros, replicas=1):
    """Device kernel the dispatcher picks for an SpMM call of this shape."""
    return lib().sputnik_hip_spmm_kernel_name(m, k, n, nonzeros, replicas).decode()


def spmm_typed_kernel_name(m, k, n, nonzeros, replicas, values_dtype, values_stride, dense_dtype):
    """Kernel spmm_typed takes for a call of this shape and these storage types (its own
    dispatch), with a workspace as large as spmm_typed_workspace_bytes asks.  Host only."""
    return lib().sputnik_hip_spmm_typed_kernel_name(m, k, n, nonzeros, replicas, TYPE_CODES[values_dtype],
                                                    values_stride, TYPE_CODES[dense_dtype]).decode()


def left_spmm_half_tiles_tile_rows(m, n, replicas):
    """Rows (128 / 256) of the matrix-core tile left_spmm_half_tiles launches.  Host only."""
    return lib().sputnik_hip_left_spmm_half_tiles_tile_rows(m, n, replicas)


def sddmm_kernel_name(m, k, n, nonzeros, replicas=1, elem_bytes=4, planned=False):
    """Device kernel the dispatcher picks for an SDDMM call of this shape."""
    return lib().sputnik_hip_sddmm_kernel_name(m, k, n, nonzeros, replicas, elem_bytes,
                                               int(bool(planned))).decode()


def _check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed with status {status}")


def _query(symbol, args, names, flags=("served",)):
    """One host query of the C API that answers through int out-parameters behind ``args``:
    -> a dict of ``names``, those among ``flags`` as bool.  Raises for a status other than 0."""
    outs = [_c_int(-1) for _ in names]
    _check(getattr(lib(), symbol)(*args, *[ctypes.cast(ctypes.pointer(o), _c_ptr) for o in outs]), symbol)
    return {name: bool(o.value) if name in flags else o.value for name, o in zip(names, outs)}


SUM_KERNELS = ("rowwave", "tiled", "mfma", "plain")   # SPUTNIK_HIP_SUM_ROWWAVE / _TILED / _MFMA / _PLAIN


def sddmm_sum_route(m, k, n, nonzeros, replicas, dtype=torch.float32, planned=False, mixed=False):
    """Route of a summed SDDMM call of this shape under the current options, with a workspace and
    scratch as large as the size queries ask: a dict of kernel (one of SUM_KERNELS), panel_width,
    panels, slab_rows and splits (include/sputnik_hip.h).  `mixed`: a (float32, half) pair whose
    half operand is `dtype`.  Host only."""
    route = _query("sputnik_hip_sddmm_sum_route",
                   (m, k, n, nonzeros, replicas, TYPE_CODES[dtype], int(bool(planned)), int(bool(mixed))),
                   ("kernel", "panel_width", "panels", "slab_rows", "splits"))
    route["kernel"] = SUM_KERNELS[route["kernel"]]
    return route


SDDMM_FAMILIES = ("rowwave", "flat", "quad", "stationary", "mfma")   # SPUTNIK_HIP_SDDMM_ROWWAVE / ...


def sddmm_launch_shape(m, k, n, nonzeros, replicas, dtype=torch.float32, out_dtype=torch.float32,
                       planned=False, summed=False, mask_heads=0):
    """What an SDDMM call of this shape launches under the current options: a dict of family (one
    of SDDMM_FAMILIES), panel_width, slab_rows, passes, accumulates, grid_x, grid_y, grid_z and
    row_blocks (include/sputnik_hip.h).  `summed`: the summed form; `mask_heads` > 0: a many-mask
    call, `nonzeros` the largest mask's count.  Host only."""
    shape = _query("sputnik_hip_sddmm_launch_shape",
                   (m, k, n, nonzeros, replicas, TYPE_CODES[dtype], TYPE_CODES[out_dtype], int(bool(planned)),
                    int(bool(summed)), mask_heads),
                   ("family", "panel_width", "slab_rows", "passes", "accumulates", "grid_x", "grid_y", "grid_z",
                    "row_blocks"), flags=("accumulates",))
    shape["family"] = SDDMM_FAMILIES[shape["family"]]
    return shape


SPMM_FAMILIES = ("rowgather", "panel", "narrow64", "wide256", "wide512", "flat")   # SPUTNIK_HIP_SPMM_*


class SpmmLaunch(ctypes.Structure):
    """sputnik_hip_spmm_launch (include/sputnik_hip.h)."""
    _fields_ = [(name, _c_int) for name in
                ("family", "tile_cols", "tile_rows", "waves", "rows_per_wave", "chunk", "sparse", "batch",
                 "grid_x", "grid_y", "slots", "nchunks", "n_tiles", "ksplits")] + \
               [(name, _c_i64) for name in
                ("workspace_bytes", "row_ok_offset", "table_offset", "partials_offset")]


def spmm_launch_shape(m, k, n, nonzeros, replicas, out_alignment=16):
    """What a float32 SpMM call of this shape launches under the current options: a dict of family
    (one of SPMM_FAMILIES) and, for the LDS-tiled kernels, tile_cols, tile_rows, waves,
    rows_per_wave, chunk, sparse, batch, grid_x, grid_y, slots, nchunks, n_tiles, ksplits,
    workspace_bytes and the byte offsets row_ok_offset, table_offset, partials_offset of the
    kernel's tables in the workspace (include/sputnik_hip.h).  `out_alignment`: bytes the output
    pointer is aligned to.  Host only."""
    launch = SpmmLaunch()
    _check(lib().sputnik_hip_spmm_launch_shape(m, k, n, nonzeros, replicas, out_alignment,
                                               ctypes.cast(ctypes.pointer(launch), _c_ptr)),
           "sputnik_hip_spmm_launch_shape")
    shape = {name: getattr(launch, name) for name, _ in SpmmLaunch._fields_}
    shape["family"] = SPMM_FAMILIES[shape["family"]]
    shape["sparse"] = bool(shape["sparse"])
    return shape


def sparse_softmax_route(m, nonzeros, replicas, dtype=torch.float32, backward=False):
    """Kernel instance the sparse softmax launches for a call of this shape under the current
    options: a dict of lanes_per_row, base_pieces, pieces (the class), rows_per_group, depth
    and nontemporal.  Host only."""
    return _query("sputnik_hip_sparse_softmax_route", (m, nonzeros, replicas, TYPE_CODES[dtype], int(bool(backward))),
                  ("lanes_per_row", "base_pieces", "pieces", "rows_per_group", "depth", "nontemporal"))


def reload_options():
    """Re-read the SPUTNIK_HIP_* knobs from the environment (read once otherwise)."""
    lib().sputnik_hip_reload_options()


def _ptr(t):
    return None if t is None else _c_ptr(t.data_ptr())


def _stream(t):
    return _c_ptr(torch.cuda.current_stream(t.device).cuda_stream)


def _require(t, dtype, name):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous {dtype} GPU tensor, got "
                         f"{t.dtype} on {t.device}, contiguous={t.is_contiguous()}")


def spmm_workspace_bytes(m, k, n, nonzeros):
    return lib().sputnik_hip_spmm_workspace_bytes(m, k, n, nonzeros)


def spmm(m, k, n, row_indices, values, row_offsets, column_indices, dense, out):
    """sputnik_hip_spmm: one 2-D SpMM, arguments in sputnik::CudaSpmm order."""
    nonzeros = column_indices.numel()
    _check(lib().sputnik_hip_spmm(m, k, n, nonzeros, _ptr(row_indices), _ptr(values),
                                  _ptr(row_offsets), _ptr(column_indices), _ptr(dense),
                                  _ptr(out), _stream(out)), "sputnik_hip_spmm")
    return out


def spmm_batched(m, k, n, replicas, row_indices, values, values_stride, row_offsets,
                 column_indices, dense, out, workspace=None):
    nonzeros = column_indices.numel()
    for t, d, nm in ((row_indices, torch.int32, "row_indices"), (values, torch.float32, "values"),
                     (row_offsets, torch.int32, "row_offsets"),
                     (column_indices, torch.int32, "column_indices"),
                     (dense, torch.float32, "dense"), (out, torch.float32, "out")):
        _require(t, d, nm)
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    _check(lib().sputnik_hip_spmm_batched(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(values), values_stride,
        _ptr(row_offsets), _ptr(column_indices), _ptr(dense), k * n, _ptr(out), m * n,
        _ptr(workspace), ws_bytes, _stream(out)), "sputnik_hip_spmm_batched")
    return out


def spmm_plan(m, k, n, row_indices, row_offsets, column_indices, workspace):
    """Topology-only pre-pass into `workspace` (reusable by spmm_batched_planned)."""
    nonzeros = column_indices.numel()
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    _check(lib().sputnik_hip_spmm_plan(m, k, n, nonzeros, _ptr(row_indices), _ptr(row_offsets),
                                       _ptr(column_indices), _ptr(workspace), ws_bytes,
                                       _stream(row_offsets)), "sputnik_hip_spmm_plan")
    return workspace


def spmm_batched_planned(m, k, n, replicas, row_indices, values, values_stride, row_offsets,
                         column_indices, dense, out, workspace):
    nonzeros = column_indices.numel()
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    _check(lib().sputnik_hip_spmm_batched_planned(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(values), values_stride,
        _ptr(row_offsets), _ptr(column_indices), _ptr(dense), k * n, _ptr(out), m * n,
        _ptr(workspace), ws_bytes, _stream(out)), "sputnik_hip_spmm_batched_planned")
    return out


def sddmm_workspace_bytes(m, k, n, nonzeros):
    return lib().sputnik_hip_sddmm_workspace_bytes(m, k, n, nonzeros)


def sddmm_batched(m, k, n, replicas, row_indices, row_offsets, column_indices, lhs, rhs, out,
                  workspace=None):
    nonzeros = column_indices.numel()
    for t, d, nm in ((row_indices, torch.int32, "row_indices"),
                     (row_offsets, torch.int32, "row_offsets"),
                     (column_indices, torch.int32, "column_indices"),
                     (lhs, torch.float32, "lhs"), (rhs, torch.float32, "rhs"),
                     (out, torch.float32, "out")):
        _require(t, d, nm)
    _check(lib().sputnik_hip_sddmm_batched(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(lhs), m * k, _ptr(rhs), n * k, _ptr(out), nonzeros, _ptr(workspace),
        0 if workspace is None else workspace.numel() * workspace.element_size(), _stream(out)),
        "sputnik_hip_sddmm_batched")
    return out


def sparse_softmax_batched(m, replicas, values, row_indices, row_offsets, column_indices, out):
    nonzeros = column_indices.numel()
    for t, d, nm in ((values, torch.float32, "values"), (row_indices, torch.int32, "row_indices"),
                     (row_offsets, torch.int32, "row_offsets"),
                     (column_indices, torch.int32, "column_indices"),
                     (out, torch.float32, "out")):
        _require(t, d, nm)
    _check(lib().sputnik_hip_sparse_softmax_batched(
        m, -1, nonzeros, replicas, _ptr(values), nonzeros, _ptr(row_indices), _ptr(row_offsets),
        _ptr(column_indices), _ptr(out), nonzeros, _stream(out)),
        "sputnik_hip_sparse_softmax_batched")
    return out


def csr_transpose_workspace_bytes(m, n, nonzeros):
    return lib().sputnik_hip_csr_transpose_workspace_bytes(m, n, nonzeros)


TRANSPOSE_PATHS = ("none", "grouped", "wide", "sparse")   # SPUTNIK_HIP_TRANSPOSE_NONE / _GROUPED / _WIDE / _SPARSE


def csr_transpose_route(m, n, nonzeros):
    """Launches csr_transpose makes for a call of this shape: a dict of path (one of
    TRANSPOSE_PATHS), chunks, ranges, groups, parts, scan_chunks_per_group and long_rank_launch
    (include/sputnik_hip.h); -1 where a field does not apply to the path.  Host only."""
    route = _query("sputnik_hip_csr_transpose_route", (m, n, nonzeros),
                   ("path", "chunks", "ranges", "groups", "parts", "scan_chunks_per_group", "long_rank_launch"))
    route["path"] = TRANSPOSE_PATHS[route["path"]]
    return route


MANY_VALUES = ("none", "scatter", "gather")   # SPUTNIK_HIP_MANY_VALUES_NONE / _SCATTER / _GATHER


def csr_transpose_many_mask_route(masks, m, n, nonzeros, heads, with_permutation, workspace_bytes):
    """What csr_transpose_many_mask does for masks of these entry counts (a sequence) with `heads`
    value rows per mask (0: no values) in a workspace of that size: a dict of one_launch (bool;
    False = mask after mask) and values_by (one of MANY_VALUES, None mask after mask).  Host only."""
    counts = [int(c) for c in nonzeros]
    outs = [_c_int(-1), _c_int(-1)]
    _check(lib().sputnik_hip_csr_transpose_many_mask_route(
        masks, m, n, max(counts, default=0), sum(counts), heads, int(bool(with_permutation)),
        workspace_bytes, *[ctypes.cast(ctypes.pointer(o), _c_ptr) for o in outs]),
        "sputnik_hip_csr_transpose_many_mask_route")
    one_launch, values_by = bool(outs[0].value), outs[1].value
    return {"one_launch": one_launch, "values_by": MANY_VALUES[values_by] if values_by >= 0 else None}


def dense_to_csr_launch_shape(masks, m, n, element_bytes):
    """The count / fill instance of the device topology build for `masks` dense matrices of
    m x n elements of that width: a dict of rows_per_wave, elements_per_lane, rows_per_workgroup
    and grid (include/sputnik_hip.h).  Host only; raises for sizes the entries reject."""
    return _query("sputnik_hip_dense_to_csr_launch_shape", (masks, m, n, element_bytes),
                  ("rows_per_wave", "elements_per_lane", "rows_per_workgroup", "grid"))


def csr_row_order_route(masks, m, n):
    """Whether the row-order kernel serves `masks` masks of m rows and n columns, and how: a dict
    of served (bool), capacity, threads and sort_size (include/sputnik_hip.h; -1 where it does
    not serve).  Host only."""
    return _query("sputnik_hip_csr_row_order_route", (masks, m, n), ("served", "capacity", "threads", "sort_size"))


def topk_to_csr_launch_shape(m, n, element_bytes, total):
    """The instance of the device top-k-to-CSR build for m x n scores of that width (2 or 4
    bytes), ``total`` mode or per row: a dict of served (bool; total mode stops at the row-order
    kernel's rows), rows_per_wave, elements_per_lane, rows_per_workgroup, digit_passes and grid
    (include/sputnik_hip.h).  Host only; raises for sizes the entry rejects."""
    return _query("sputnik_hip_topk_to_csr_launch_shape", (m, n, element_bytes, int(bool(total))),
                  ("served", "rows_per_wave", "elements_per_lane", "rows_per_workgroup", "digit_passes", "grid"))


def random_csr_launch_shape(m, n, total):
    """The instance of the device draw of a random m x n topology, ``total`` mode or per row: a
    dict of served (bool; total mode stops at the row-order kernel's rows), rows_per_wave,
    elements_per_lane, rows_per_workgroup, digit_passes, grid and launches (1 per row, 9 in
    total mode; include/sputnik_hip.h).  Host only; raises for sizes the entry rejects."""
    return _query("sputnik_hip_random_csr_launch_shape", (m, n, int(bool(total))),
                  ("served", "rows_per_wave", "elements_per_lane", "rows_per_workgroup", "digit_passes", "grid",
                   "launches"))


def random_csr_workspace_bytes(m, n, total):
    """Bytes of workspace sputnik_hip_random_csr wants (0 per row).  Host only."""
    return int(lib().sputnik_hip_random_csr_workspace_bytes(m, n, int(bool(total))))


def attention_pattern_launch_shape(m, n, offset=0):
    """The instance of the device build of an attention pattern over m rows and n columns at
    that offset: a dict of served (bool: m <= 16384, m * n <= INT_MAX, |offset| < 2**30; the
    other fields are -1 where it is not), rows_per_wave, columns_per_lane (4),
    rows_per_workgroup, grid and launches (4: count, scan, fill, row order;
    include/sputnik_hip.h).  Host only; sizes beyond int32 and offsets beyond int64 are not
    served, negative sizes raise."""
    m, n, offset = int(m), int(n), int(offset)
    if m > 2 ** 31 - 1 or n > 2 ** 31 - 1 or abs(offset) >= 2 ** 63:
        return dict(served=False, rows_per_wave=-1, columns_per_lane=-1, rows_per_workgroup=-1, grid=-1, launches=-1)
    return _query("sputnik_hip_attention_pattern_launch_shape", (max(m, -1), max(n, -1), offset),
                  ("served", "rows_per_wave", "columns_per_lane", "rows_per_workgroup", "grid", "launches"))


def csr_regrow_launch_shape(m, n, score_bytes, value_bytes):
    """The instance of the per-row drop-and-grow kernel for an m x n pattern with scores and
    values of those widths (2 or 4 bytes): a dict of served (bool: n <= max_n; the fields but
    max_n are -1 where it is not), rows_per_wave, elements_per_lane, rows_per_workgroup,
    value_digit_passes, score_digit_passes, lds_bytes, max_n and grid (include/sputnik_hip.h).
    Host only; raises for sizes the entry rejects."""
    return _query("sputnik_hip_csr_regrow_launch_shape", (m, n, score_bytes, value_bytes),
                  ("served", "rows_per_wave", "elements_per_lane", "rows_per_workgroup", "value_digit_passes",
                   "score_digit_passes", "lds_bytes", "max_n", "grid"))


def csr_regrow_total_launch_shape(m, n, nonzeros, score_bytes, value_bytes):
    """The instances of the matrix-wide drop-and-grow step for an m x n pattern of `nonzeros`
    entries with scores and values of those widths (2 or 4 bytes): a dict of served (bool:
    m <= max_m and n <= max_n; the fields but the two limits are -1 where it is not),
    rows_per_wave, elements_per_lane, rows_per_workgroup, value_digit_passes, score_digit_passes,
    lds_bytes, max_m, max_n, grid, value_rows_per_wave, value_rows_grid, flat_grid and launches
    (include/sputnik_hip.h).  Host only; raises for sizes the entry rejects."""
    return _query("sputnik_hip_csr_regrow_total_launch_shape", (m, n, nonzeros, score_bytes, value_bytes),
                  ("served", "rows_per_wave", "elements_per_lane", "rows_per_workgroup", "value_digit_passes",
                   "score_digit_passes", "lds_bytes", "max_m", "max_n", "grid", "value_rows_per_wave",
                   "value_rows_grid", "flat_grid", "launches"))


def csr_regrow_total_workspace_bytes(m, n, nonzeros):
    """Bytes of workspace one matrix-wide drop-and-grow call takes (host only): two sets of bins,
    thresholds, quotas and tie counts, the kept lengths, and 2 * m * ceil(n / 32) words of bit
    planes."""
    return lib().sputnik_hip_csr_regrow_total_workspace_bytes(m, n, nonzeros)


def csr_regrow_random_launch_shape(m, n, nonzeros, value_bytes, total):
    """The instances of the drop-and-grow step under generated scores (SET) for an m x n pattern
    of `nonzeros` values of that width (2 or 4 bytes), ``total`` (matrix-wide) or per row: a
    dict of served (bool: per row n <= max_n = 61440; matrix-wide m <= max_m = 16384 and
    n <= max_n = 65536; the other fields are -1 where it is not), rows_per_wave,
    elements_per_lane, rows_per_workgroup, value_digit_passes, score_digit_passes (4: 32-bit
    keys), lds_bytes, max_m (-1 per row), max_n, grid and launches (1 per row, 8 +
    value_digit_passes + 4 matrix-wide; include/sputnik_hip.h).  Host only; raises for sizes
    the entry rejects."""
    return _query("sputnik_hip_csr_regrow_random_launch_shape", (m, n, nonzeros, value_bytes, int(bool(total))),
                  ("served", "rows_per_wave", "elements_per_lane", "rows_per_workgroup", "value_digit_passes",
                   "score_digit_passes", "lds_bytes", "max_m", "max_n", "grid", "launches"))


def csr_regrow_random_workspace_bytes(m, n, nonzeros, total):
    """Bytes of workspace one drop-and-grow call under generated scores takes (0 per row, that of
    ``csr_regrow_total_workspace_bytes`` matrix-wide).  Host only."""
    return int(lib().sputnik_hip_csr_regrow_random_workspace_bytes(m, n, nonzeros, int(bool(total))))


def csr_topk_launch_shape(m, n, nonzeros, value_bytes, total):
    """The instance of the top-k over the entries of an m x n CSR pattern of `nonzeros` values of
    that width (2 or 4 bytes), ``total`` mode or per row: a dict of served (bool: m within the
    row-order kernel's rows; the other fields are -1 where it is not), rows_per_wave,
    group_lanes, elements_per_lane, rows_per_workgroup, digit_passes, rows_grid and flat_grid
    (include/sputnik_hip.h).  The group width follows the mean row length ``nonzeros // m``.
    Host only; raises for sizes the entry rejects."""
    return _query("sputnik_hip_csr_topk_launch_shape", (m, n, nonzeros, value_bytes, int(bool(total))),
                  ("served", "rows_per_wave", "group_lanes", "elements_per_lane", "rows_per_workgroup", "digit_passes",
                   "rows_grid", "flat_grid"))


def csr_topk_global_launch_shape(rows, nonzeros, value_bytes):
    """The instance of the one top-k across several CSR patterns (``rows[l]`` rows and
    ``nonzeros[l]`` values of that width, 2 or 4 bytes, per layer): a dict of served (bool: every
    layer within the row-order kernel's rows and the entries within int32; the other fields are
    -1 where it is not), digit_passes, layers_per_launch (layers one digit launch takes in its
    argument table), elements_per_workgroup (entries one workgroup of the flat walk covers) and
    digit_launches (include/sputnik_hip.h).  Host only; raises for sizes the entry rejects."""
    if len(rows) != len(nonzeros):
        raise ValueError(f"csr_topk_global_launch_shape: {len(rows)} rows for {len(nonzeros)} nonzeros")
    layers = len(rows)
    c_rows, c_nonzeros = (_c_int * layers)(*rows), (_c_int * layers)(*nonzeros)
    return _query("sputnik_hip_csr_topk_global_launch_shape",
                  (layers, ctypes.cast(c_rows, _c_ptr), ctypes.cast(c_nonzeros, _c_ptr), value_bytes),
                  ("served", "digit_passes", "layers_per_launch", "elements_per_workgroup", "digit_launches"))


def csr_transpose(m, n, replicas, values, row_offsets, column_indices, out_values,
                  out_row_offsets, out_column_indices, out_permutation, workspace, checked=False):
    """``checked``: the synchronising entry, which raises for a pattern the transpose
    is not defined for (a row storing a column twice, a column out of range)."""
    nonzeros = column_indices.numel()
    for t, d, nm in ((values, torch.float32, "values"), (row_offsets, torch.int32, "row_offsets"),
                     (column_indices, torch.int32, "column_indices"),
                     (out_values, torch.float32, "out_values"),
                     (out_row_offsets, torch.int32, "out_row_offsets"),
                     (out_column_indices, torch.int32, "out_column_indices")):
        _require(t, d, nm)
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    entry = lib().sputnik_hip_csr_transpose_checked if checked else lib().sputnik_hip_csr_transpose
    _check(entry(
        m, n, nonzeros, replicas, _ptr(values), nonzeros, _ptr(row_offsets), _ptr(column_indices),
        _ptr(out_values), nonzeros, _ptr(out_row_offsets), _ptr(out_column_indices),
        _ptr(out_permutation), _ptr(workspace), ws_bytes, _stream(out_values)),
        "sputnik_hip_csr_transpose")
    return out_values, out_row_offsets, out_column_indices


# ---------------------------------------------------------------------------
# extensions
# ---------------------------------------------------------------------------
def _ws_bytes(workspace):
    return 0 if workspace is None else workspace.numel() * workspace.element_size()


def spmm_bias_batched(m, k, n, replicas, row_indices, values, values_stride, row_offsets,
                      column_indices, dense, bias, relu, out, workspace=None):
    nonzeros = column_indices.numel()
    for t, d, nm in ((row_indices, torch.int32, "row_indices"), (values, torch.float32, "values"),
                     (row_offsets, torch.int32, "row_offsets"),
                     (column_indices, torch.int32, "column_indices"),
                     (dense, torch.float32, "dense"), (out, torch.float32, "out")):
        _require(t, d, nm)
    if bias is not None:
        _require(bias, torch.float32, "bias")
        if bias.numel() != m:
            raise ValueError(f"bias: expected {m} elements, got {bias.numel()}")
    _check(lib().sputnik_hip_spmm_bias_batched(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(values), values_stride,
        _ptr(row_offsets), _ptr(column_indices), _ptr(dense), k * n, _ptr(bias), int(bool(relu)),
        _ptr(out), m * n, _ptr(workspace), _ws_bytes(workspace), _stream(out)),
        "sputnik_hip_spmm_bias_batched")
    return out


def _stride(stride, nonzeros):
    return nonzeros if stride is None else int(stride)


def sparse_softmax_scaled_batched(m, replicas, values, row_indices, row_offsets, column_indices,
                                  scale, out, *, values_stride=None, out_stride=None):
    """Replica r of an operand begins r * its stride elements into the tensor (default: the
    rows follow each other, stride = nonzeros)."""
    nonzeros = column_indices.numel()
    for t, d, nm in ((values, torch.float32, "values"), (row_indices, torch.int32, "row_indices"),
                     (row_offsets, torch.int32, "row_offsets"),
                     (column_indices, torch.int32, "column_indices"),
                     (out, torch.float32, "out")):
        _require(t, d, nm)
    _check(lib().sputnik_hip_sparse_softmax_scaled_batched(
        m, -1, nonzeros, replicas, _ptr(values), _stride(values_stride, nonzeros), _ptr(row_indices),
        _ptr(row_offsets), _ptr(column_indices), float(scale), _ptr(out),
        _stride(out_stride, nonzeros), _stream(out)),
        "sputnik_hip_sparse_softmax_scaled_batched")
    return out


def sparse_softmax_backward_batched(m, replicas, softmax_out, grad_out, row_offsets, scale,
                                    grad_values, *, nonzeros=None, softmax_out_stride=None,
                                    grad_out_stride=None, grad_values_stride=None):
    """`nonzeros` (default: the last dimension of softmax_out) and one stride per operand
    (default: nonzeros) describe operands that are flat views into padded buffers."""
    if nonzeros is None:
        nonzeros = softmax_out.shape[-1]
    for t, d, nm in ((softmax_out, torch.float32, "softmax_out"),
                     (grad_out, torch.float32, "grad_out"),
                     (row_offsets, torch.int32, "row_offsets"),
                     (grad_values, torch.float32, "grad_values")):
        _require(t, d, nm)
    _check(lib().sputnik_hip_sparse_softmax_backward_batched(
        m, nonzeros, replicas, _ptr(softmax_out), _stride(softmax_out_stride, nonzeros),
        _ptr(grad_out), _stride(grad_out_stride, nonzeros), _ptr(row_offsets), float(scale),
        _ptr(grad_values), _stride(grad_values_stride, nonzeros), _stream(grad_values)),
        "sputnik_hip_sparse_softmax_backward_batched")
    return grad_values


TYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}   # SPUTNIK_HIP_F32 / F16 / BF16


def _type_code(*tensors):
    dtype = tensors[0].dtype
    if dtype not in TYPE_CODES or any(t.dtype != dtype for t in tensors):
        raise TypeError("operands must share one of float32 / float16 / bfloat16, got "
                        + ", ".join(str(t.dtype) for t in tensors))
    return TYPE_CODES[dtype]


def csr_transpose_typed(m, n, replicas, values, row_offsets, column_indices, out_values,
                        out_row_offsets, out_column_indices, out_permutation, workspace,
                        checked=False):
    """csr_transpose of float32 / float16 / bfloat16 values; transposed values float32."""
    nonzeros = column_indices.numel()
    _require(out_values, torch.float32, "out_values")
    _check(lib().sputnik_hip_csr_transpose_typed(
        m, n, nonzeros, replicas, _ptr(values), _type_code(values), nonzeros, _ptr(row_offsets),
        _ptr(column_indices), _ptr(out_values), nonzeros, _ptr(out_row_offsets),
        _ptr(out_column_indices), _ptr(out_permutation), _ptr(workspace), _ws_bytes(workspace),
        int(bool(checked)), _stream(out_values)), "sputnik_hip_csr_transpose_typed")
    return out_values


def spmm_typed_workspace_bytes(m, k, n, nonzeros, replicas, values, values_stride, dense):
    return lib().sputnik_hip_spmm_typed_workspace_bytes(m, k, n, nonzeros, replicas,
                                                        _type_code(values), values_stride,
                                                        _type_code(dense))


def spmm_typed(m, k, n, replicas, row_indices, values, values_stride, row_offsets, column_indices,
               dense, out, workspace=None, bias=None, relu=False):
    """SpMM with values / dense stored as float32, float16 or bfloat16; out float32."""
    nonzeros = column_indices.numel()
    for t, nm in ((row_indices, "row_indices"), (row_offsets, "row_offsets"),
                  (column_indices, "column_indices")):
        _require(t, torch.int32, nm)
    _require(out, torch.float32, "out")
    for t, nm in ((values, "values"), (dense, "dense")):
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError(f"{nm}: expected a contiguous GPU tensor")
    _check(lib().sputnik_hip_spmm_typed(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(values), _type_code(values),
        values_stride, _ptr(row_offsets), _ptr(column_indices), _ptr(dense), _type_code(dense),
        k * n, _ptr(bias), int(bool(relu)), _ptr(out), m * n, _ptr(workspace),
        _ws_bytes(workspace), _stream(out)), "sputnik_hip_spmm_typed")
    return out


def sddmm_typed(m, k, n, replicas, row_indices, row_offsets, column_indices, lhs, rhs, out,
                workspace=None, planned=False):
    """SDDMM on float32 / float16 / bfloat16 operands (lhs, rhs alike); out float32 or
    the operands' type."""
    nonzeros = column_indices.numel()
    for t, nm in ((row_indices, "row_indices"), (row_offsets, "row_offsets"),
                  (column_indices, "column_indices")):
        _require(t, torch.int32, nm)
    in_code = _type_code(lhs, rhs)
    out_code = _type_code(out)
    for t, nm in ((lhs, "lhs"), (rhs, "rhs"), (out, "out")):
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError(f"{nm}: expected a contiguous GPU tensor")
    _check(lib().sputnik_hip_sddmm_typed(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(lhs), m * k, _ptr(rhs), n * k, in_code, _ptr(out), nonzeros, out_code, _ptr(workspace),
        _ws_bytes(workspace), int(bool(planned)), _stream(out)), "sputnik_hip_sddmm_typed")
    return out


def sparse_softmax_typed(m, replicas, values, row_indices, row_offsets, column_indices, scale, out,
                         *, values_stride=None, out_stride=None):
    """softmax(scale * values) on float32 / float16 / bfloat16 storage (in and out alike);
    strides in elements, default nonzeros."""
    nonzeros = column_indices.numel()
    for t, nm in ((row_indices, "row_indices"), (row_offsets, "row_offsets"),
                  (column_indices, "column_indices")):
        _require(t, torch.int32, nm)
    code = _type_code(values, out)
    _check(lib().sputnik_hip_sparse_softmax_typed(
        m, -1, nonzeros, replicas, _ptr(values), _stride(values_stride, nonzeros), _ptr(row_indices),
        _ptr(row_offsets), _ptr(column_indices), float(scale), _ptr(out),
        _stride(out_stride, nonzeros), code, _stream(out)),
        "sputnik_hip_sparse_softmax_typed")
    return out


def sparse_softmax_backward_typed(m, replicas, softmax_out, grad_out, row_offsets, scale,
                                  grad_values, *, nonzeros=None, softmax_out_stride=None,
                                  grad_out_stride=None, grad_values_stride=None):
    """`nonzeros` (default: the last dimension of softmax_out) and one stride per operand, in
    elements (default: nonzeros)."""
    if nonzeros is None:
        nonzeros = softmax_out.shape[-1]
    _require(row_offsets, torch.int32, "row_offsets")
    code = _type_code(softmax_out, grad_out, grad_values)
    _check(lib().sputnik_hip_sparse_softmax_backward_typed(
        m, nonzeros, replicas, _ptr(softmax_out), _stride(softmax_out_stride, nonzeros),
        _ptr(grad_out), _stride(grad_out_stride, nonzeros), _ptr(row_offsets), float(scale),
        _ptr(grad_values), _stride(grad_values_stride, nonzeros), code, _stream(grad_values)),
        "sputnik_hip_sparse_softmax_backward_typed")
    return grad_values


def _host_counts(nonzeros):
    """[masks] nonzero counts as a C int array living on the host."""
    counts = [int(x) for x in (nonzeros.tolist() if torch.is_tensor(nonzeros) else nonzeros)]
    return (ctypes.c_int * len(counts))(*counts), counts


def spmm_many_mask(masks, m, k, n, nonzeros, replicas, row_indices, values, row_offsets,
                   column_indices, dense, out, workspace=None):
    arr, _ = _host_counts(nonzeros)
    _check(lib().sputnik_hip_spmm_many_mask(
        masks, m, k, n, arr, replicas, _ptr(row_indices), _ptr(values), values.shape[-1],
        _ptr(row_offsets), _ptr(column_indices), _ptr(dense), k * n, _ptr(out), m * n,
        _ptr(workspace), _ws_bytes(workspace), _stream(out)), "sputnik_hip_spmm_many_mask")
    return out


def sddmm_many_mask_workspace_bytes(masks, m, k, n, largest_nonzeros):
    """One plan per mask: with it all masks run on the LDS-tiled kernel in one launch."""
    return lib().sputnik_hip_sddmm_many_mask_workspace_bytes(masks, m, k, n, largest_nonzeros)


def sddmm_many_mask(masks, m, k, n, nonzeros, replicas, row_indices, row_offsets, column_indices,
                    lhs, rhs, out, workspace=None):
    arr, _ = _host_counts(nonzeros)
    _check(lib().sputnik_hip_sddmm_many_mask(
        masks, m, k, n, arr, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(lhs), m * k, _ptr(rhs), n * k, _ptr(out), out.shape[-1], _ptr(workspace),
        _ws_bytes(workspace), _stream(out)), "sputnik_hip_sddmm_many_mask")
    return out


def sparse_softmax_many_mask(masks, m, nonzeros, replicas, values, row_indices, row_offsets,
                             column_indices, scale, out):
    arr, _ = _host_counts(nonzeros)
    _check(lib().sputnik_hip_sparse_softmax_many_mask(
        masks, m, arr, replicas, _ptr(values), values.shape[-1], _ptr(row_indices),
        _ptr(row_offsets), _ptr(column_indices), float(scale), _ptr(out), out.shape[-1],
        _stream(out)), "sputnik_hip_sparse_softmax_many_mask")
    return out


def sparse_softmax_backward_many_mask(masks, m, nonzeros, replicas, softmax_out, grad_out,
                                      row_offsets, scale, grad_values):
    arr, _ = _host_counts(nonzeros)
    _check(lib().sputnik_hip_sparse_softmax_backward_many_mask(
        masks, m, arr, replicas, _ptr(softmax_out), softmax_out.shape[-1], _ptr(grad_out),
        grad_out.shape[-1], _ptr(row_offsets), float(scale), _ptr(grad_values),
        grad_values.shape[-1], _stream(grad_values)),
        "sputnik_hip_sparse_softmax_backward_many_mask")
    return grad_values


def csr_transpose_many_mask_workspace_bytes(masks, m, n, largest_nonzeros):
    """A region of tables per mask: with it all masks are transposed by the same three launches."""
    return lib().sputnik_hip_csr_transpose_many_mask_workspace_bytes(masks, m, n, largest_nonzeros)


def csr_transpose_many_mask(masks, m, n, nonzeros, replicas, values, row_offsets, column_indices,
                            out_values, out_row_offsets, out_column_indices, out_permutation,
                            workspace):
    arr, _ = _host_counts(nonzeros)
    _check(lib().sputnik_hip_csr_transpose_many_mask(
        masks, m, n, arr, replicas, _ptr(values), 0 if values is None else values.shape[-1],
        _ptr(row_offsets), _ptr(column_indices), _ptr(out_values),
        0 if out_values is None else out_values.shape[-1], _ptr(out_row_offsets),
        _ptr(out_column_indices), _ptr(out_permutation), _ptr(workspace), _ws_bytes(workspace),
        _stream(out_row_offsets)), "sputnik_hip_csr_transpose_many_mask")
    return out_values, out_row_offsets, out_column_indices


def sparse_attention_supported(m, n, d, nonzeros):
    return bool(lib().sputnik_hip_sparse_attention_supported(m, n, d, nonzeros))


def sparse_attention_workspace_bytes(m, n, d, nonzeros):
    return lib().sputnik_hip_sparse_attention_workspace_bytes(m, n, d, nonzeros)


def _drop(p, rng, rng_state_out):
    """The (p, state, rng_state_out) arguments of a `_dropout` entry point, or () for the form
    without them: no state and no output given.  `rng`: a PhiloxState, or (seed, offset)."""
    if rng is None and rng_state_out is None:
        if p:
            raise ValueError("dropout needs a Philox state: rng=PhiloxState(...) or (seed, offset)")
        return ()
    if rng is None:
        rng = PhiloxState()
    elif not isinstance(rng, PhiloxState):
        rng = PhiloxState(seed=int(rng[0]), offset=int(rng[1]))
    return (float(p), rng, _ptr(rng_state_out))


def _float_attention_operands(m, n, d, column_indices, q_stride, k_stride, v_stride, out_stride,
                              lse_stride, nonzeros):
    """The defaults of the float32 attention forms: replicas follow each other (q and out
    m * d, k and v n * d, lse m elements apart) and every entry of column_indices is meant."""
    return (column_indices.numel() if nonzeros is None else int(nonzeros), _stride(q_stride, m * d),
            _stride(k_stride, n * d), _stride(v_stride, n * d), _stride(out_stride, m * d),
            _stride(lse_stride, m))


def sparse_attention_forward(m, n, d, replicas, row_indices, row_offsets, column_indices, q, k, v,
                             scale, out, lse=None, workspace=None, *, q_stride=None, k_stride=None,
                             v_stride=None, out_stride=None, lse_stride=None, nonzeros=None, p=0.0,
                             rng=None, rng_state_out=None):
    """Fused softmax(scale * q k^T at the mask) v.  q [R,m,d], k and v [R,n,d].  Replica r of an
    operand begins r * its stride elements into the tensor (default: the replicas follow each
    other); `rng` or `rng_state_out` select the `_dropout` form (p = 0: nothing is dropped)."""
    nonzeros, qs, ks, vs, os_, ls = _float_attention_operands(
        m, n, d, column_indices, q_stride, k_stride, v_stride, out_stride, lse_stride, nonzeros)
    for t, dt, nm in ((row_indices, torch.int32, "row_indices"),
                      (row_offsets, torch.int32, "row_offsets"),
                      (column_indices, torch.int32, "column_indices"), (q, torch.float32, "q"),
                      (k, torch.float32, "k"), (v, torch.float32, "v"),
                      (out, torch.float32, "out")):
        _require(t, dt, nm)
    drop = _drop(p, rng, rng_state_out)
    name = "sputnik_hip_sparse_attention_forward" + ("_dropout" if drop else "")
    _check(getattr(lib(), name)(
        m, n, d, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(q), qs, _ptr(k), ks, _ptr(v), vs, float(scale), _ptr(out), os_, _ptr(lse), ls, *drop,
        _ptr(workspace), _ws_bytes(workspace), _stream(out)), name)
    return out


def sparse_attention_rows_supported(m, n, d, nonzeros):
    return bool(lib().sputnik_hip_sparse_attention_rows_supported(m, n, d, nonzeros))


def sparse_attention_rows_forward(m, n, d, replicas, row_indices, row_offsets, column_indices, q, k,
                                  v, scale, out, lse=None, *, q_stride=None, k_stride=None,
                                  v_stride=None, out_stride=None, lse_stride=None, nonzeros=None,
                                  p=0.0, rng=None, rng_state_out=None):
    """The row-group forward (d = 128): sparse_attention_forward's arguments without a
    workspace.  Returns the library's status."""
    nonzeros, qs, ks, vs, os_, ls = _float_attention_operands(
        m, n, d, column_indices, q_stride, k_stride, v_stride, out_stride, lse_stride, nonzeros)
    drop = _drop(p, rng, rng_state_out) or (0.0, PhiloxState(), None)
    return lib().sputnik_hip_sparse_attention_rows_forward(
        m, n, d, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(q), qs, _ptr(k), ks, _ptr(v), vs, float(scale), _ptr(out), os_, _ptr(lse), ls, *drop,
        _stream(out))


def sparse_attention_backward_supported(m, n, d, nonzeros):
    return bool(lib().sputnik_hip_sparse_attention_backward_supported(m, n, d, nonzeros))


def sparse_attention_backward_workspace_bytes(m, n, d, nonzeros, replicas):
    return lib().sputnik_hip_sparse_attention_backward_workspace_bytes(m, n, d, nonzeros, replicas)


def sparse_attention_backward(m, n, d, replicas, row_indices, row_offsets, column_indices,
                              t_row_indices, t_row_offsets, t_column_indices, permutation, q, k, v,
                              scale, out, grad_out, lse, grad_q, grad_k, grad_v, workspace, *,
                              q_stride=None, k_stride=None, v_stride=None, out_stride=None,
                              grad_out_stride=None, lse_stride=None, grad_q_stride=None,
                              grad_k_stride=None, grad_v_stride=None, nonzeros=None, p=0.0, rng=None):
    """sputnik_hip_sparse_attention_backward: any of grad_q, grad_k, grad_v may be None; one
    stride per operand as in sparse_attention_forward.  `rng` replays the forward's dropout:
    a PhiloxState (values, or seed_ptr / offset_ptr into a published rng_state_out) or
    (seed, offset).  Returns the library's status."""
    nonzeros, qs, ks, vs, os_, ls = _float_attention_operands(
        m, n, d, column_indices, q_stride, k_stride, v_stride, out_stride, lse_stride, nonzeros)
    drop = _drop(p, rng, None) or (0.0, PhiloxState())
    first = next(t for t in (grad_q, grad_k, grad_v, q) if t is not None)
    return lib().sputnik_hip_sparse_attention_backward(
        m, n, d, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(t_row_indices), _ptr(t_row_offsets), _ptr(t_column_indices), _ptr(permutation),
        _ptr(q), qs, _ptr(k), ks, _ptr(v), vs, float(scale), _ptr(out), os_, _ptr(grad_out),
        _stride(grad_out_stride, m * d), _ptr(lse), ls, _ptr(grad_q), _stride(grad_q_stride, m * d),
        _ptr(grad_k), _stride(grad_k_stride, n * d), _ptr(grad_v), _stride(grad_v_stride, n * d),
        drop[0], drop[1], _ptr(workspace), _ws_bytes(workspace), _stream(first))


def _head_view(t):
    """(pointer, batch, head, row strides) of a [B, H, rows, d] view with a unit last stride."""
    if not (t.is_cuda and t.dim() == 4 and t.stride(3) == 1):
        raise ValueError("expected a [B, H, rows, d] GPU view with a unit last stride")
    return [_ptr(t), t.stride(0), t.stride(1), t.stride(2)]


def sparse_attention_heads_supported(m, n, d, nonzeros, q, k, v, out):
    """Whether the half-storage fused kernel serves these [B, H, rows, d] views."""
    views = _head_view(q) + _head_view(k) + _head_view(v) + _head_view(out)
    return bool(lib().sputnik_hip_sparse_attention_heads_supported(
        m, n, d, nonzeros, q.size(0), q.size(1), TYPE_CODES[q.dtype], TYPE_CODES[out.dtype], *views))


def sparse_attention_heads_workspace_bytes(m, n, d, nonzeros):
    return lib().sputnik_hip_sparse_attention_heads_workspace_bytes(m, n, d, nonzeros)


def sparse_attention_heads_forward(m, n, d, row_indices, row_offsets, column_indices, q, k, v, scale, out,
                                   lse=None, workspace=None, planned=False, *, lse_stride=None,
                                   nonzeros=None, p=0.0, rng=None, rng_state_out=None):
    """Fused attention on float16 / bfloat16 head views q [B,H,m,d], k and v [B,H,n,d] into the
    view `out` (float32 or the operands' type); lse [B*H, lse_stride] float32 or None.
    `planned`: the workspace holds sputnik_hip_sparse_attention_plan's pre-pass; `rng` or
    `rng_state_out`: the `_dropout` form."""
    drop = _drop(p, rng, rng_state_out)
    name = ("sputnik_hip_sparse_attention_heads_forward" + ("_planned" if planned else "")
            + ("_dropout" if drop else ""))
    _check(getattr(lib(), name)(
        m, n, d, column_indices.numel() if nonzeros is None else int(nonzeros), q.size(0), q.size(1),
        _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices), TYPE_CODES[q.dtype], *_head_view(q),
        *_head_view(k), *_head_view(v), float(scale), _ptr(out), TYPE_CODES[out.dtype],
        *_head_view(out)[1:], _ptr(lse), _stride(lse_stride, m), *drop, _ptr(workspace),
        _ws_bytes(workspace), _stream(out)), name)
    return out


# ---- the fused attention with one mask per batch element: these return the library's status
# (0, SPUTNIK_HIP_UNSUPPORTED = -2, SPUTNIK_HIP_INVALID_ARGUMENT) instead of raising ----
def sparse_attention_many_mask_workspace_bytes(masks, m, n, d, largest_nonzeros):
    return lib().sputnik_hip_sparse_attention_many_mask_workspace_bytes(masks, m, n, d, largest_nonzeros)


def sparse_attention_many_mask_plan(masks, m, n, d, nonzeros, row_indices, row_offsets, column_indices,
                                    workspace):
    arr, _ = _host_counts(nonzeros)
    return lib().sputnik_hip_sparse_attention_many_mask_plan(
        masks, m, n, d, arr, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices), _ptr(workspace),
        _ws_bytes(workspace), _stream(row_offsets))


def sparse_attention_many_mask_forward(masks, m, n, d, nonzeros, replicas, row_indices, row_offsets,
                                       column_indices, q, k, v, scale, out, lse=None, workspace=None,
                                       planned=False, *, q_stride=None, k_stride=None, v_stride=None,
                                       out_stride=None, lse_stride=None, p=0.0, rng=None,
                                       rng_state_out=None):
    """q [R,m,d], k and v [R,n,d] float32, replica r under mask r // (R // masks); lse
    [R, lse_stride] or None; one stride per operand as in sparse_attention_forward.  `planned`:
    the workspace holds the plan of sparse_attention_many_mask_plan; `rng` or `rng_state_out`:
    the `_dropout` form."""
    arr, _ = _host_counts(nonzeros)
    _, qs, ks, vs, os_, ls = _float_attention_operands(
        m, n, d, column_indices, q_stride, k_stride, v_stride, out_stride, lse_stride, 0)
    drop = _drop(p, rng, rng_state_out)
    name = ("sputnik_hip_sparse_attention_many_mask_forward" + ("_planned" if planned else "")
            + ("_dropout" if drop else ""))
    return getattr(lib(), name)(
        masks, m, n, d, arr, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(q), qs, _ptr(k), ks, _ptr(v), vs, float(scale), _ptr(out), os_, _ptr(lse), ls, *drop,
        _ptr(workspace), _ws_bytes(workspace), _stream(out))


def sparse_attention_heads_many_mask_forward(masks, m, n, d, nonzeros, row_indices, row_offsets,
                                             column_indices, q, k, v, scale, out, lse=None,
                                             workspace=None, planned=False, *, lse_stride=None,
                                             p=0.0, rng=None, rng_state_out=None):
    """Half head views q [B,H,m,d], k and v [B,H,n,d], batch element b under mask b, into the view
    `out` (float32 or the operands' type); lse [B*H, lse_stride] float32 or None.  `rng` or
    `rng_state_out`: the `_dropout` form."""
    arr, _ = _host_counts(nonzeros)
    drop = _drop(p, rng, rng_state_out)
    name = ("sputnik_hip_sparse_attention_heads_many_mask_forward" + ("_planned" if planned else "")
            + ("_dropout" if drop else ""))
    return getattr(lib(), name)(
        masks, m, n, d, arr, q.size(0), q.size(1), _ptr(row_indices), _ptr(row_offsets),
        _ptr(column_indices), TYPE_CODES[q.dtype], *_head_view(q), *_head_view(k), *_head_view(v),
        float(scale), _ptr(out), TYPE_CODES[out.dtype], *_head_view(out)[1:], _ptr(lse),
        _stride(lse_stride, m), *drop, _ptr(workspace), _ws_bytes(workspace), _stream(out))


def sparse_linear_half_rows_forward(out_features, image, values_dtype, x, y):
    """y[b][s][o] = sum_i x[b][s][i] W[o][i] from W's image (sputnik_hip_sparse_linear_half_image),
    x [B, S, in] half, y a [B, S, out] view (float32 or x's type), both with unit last strides."""
    _check(lib().sputnik_hip_sparse_linear_half_rows_forward(
        out_features, x.size(2), x.size(1), x.size(0), _ptr(image), TYPE_CODES[values_dtype], _ptr(x),
        x.stride(0), x.stride(1), TYPE_CODES[x.dtype], _ptr(y), TYPE_CODES[y.dtype], y.stride(0), y.stride(1),
        _stream(x)), "sputnik_hip_sparse_linear_half_rows_forward")
    return y


def sddmm_plan(m, k, n, row_indices, row_offsets, column_indices, workspace):
    """Topology-only pre-pass of the tiled SDDMM kernels into `workspace`."""
    _check(lib().sputnik_hip_sddmm_plan(m, k, n, column_indices.numel(), _ptr(row_indices),
                                        _ptr(row_offsets), _ptr(column_indices), _ptr(workspace),
                                        _ws_bytes(workspace), _stream(row_offsets)),
           "sputnik_hip_sddmm_plan")
    return workspace


def sddmm_batched_planned(m, k, n, replicas, row_indices, row_offsets, column_indices, lhs, rhs,
                          out, workspace):
    nonzeros = column_indices.numel()
    _check(lib().sputnik_hip_sddmm_batched_planned(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(lhs), m * k, _ptr(rhs), n * k, _ptr(out), nonzeros, _ptr(workspace),
        _ws_bytes(workspace), _stream(out)), "sputnik_hip_sddmm_batched_planned")
    return out


def spmm_permuted_batched(m, k, n, replicas, row_indices, values, values_stride, permutation,
                          row_offsets, column_indices, dense, out):
    """out = A @ dense with A's values taken as values[permutation[p]]; returns the
    status (SPUTNIK_HIP_UNSUPPORTED = -2 when the shape is not served)."""
    nonzeros = column_indices.numel()
    st = lib().sputnik_hip_spmm_permuted_batched(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(values), values_stride,
        _ptr(permutation), _ptr(row_offsets), _ptr(column_indices), _ptr(dense), k * n, _ptr(out),
        m * n, _stream(out))
    if st != -2:
        _check(st, "sputnik_hip_spmm_permuted_batched")
    return st


class SpmmProblem(ctypes.Structure):
    """sputnik_hip_spmm_problem (include/sputnik_hip.h)."""
    _fields_ = [("row_indices", ctypes.c_void_p), ("row_offsets", ctypes.c_void_p),
                ("column_indices", ctypes.c_void_p), ("values", ctypes.c_void_p),
                ("value_permutation", ctypes.c_void_p), ("dense", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("nonzeros", ctypes.c_int)]


def spmm_group_batched(m, k, n, replicas, problems, block_rows=0, accumulate=False):
    """`problems`: list of dicts with row_indices (or None), row_offsets,
    column_indices, values, permutation (or None), dense, out.  Returns the status
    (SPUTNIK_HIP_UNSUPPORTED = -2 when the combination is not served)."""
    array = (SpmmProblem * len(problems))()
    for slot, p in zip(array, problems):
        slot.row_indices = _ptr(p.get("row_indices"))
        slot.row_offsets = _ptr(p["row_offsets"])
        slot.column_indices = _ptr(p["column_indices"])
        slot.values = _ptr(p["values"])
        slot.value_permutation = _ptr(p.get("permutation"))
        slot.dense = _ptr(p["dense"])
        slot.out = _ptr(p["out"])
        slot.nonzeros = p["column_indices"].numel()
    st = lib().sputnik_hip_spmm_group_batched(
        m, k, n, replicas, len(problems), ctypes.cast(array, ctypes.c_void_p), k * n, m * n,
        block_rows, int(bool(accumulate)), _stream(problems[0]["out"]))
    if st != -2:
        _check(st, "sputnik_hip_spmm_group_batched")
    return st


class SddmmSumProblem(ctypes.Structure):
    """sputnik_hip_sddmm_sum_problem (include/sputnik_hip.h)."""
    _fields_ = [("row_indices", ctypes.c_void_p), ("row_offsets", ctypes.c_void_p),
                ("column_indices", ctypes.c_void_p), ("lhs", ctypes.c_void_p),
                ("rhs", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
                ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_size_t),
                ("nonzeros", ctypes.c_int)]


def sddmm_sum_group_planned(m, k, n, replicas, problems):
    """`problems`: list of dicts with row_indices, row_offsets, column_indices, lhs, rhs, out,
    workspace (planned: sddmm_sum_plan), scratch -- up to four summed SDDMMs of one shape,
    their partial vectors added by one launch."""
    array = (SddmmSumProblem * len(problems))()
    for slot, p in zip(array, problems):
        slot.row_indices = _ptr(p["row_indices"])
        slot.row_offsets = _ptr(p["row_offsets"])
        slot.column_indices = _ptr(p["column_indices"])
        slot.lhs = _ptr(p["lhs"])
        slot.rhs = _ptr(p["rhs"])
        slot.out = _ptr(p["out"])
        slot.workspace = _ptr(p["workspace"])
        slot.workspace_bytes = _ws_bytes(p["workspace"])
        slot.scratch = _ptr(p.get("scratch"))
        slot.scratch_bytes = _ws_bytes(p.get("scratch"))
        slot.nonzeros = p["column_indices"].numel()
    _check(lib().sputnik_hip_sddmm_sum_group_planned(
        m, k, n, replicas, len(problems), ctypes.cast(array, ctypes.c_void_p), m * k, n * k,
        _stream(problems[0]["out"])), "sputnik_hip_sddmm_sum_group_planned")


def sddmm_sum_workspace_bytes(m, k, n, nonzeros):
    return lib().sputnik_hip_sddmm_sum_workspace_bytes(m, k, n, nonzeros)


def sddmm_sum_plan(m, k, n, row_indices, row_offsets, column_indices, workspace):
    """Topology-only pre-pass of the SUMMED tiled SDDMM into `workspace`."""
    _check(lib().sputnik_hip_sddmm_sum_plan(m, k, n, column_indices.numel(), _ptr(row_indices),
                                            _ptr(row_offsets), _ptr(column_indices),
                                            _ptr(workspace), _ws_bytes(workspace),
                                            _stream(row_offsets)),
           "sputnik_hip_sddmm_sum_plan")
    return workspace


def sddmm_sum_scratch_bytes(m, k, n, nonzeros, replicas):
    return lib().sputnik_hip_sddmm_sum_scratch_bytes(m, k, n, nonzeros, replicas)


def sddmm_sum_batched(m, k, n, replicas, row_indices, row_offsets, column_indices, lhs, rhs, out,
                      workspace, scratch, planned=False):
    """out[nnz] = sum over the replicas of sddmm(lhs_r, rhs_r)."""
    nonzeros = column_indices.numel()
    fn = lib().sputnik_hip_sddmm_sum_batched_planned if planned else lib().sputnik_hip_sddmm_sum_batched
    _check(fn(m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets),
              _ptr(column_indices), _ptr(lhs), m * k, _ptr(rhs), n * k, _ptr(out), _ptr(workspace),
              _ws_bytes(workspace), _ptr(scratch), _ws_bytes(scratch), _stream(out)),
           "sputnik_hip_sddmm_sum_batched")
    return out


def sddmm_sum_typed(m, k, n, replicas, row_indices, row_offsets, column_indices, lhs, rhs, out,
                    workspace, scratch, planned=False):
    """sddmm_sum_batched on float32 / float16 / bfloat16 operands; out float32."""
    nonzeros = column_indices.numel()
    _require(out, torch.float32, "out")
    _check(lib().sputnik_hip_sddmm_sum_typed(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(lhs), m * k, _ptr(rhs), n * k, _type_code(lhs, rhs), _ptr(out), _ptr(workspace),
        _ws_bytes(workspace), int(bool(planned)), _ptr(scratch), _ws_bytes(scratch), _stream(out)),
        "sputnik_hip_sddmm_sum_typed")
    return out


def left_spmm_half_tiles_workspace_bytes(m, k, n, nonzeros, replicas, values, dense, tile_dtype):
    return lib().sputnik_hip_left_spmm_half_tiles_workspace_bytes(
        m, k, n, nonzeros, replicas, _type_code(values), _type_code(dense),
        TYPE_CODES[tile_dtype])


def left_spmm_half_tiles(m, k, n, replicas, row_offsets, column_indices, values, dense, tile_dtype, out,
                         workspace, bias=None, relu=False):
    """left_spmm on the matrix cores (values shared, dense [R, k, n], out [R, m, n] float32);
    raises (status -2) where the route does not serve the call."""
    _require(out, torch.float32, "out")
    _check(lib().sputnik_hip_left_spmm_half_tiles(
        m, k, n, column_indices.numel(), replicas, _ptr(row_offsets), _ptr(column_indices),
        _ptr(values), _type_code(values), _ptr(dense), _type_code(dense), k * n,
        TYPE_CODES[tile_dtype], _ptr(bias), int(bool(relu)), _ptr(out), m * n,
        _ptr(workspace), _ws_bytes(workspace), _stream(out)), "sputnik_hip_left_spmm_half_tiles")
    return out


def sddmm_sum_mixed_scratch_bytes(m, k, n, nonzeros, replicas, lhs, rhs):
    return lib().sputnik_hip_sddmm_sum_mixed_scratch_bytes(m, k, n, nonzeros, replicas,
                                                           _type_code(lhs), _type_code(rhs))


def sddmm_sum_mixed(m, k, n, replicas, row_indices, row_offsets, column_indices, lhs, rhs, out,
                    workspace, scratch, planned=False):
    """The summed SDDMM on a (float32, half) pair of operands: the float32 one enters the
    matrix-core product as half planes over its range (include/sputnik_hip.h).  Raises (status -2) where that
    route does not serve the shape."""
    nonzeros = column_indices.numel()
    _require(out, torch.float32, "out")
    _check(lib().sputnik_hip_sddmm_sum_mixed(
        m, k, n, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(lhs), _type_code(lhs), m * k, _ptr(rhs), _type_code(rhs), n * k, _ptr(out),
        _ptr(workspace), _ws_bytes(workspace), int(bool(planned)), _ptr(scratch), _ws_bytes(scratch),
        _stream(out)), "sputnik_hip_sddmm_sum_mixed")
    return out


def sparse_attention_plan(m, n, d, row_indices, row_offsets, column_indices, workspace):
    _check(lib().sputnik_hip_sparse_attention_plan(
        m, n, d, column_indices.numel(), _ptr(row_indices), _ptr(row_offsets),
        _ptr(column_indices), _ptr(workspace), _ws_bytes(workspace), _stream(row_offsets)),
        "sputnik_hip_sparse_attention_plan")
    return workspace


def sparse_attention_forward_planned(m, n, d, replicas, row_indices, row_offsets, column_indices,
                                     q, k, v, scale, out, lse, workspace, *, q_stride=None,
                                     k_stride=None, v_stride=None, out_stride=None, lse_stride=None,
                                     nonzeros=None, p=0.0, rng=None, rng_state_out=None):
    """sparse_attention_forward on a workspace that holds sparse_attention_plan's pre-pass (the
    same keywords)."""
    nonzeros, qs, ks, vs, os_, ls = _float_attention_operands(
        m, n, d, column_indices, q_stride, k_stride, v_stride, out_stride, lse_stride, nonzeros)
    drop = _drop(p, rng, rng_state_out)
    name = "sputnik_hip_sparse_attention_forward_planned" + ("_dropout" if drop else "")
    _check(getattr(lib(), name)(
        m, n, d, nonzeros, replicas, _ptr(row_indices), _ptr(row_offsets), _ptr(column_indices),
        _ptr(q), qs, _ptr(k), ks, _ptr(v), vs, float(scale), _ptr(out), os_, _ptr(lse), ls, *drop,
        _ptr(workspace), _ws_bytes(workspace), _stream(out)), name)
    return out


def transpose_batched(batches, rows, cols, inp, out):
    """out[b][c][r] = inp[b][r][c] for contiguous [batches, rows, cols] fp32."""
    _require(inp, torch.float32, "inp")
    _require(out, torch.float32, "out")
    _check(lib().sputnik_hip_transpose_batched(batches, rows, cols, _ptr(inp), rows * cols,
                                               _ptr(out), rows * cols, _stream(out)),
           "sputnik_hip_transpose_batched")
    return out
