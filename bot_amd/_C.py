"""ctypes binding of libbot_gnn.so (include/bot_gnn.h) — the only compute backend of bot_amd.

There is no CPU or pure-PyTorch fallback: if the shared library is missing the import fails, and
every wrapper refuses non-HIP tensors.  Tensors cross the boundary as raw device pointers plus
sizes/strides; launches go to torch's current HIP stream and are not synchronised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int32, c_int64, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOT_AMD_LIB") or os.path.join(_HERE, "lib", "libbot_gnn.so")  # override: A/B builds of the kernels
ABI_VERSION = 19

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build the gfx950 kernels first "
        "(`make -C bot_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`). "
        "bot_amd has no CPU / PyTorch fallback."
    )
_lib = ctypes.CDLL(LIB_PATH)

_P = c_void_p
_SIGS = {
    "bot_abi_version": (ctypes.c_int, []),
    "bot_last_error": (c_char_p, []),
    "bot_last_kernel": (c_char_p, []),
    "bot_debug_abort_trace": (ctypes.c_int, [c_char_p]),
    "bot_row_plan_default_chunk": (c_int32, [c_int64]),
    "bot_row_plan_size_host": (ctypes.c_int, [_P, c_int64, c_int32, _P, _P, _P]),
    "bot_row_plan_fill_host": (ctypes.c_int, [_P, c_int64, c_int32, _P, _P, _P]),
    "bot_degrees_i64": (ctypes.c_int, [_P, c_int64, _P, _P]),
    "bot_spmm_workspace_floats": (c_int64, [c_int64, c_int32, c_int32]),
    "bot_spmm_set_layout": (ctypes.c_int, [c_int32]),
    "bot_spmm_set_zero_skip": (ctypes.c_int, [c_int32]),
    "bot_spmm_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int64, _P, _P,
                                    c_int32, c_int32, _P, c_int64, c_int64, _P, c_int64, c_int64, _P, _P]),
    "bot_spmm_blocked_f32": (ctypes.c_int, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, c_int64, _P,
                                            c_int32, c_int32, _P, c_int64, _P, c_int64, _P]),
    "bot_spmm_dot_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int64, _P, _P,
                                        _P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, c_int64, _P, _P, _P, _P]),
    "bot_spmm_bcast_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P, c_int32,
                                          c_int32, _P, c_int64, c_int64, _P, _P]),
    "bot_spmm_bcast_halves_f16": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P, c_int32, c_int32, _P, _P,
                                                 c_int64, c_int64, c_int32, c_int32, _P, _P]),
    "bot_spmm_dot_bcast_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int64, _P,
                                              _P, _P, c_int64, c_int32, c_int32, _P, c_int64, _P, _P, _P]),
    "bot_sddmm_dot_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, c_int64, _P, c_int64, c_int64,
                                         c_int32, c_int32, _P, _P, c_int32, _P]),
    "bot_sddmm_dot_bcast_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int32,
                                               c_int32, _P, _P, _P]),
    "bot_sddmm_u_add_v_f32": (ctypes.c_int, [_P, _P, c_int64, _P, _P, c_int32, _P, _P]),
    "bot_gat_attn_fwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, _P, _P, _P, _P, c_float,
                                            c_int32, _P, _P, _P, c_float, c_uint64, _P, _P, _P]),
    "bot_gat_attn_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, _P, _P, _P, c_float, c_int32,
                                            _P, _P, _P, _P, _P, _P, _P, c_float, c_uint64, _P, _P]),
    "bot_gat_infer_workspace_floats": (c_int64, [c_int64, c_int32, c_int32]),
    "bot_gat_infer_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64,
                                         _P, c_int64, _P, c_int64, _P, _P, c_float, c_int32, c_int32, _P, c_int64, c_int64, _P, _P,
                                         c_int32, _P, c_int64, c_int64, _P, _P, _P]),
    "bot_segment_sum_f32": (ctypes.c_int, [_P, c_int64, c_int64, _P, c_int64, c_int32, _P, _P, c_int32, _P, _P]),
    "bot_gather_rows_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P]),
    "bot_scatter_add_rows_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P]),
    "bot_merge_weight_fwd_f32": (ctypes.c_int, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "bot_merge_weight_bwd_f32": (ctypes.c_int, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    "bot_edge_mlp_workspace_floats": (c_int64, []),
    "bot_edge_mlp_fwd_f32": (ctypes.c_int, [_P, c_int32, _P, _P, c_int32, _P, c_int32, c_int64, _P, _P]),
    "bot_edge_mlp_bwd_f32": (ctypes.c_int, [_P, c_int32, _P, _P, c_int32, _P, c_int32, _P, c_int64, _P, _P, _P, _P, _P]),
    "bot_random_keep_workspace_bytes": (c_int64, []),
    "bot_random_keep_u8": (ctypes.c_int, [c_int64, c_int64, c_uint64, _P, _P, _P]),
    "bot_halves_workspace_floats": (c_int64, []),
    "bot_halves_scale_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P, _P]),
    "bot_halves_split_f16": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, c_int32, _P, c_int64, c_int32, _P]),
    "bot_halves_split_cols_f16": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, c_int32, _P, c_int64, c_int32, c_int32, _P]),
    "bot_halves_split_heads_f16": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, c_int32, _P, _P, c_int64, c_int32, c_int32, _P]),
    "bot_gemm_halves_f32": (ctypes.c_int, [c_int32, c_int32, c_int64, c_int64, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64,
                                           c_int32, c_int64, c_int64, c_int64, c_float, _P, c_int64, c_int32, c_int32, _P]),
    "bot_gemm_halves3_nt_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, _P, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, _P, c_int64,
                                               c_int32, _P]),
    "bot_gemm_halves3_tn_workspace_floats": (c_int64, [c_int64, c_int64, c_int64]),
    "bot_gemm_halves3_tn_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, _P,
                                               c_int64, _P, c_int32, _P]),
    "bot_gemm_halves3_nt_grouped_f32": (ctypes.c_int, [c_int64, c_int64, _P, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, _P, c_int64, c_int32, _P,
                                                       c_int32, _P, _P, c_int32, _P, c_int32, _P]),
    "bot_gemm_halves3_tn_grouped_workspace_floats": (c_int64, [c_int64, c_int32]),
    "bot_gemm_halves3_tn_grouped_f32": (ctypes.c_int, [c_int64, _P, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, _P, c_int32, _P, _P, c_int32, _P]),
    "bot_tn_narrow_workspace_floats": (c_int64, [c_int64, c_int32, c_int32]),
    "bot_tn_narrow_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, c_int32, _P, _P]),
    "bot_bn_act_bwd_reduce_max_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_float, c_uint64, _P, _P, _P, _P, _P]),
    "bot_bn_bwd_bound_f32": (ctypes.c_int, [c_int32, c_int64, _P, _P, _P, c_double, _P, _P, _P, _P]),
    "bot_bn_act_bwd_apply_halves_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_float, c_uint64, _P, _P, _P, c_double,
                                                       _P, c_int64, _P, _P, c_int64, c_int32, c_int32, c_int32, _P]),
    "bot_label_split_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P, c_float, c_uint64, _P, c_int32, _P, _P, _P, _P, _P]),
    "bot_build_input_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_float, c_uint64, _P, _P, c_int64, _P]),
    "bot_build_input_reuse_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, c_int64, c_float, c_uint64, _P, _P, c_int64, _P]),
    "bot_node_loss_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, c_int64, _P, _P, c_int32, c_float, _P, c_int64, _P, c_int64, _P]),
    "bot_rmsprop_step_f32": (ctypes.c_int, [c_int32, _P, _P, _P, _P, c_float, _P, c_float, c_float, c_float, _P]),
    "bot_gemm_halves_last_algo": (ctypes.c_int, [_P, _P]),
    "bot_gemm_halves_library_version": (ctypes.c_int, [_P, _P]),
    "bot_tn_gemm_workspace_floats": (c_int64, [c_int64, c_int32, c_int32, c_int32]),
    "bot_tn_gemm_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, c_int32, c_int32, c_int64, c_int64,
                                       c_int64, _P, _P]),
    "bot_skinny_gemm_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int32, _P, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32,
                                           c_int64, c_int64, c_int64, _P]),
    "bot_bn_workspace_floats": (c_int64, [c_int32]),
    "bot_colstats_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P, _P, _P]),
    "bot_colsum_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P, _P]),
    "bot_bn_stats_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P, _P]),
    "bot_bn_stats_halves_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, c_float, _P, _P, _P]),
    "bot_bn_act_fwd_halves_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_float, c_uint64, _P, _P, c_int64,
                                                 _P, _P, c_int64, c_int32, c_int32, _P]),
    "bot_bn_act_fwd_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_float, c_uint64, _P, _P, c_int64, _P]),
    "bot_bn_act_bwd_reduce_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_float,
                                                 c_uint64, _P, _P, _P, _P, _P]),
    "bot_bn_act_bwd_apply_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_float,
                                                c_uint64, _P, _P, _P, c_double, _P, c_int64, _P, _P]),
    "bot_halves_tn_combine_f32": (ctypes.c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, c_int64, _P]),
    "bot_halves_scale_from_slots2_f32": (ctypes.c_int, [_P, c_float, _P, c_float, _P, _P]),
    "bot_halves_tail_f16": (ctypes.c_int, [c_int64, c_int32, _P, _P, _P, _P, _P, c_int64, c_int32, _P]),
    "bot_spmm_dot_halves_fits": (ctypes.c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, c_int64, c_int32]),
    "bot_spmm_dot_halves_f16": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int64, _P, _P, _P, c_int64, c_int64,
                                               c_int32, c_int32, _P, _P, c_int64, c_int64, c_int32, _P, _P, _P]),
    "bot_gemm_halves3_nt_bn_rows": (c_int32, [c_int64]),
    "bot_gemm_halves3_nt3_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, _P, c_int64,
                                                _P, c_int32, _P]),
    "bot_gemm_halves3_nt_bn_deferred_max_k": (c_int32, []),
    "bot_gemm_halves3_nt_bn_reduce_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, _P, c_int64,
                                                         _P, _P]),
    "bot_gemm_halves3_nt_bn_apply_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, _P,
                                                        _P, _P, c_double, _P, c_int64, _P, _P, c_int64, c_int32, c_int32, c_int32, _P, _P]),
    "bot_bn_act_bwd_reduce_partials_f32": (ctypes.c_int, [_P, c_int32, c_int32, _P, _P, _P]),
    "bot_bn_bwd_bound_partials_f32": (ctypes.c_int, [c_int32, _P, c_int32, _P, _P, c_double, _P, _P, _P, _P]),
    "bot_bn_bwd_partials_finish_f32": (ctypes.c_int, [_P, _P, c_int32, c_int32, _P, _P, c_int32, c_double, _P, _P, _P, _P]),
    "bot_gemm_halves3_nt2_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, _P, c_int64,
                                                c_int32, _P]),
    "bot_halves_split_frag_f16": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P, c_int32, _P]),
    "bot_gemm_halves3_tn2_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, c_int64, _P, c_int64, c_int64, _P, c_int64, c_int64, _P,
                                                c_int64, _P, c_int32, _P]),
    "bot_stream_create": (ctypes.c_int, [c_int32, _P]),
    "bot_gemm_halves3_nt_grouped2_f32": (ctypes.c_int, [c_int64, c_int64, _P, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, _P, c_int64, c_int32, _P,
                                                        c_int32, _P, _P, c_int32, _P, _P, _P, _P, c_int32, c_int32, _P]),
    "bot_bn_stats_halves_partials_f32": (ctypes.c_int, [_P, _P, c_int32, _P, c_int64, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, c_float, _P, _P, _P]),
    "bot_absmax_slots": (c_int32, []),
    "bot_absmax_slots_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, _P]),
    "bot_halves_scale_from_slots_f32": (ctypes.c_int, [_P, _P, _P]),
    "bot_sample_neighbors_count_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int32, _P, _P]),
    "bot_sample_neighbors_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int32, c_uint64, _P, _P, _P]),
    "bot_block_tiles": (c_int64, [c_int64]),
    "bot_block_mark_i32": (ctypes.c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "bot_block_relabel_i32": (ctypes.c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, _P]),
    "bot_subgraph_mark_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P, _P]),
    "bot_subgraph_count_i32": (ctypes.c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "bot_subgraph_fill_i32": (ctypes.c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P]),
    "bot_subgraph_unmark_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P]),
    "bot_subgraph_tally_i32": (ctypes.c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "bot_saint_walk_i32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, c_int32, c_uint64, _P, _P]),
    "bot_saint_nodes_mark_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P, _P, _P]),
    "bot_saint_nodes_list_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P, _P]),
    "bot_node_loss_weighted_f32": (ctypes.c_int, [_P, c_int64, c_int64, c_int32, _P, c_int64, _P, _P, _P, c_int32, c_float, _P, c_int64, _P, c_int64, _P]),
    "bot_rocauc_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "bot_rocauc_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, _P, _P, _P, c_int64, _P]),
    "bot_propagate_step_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                              c_float, c_float, _P, _P, c_float, c_float, _P, _P, _P, _P, _P]),
    "bot_propagate_step_w_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                                c_float, c_float, _P, _P, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "bot_appnp_step_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                          c_float, c_float, _P, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, c_float, c_uint64, c_int32, _P]),
    "bot_spmm_max_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int32, c_int32, _P, c_int64,
                                        _P, c_int64, _P, _P]),
    "bot_spmm_max_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int32, _P,
                                            c_int64, _P, _P]),
    "bot_spmm_pna_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, _P,
                                        c_int32, _P, c_int32, c_int32, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_pna_bwd_prep_f32": (ctypes.c_int, [_P, c_int64, _P, c_int64, _P, c_int32, _P, c_int32, c_int32, c_int32, _P, c_int64, _P, c_int64, _P, c_int64,
                                            _P, c_int64, _P]),
    "bot_spmm_pna_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int32, c_int32,
                                            _P, c_int64, _P, _P]),
    "bot_spmm_pna_edge_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32,
                                             _P, c_int32, _P, _P, _P, c_int32, _P, c_int32, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_pna_edge_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64, _P, c_int32, _P, _P, _P,
                                                 c_int64, _P, c_int32, c_int32, _P, c_int64, _P, _P, _P, c_int64, _P]),
    "bot_spmm_softmax_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, c_int32, c_float,
                                            _P, c_int64, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_softmax_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int32, c_float, _P, c_int64,
                                                _P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P, _P]),
    "bot_spmm_softmax_edge_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, c_int32, _P,
                                                 _P, _P, _P, c_int32, c_float, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_softmax_edge_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int32, _P, _P, _P, _P,
                                                     c_int32, c_float, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P, _P, _P,
                                                     c_int64, _P]),
    "bot_gatv2_logits_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int32, c_int32, c_float, _P, _P,
                                            c_int64, _P]),
    "bot_gatv2_logits_bwd_dst_workspace_floats": (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    "bot_gatv2_logits_bwd_dst_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P,
                                                    c_int32, c_int32, c_float, _P, c_int64, _P, _P, c_int64, _P, _P, _P]),
    "bot_gatv2_logits_bwd_src_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P,
                                                    c_int32, c_int32, c_float, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_gate_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                         c_int32, c_float, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_gate_bwd_dst_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P,
                                                 c_int64, _P, c_int64, c_int32, _P, c_int64, _P, _P]),
    "bot_spmm_gate_bwd_src_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64,
                                                 _P, c_int64, _P, c_int64, c_int32, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_gate_edge_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P,
                                              c_int64, c_int32, c_int32, c_float, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, _P, _P]),
    "bot_spmm_gate_edge_bwd_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P,
                                                  c_int64, _P, c_int64, c_int32, _P, c_int64, _P, c_int64, c_int32, _P, _P]),
    "bot_spmm_gate_edge_bwd_src_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, _P, c_int64, _P, c_int64, _P,
                                                      c_int64, c_int32, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_spmm_rel_expand_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, _P, _P, c_int32, c_int32, _P, c_int64,
                                               c_int32, _P, c_int64, _P, _P]),
    "bot_spmm_rel_contract_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, _P, _P, c_int32, c_int32, _P, c_int64,
                                                 c_int32, _P, c_int64, _P, _P]),
    "bot_dot_attn_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                        c_int32, c_float, _P, c_float, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_dot_attn_bwd_dst_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32,
                                                c_int32, c_float, _P, c_float, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, c_int64, _P, _P]),
    "bot_dot_attn_bwd_src_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P,
                                                c_int32, c_int32, c_float, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_dot_attn_edge_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P,
                                             c_int64, _P, c_int64, c_int32, c_int32, c_int32, c_float, _P, c_float, _P, c_int64, _P, c_int64, _P, c_int64,
                                             _P, _P]),
    "bot_dot_attn_edge_bwd_dst_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P,
                                                     c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, c_int32, c_float, _P, c_float, _P, c_int64,
                                                     _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, _P]),
    "bot_sample_weights_prepare_f32": (ctypes.c_int, [_P, _P, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "bot_sample_neighbors_weighted_count_i32": (ctypes.c_int, [_P, c_int64, _P, c_int64, c_int32, _P, _P]),
    "bot_sample_neighbors_weighted_i32": (ctypes.c_int, [_P, _P, _P, c_int64, _P, c_int64, c_int32, c_uint64, _P, _P, _P]),
    "bot_row_plan_device_workspace_bytes": (c_int64, [c_int64]),
    "bot_row_plan_size_device": (ctypes.c_int, [_P, c_int64, c_int32, _P, c_int64, _P, _P]),
    "bot_row_plan_fill_device": (ctypes.c_int, [_P, c_int64, c_int32, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P]),
    "bot_csc_transpose_workspace_bytes": (c_int64, [c_int64]),
    "bot_csc_transpose_i32": (ctypes.c_int, [_P, _P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, c_int64, _P]),
}
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(_lib, _name)  # AttributeError here = header and library disagree
    _fn.restype, _fn.argtypes = _res, _args
EXPORTED = tuple(_SIGS)

if _lib.bot_abi_version() != ABI_VERSION:
    raise ImportError(f"libbot_gnn.so ABI {_lib.bot_abi_version()} != binding ABI {ABI_VERSION}; rebuild")


class BotKernelError(RuntimeError):
    pass


# bench.py sets this to a list to time individual launches with HIP events recorded on the launch stream
# (torch's current stream); entries are (kernel family, shape key, start event, end event).
PROFILE = None


PROFILE_SKIP = ()   # kernel families not to time while PROFILE is a list


def _timed(name, key, launch):
    if PROFILE is None or name in PROFILE_SKIP:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = launch()
    e1.record()
    PROFILE.append((name, key, e0, e1, _lib.bot_last_kernel().decode()))
    return rc


def _check(rc: int, what: str):
    if rc != 0:
        raise BotKernelError(f"{what} failed (rc={rc}): {_lib.bot_last_error().decode()}")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    """Row pitch of a row-major matrix view; torch leaves the stride of a size-1 dimension arbitrary, so a one-row matrix reports
    its width."""
    return max(int(t.stride(-2)), int(t.shape[-1])) if t.shape[-2] == 1 else int(t.stride(-2))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise BotKernelError(
                "bot_amd kernels run on MI355X only: got a CPU tensor and there is no CPU fallback "
                "(move the graph and features to the GPU)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise BotKernelError(f"operands live on different devices ({dev} and {t.device}): graph structures and features "
                                 "must be on the same GPU")


def _f32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise BotKernelError(f"{name} must be float32, got {t.dtype}")
    return t


def _i32(t, name):
    if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
        raise BotKernelError(f"{name} must be contiguous int32")
    return t


# ------------------------------------------------------------------------------------------------ host plan
def default_chunk(nnz: int) -> int:
    return int(_lib.bot_row_plan_default_chunk(int(nnz)))


def row_plan(indptr_cpu: torch.Tensor, chunk: int):
    """Host-side work plan for one compressed direction (include/bot_gnn.h "Row plan").

    indptr_cpu: CPU int32 [n_rows+1].  Returns CPU int32 tensors (items [n_items,4], long_rows, long_ptr)."""
    assert indptr_cpu.device.type == "cpu" and indptr_cpu.dtype == torch.int32 and indptr_cpu.is_contiguous()
    PLAN_COUNTS["host_plan"] += 1
    n_rows = indptr_cpu.numel() - 1
    if n_rows == 0:     # a direction without rows (the halo rows of a 1-rank partition): an empty plan
        return torch.empty((0, 4), dtype=torch.int32), torch.empty((0,), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32), 0
    n_items, n_long, n_slots = c_int64(), c_int64(), c_int64()
    _check(_lib.bot_row_plan_size_host(indptr_cpu.data_ptr(), n_rows, chunk, ctypes.addressof(n_items),
                                       ctypes.addressof(n_long), ctypes.addressof(n_slots)), "row_plan_size")
    items = torch.empty((n_items.value, 4), dtype=torch.int32)
    long_rows = torch.empty((n_long.value,), dtype=torch.int32)
    long_ptr = torch.empty((n_long.value + 1,), dtype=torch.int32)
    _check(_lib.bot_row_plan_fill_host(indptr_cpu.data_ptr(), n_rows, chunk, items.data_ptr(), _ptr(long_rows) if n_long.value else None,
                                       long_ptr.data_ptr()), "row_plan_fill")
    return items, long_rows, long_ptr, int(n_slots.value)


# ------------------------------------------------------------------------------------------------ device plan / transpose
# calls of row_plan_device / csc_transpose that ran on the device, and of row_plan (the host planner, the fallback included): what tells
# the device path of a mini-batch graph from the host path
PLAN_COUNTS = {"device_plan": 0, "device_transpose": 0, "host_plan": 0}
DEVICE_PLAN_MAX_CHUNK = 1024   # csrc/plan.hip kPlanMaxChunk


def _ws_bytes(n, dev):
    return torch.empty(max(int(n), 8) // 8 + 1, dtype=torch.int64, device=dev)


def row_plan_device(indptr: torch.Tensor, chunk: int):
    """`row_plan` for a DEVICE indptr (int32 [n_rows + 1]) on the device (include/bot_gnn.h bot_row_plan_*_device): the same arrays bit for
    bit, as device tensors - (items [n_items, 4], long_rows [n_long], long_ptr [n_long + 1], n_slots), n_items and n_long being the
    tensors' sizes.  One device->host read (three int64: n_long, n_slots and the count of rows with a negative degree, which raises
    BotKernelError as the host planner's BOT_E_PLAN does).  A chunk above DEVICE_PLAN_MAX_CHUNK goes to the host planner."""
    _dev(indptr)
    _i32(indptr, "indptr")
    dev, chunk = indptr.device, int(chunk)
    n_rows = int(indptr.numel()) - 1
    if chunk > DEVICE_PLAN_MAX_CHUNK:
        items, long_rows, long_ptr, n_slots = row_plan(indptr.cpu().contiguous(), chunk)
        return items.to(dev), long_rows.to(dev), long_ptr.to(dev), n_slots
    if n_rows <= 0:
        return (torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev),
                torch.zeros((1,), dtype=torch.int32, device=dev), 0)
    size = int(_lib.bot_row_plan_device_workspace_bytes(n_rows))
    ws = _ws_bytes(size, dev)
    sizes = torch.empty(3, dtype=torch.int64, device=dev)
    st = _stream()
    _check(_timed("row_plan_device", ("size",), lambda: _lib.bot_row_plan_size_device(
        indptr.data_ptr(), n_rows, chunk, ws.data_ptr(), ws.numel() * 8, sizes.data_ptr(), st)), "row_plan_size_device")
    n_long, n_slots, n_bad = (int(v) for v in sizes.tolist())       # the one device->host read
    if n_bad:
        raise BotKernelError(f"row_plan_device failed (rc=-4): row plan: indptr not monotone at {n_bad} of {n_rows} rows")
    n_items = n_rows - n_long + n_slots
    items = torch.empty((n_items, 4), dtype=torch.int32, device=dev)
    long_rows = torch.empty((n_long,), dtype=torch.int32, device=dev)
    long_ptr = torch.empty((n_long + 1,), dtype=torch.int32, device=dev)
    _check(_timed("row_plan_device", ("fill",), lambda: _lib.bot_row_plan_fill_device(
        indptr.data_ptr(), n_rows, chunk, ws.data_ptr(), ws.numel() * 8, n_items, n_long, n_slots, items.data_ptr(),
        _ptr(long_rows) if n_long else None, long_ptr.data_ptr(), st)), "row_plan_fill_device")
    PLAN_COUNTS["device_plan"] += 1
    return items, long_rows, long_ptr, n_slots


def csc_transpose(indptr: torch.Tensor, indices: torch.Tensor, n_src: int):
    """The CSR direction of a finished device CSC (include/bot_gnn.h bot_csc_transpose_i32): (indptr_r int32 [n_src + 1], indices_r int32 [E]
    = the destination row of each entry, eid_r int32 [E] = its CSC position), as `graph.build_direction` compresses the same edges by source.
    One device->host read (the count of indices outside [0, n_src), which raises BotKernelError)."""
    _dev(indptr, indices)
    _i32(indptr, "indptr"), _i32(indices, "indices")
    dev = indptr.device
    n_dst, E, n_src = int(indptr.numel()) - 1, int(indices.numel()), int(n_src)
    size = int(_lib.bot_csc_transpose_workspace_bytes(E))
    ws = _ws_bytes(size, dev) if E > 0 and size > 0 else None
    indptr_r = (torch.empty if E else torch.zeros)(max(n_src, 0) + 1, dtype=torch.int32, device=dev)   # E == 0: nothing is launched
    indices_r = torch.empty(E, dtype=torch.int32, device=dev)
    eid_r = torch.empty(E, dtype=torch.int32, device=dev)
    n_bad = torch.empty(1, dtype=torch.int64, device=dev)
    _check(_timed("csc_transpose", (), lambda: _lib.bot_csc_transpose_i32(
        indptr.data_ptr(), _ptr(indices) if E else None, n_dst, n_src, E, indptr_r.data_ptr(), _ptr(indices_r) if E else None,
        _ptr(eid_r) if E else None, n_bad.data_ptr(), _ptr(ws), 0 if ws is None else ws.numel() * 8, _stream())), "csc_transpose")
    bad = int(n_bad) if E else 0                                    # the one device->host read
    if bad:
        raise BotKernelError(f"csc_transpose: {bad} of the {E} indices lie outside [0, {n_src})")
    PLAN_COUNTS["device_transpose"] += 1
    return indptr_r, indices_r, eid_r


# ------------------------------------------------------------------------------------------------ kernels
# `d` is a bot_amd.graph.Direction: indptr/indices (int32, device), items/long_rows/long_ptr, sizes.

def degrees(d) -> torch.Tensor:
    _dev(d.indptr)
    out = torch.empty(d.n_rows, dtype=torch.int64, device=d.indptr.device)
    _check(_lib.bot_degrees_i64(d.indptr.data_ptr(), d.n_rows, out.data_ptr(), _stream()), "degrees")
    return out


def _slab(x, name):
    """[n,H,D] float32 view with unit inner stride -> (tensor, ld, hs)."""
    _f32(x, name)
    if x.dim() != 3:
        raise BotKernelError(f"{name} must be [n,H,D]")
    if x.stride(2) != 1 and x.shape[2] != 1:
        x = x.contiguous()
    if x.shape[1] == 1:
        return x, x.stride(0), max(x.shape[2], 1)
    return x, x.stride(0), x.stride(1)


def spmm_blocked(bp, x, w, out, addend=None):
    """L2-blocked SpMM over the tiles of `bp` (bot_amd.blocked.BlockedPlan); writes only the rows bp covers.  x / out /
    addend: [n,H,D] with contiguous rows (any row stride)."""
    H, D = x.shape[1], x.shape[2]
    _check(_timed("spmm_blocked", (H, D, w is not None), lambda: _lib.bot_spmm_blocked_f32(
        bp.tile_rows.data_ptr(), bp.ptr.data_ptr(), bp.b_src.data_ptr(), bp.b_lrow.data_ptr(), bp.b_pos.data_ptr(), bp.n_tiles,
        bp.nblk, bp.block_rows, bp.T, bp.epi, bp.round_tiles, x.data_ptr(), x.stride(0), _ptr(w), H, D, out.data_ptr(), out.stride(0),
        _ptr(addend), addend.stride(0) if addend is not None else 0, _stream())),
        "spmm_blocked")
    return out


def _rows_contiguous(t):
    """[n,H,D] whose rows are H*D contiguous floats (row stride free)."""
    return t.stride(2) == 1 and (t.shape[1] == 1 or t.stride(1) == t.shape[2])


SPMM_LAYOUT = None   # None: per direction (flat 16-byte lanes when its plan is in XCD order = the numbering has locality); "flat" / "rows": force


def spmm_set_zero_skip(on):
    """Process-wide: do the weighted sweeps (spmm with w, spmm_dot, spmm_dot_halves) skip the neighbour rows whose weight is exactly 0
    (include/bot_gnn.h bot_spmm_set_zero_skip)?  Default on; off gives the same finite results and reads every row."""
    _check(_lib.bot_spmm_set_zero_skip(int(on)), "spmm_set_zero_skip")


def spmm(d, x, w=None, wperm=None, out=None, addend=None):
    """out[r,h,:] = sum_k w[wperm[k],h] * x[indices[k],h,:] (+ addend[r,h,:])   (w None: plain sum).  x: [n_src,H,D]."""
    _dev(x, w, d.indptr)
    x, ldx, hsx = _slab(x, "x")
    if wperm is None and out is None and _rows_contiguous(x) and (
            addend is None or (addend.dim() == 3 and addend.dtype == torch.float32 and _rows_contiguous(addend))):
        from . import blocked
        bp = blocked.plan_for(d, x.shape[0], x.shape[1], x.shape[2])
        if bp is not None:
            # the plan's LDS layout assumes the vector width blocked.layout() derives from D alone; the C side re-derives it
            # from the operands' alignment too — a slab whose base or row stride is not a multiple of it takes the row kernel
            vec = blocked.layout(x.shape[1], x.shape[2])[0]
            ok = lambda t: t is None or (t.data_ptr() % (4 * vec) == 0 and t.stride(0) % vec == 0)
            if not (ok(x) and ok(addend)):
                bp = None
        if bp is not None:  # dense graph: L2-blocked sweep for the regular rows, row-per-group kernel for the hubs
            if w is not None:
                w = _f32(w, "w").contiguous()
            out = torch.empty((d.n_rows, x.shape[1], x.shape[2]), dtype=torch.float32, device=x.device)
            spmm_blocked(bp, x, w, out, addend)
            if bp.heavy is not None:
                spmm(bp.heavy, x, w, None, out=out, addend=addend)
            return out
    lda = hsa = 0
    if addend is not None:
        addend, lda, hsa = _slab(addend, "addend")
    H, D = x.shape[1], x.shape[2]
    if w is not None:
        _f32(w, "w")
        w = w.contiguous()
        if w.dim() != 2 or w.shape[1] != H:
            raise BotKernelError(f"w must be [nnz,{H}], got {tuple(w.shape)}")
    if out is None:
        out = torch.empty((d.n_rows, H, D), dtype=torch.float32, device=x.device)
    out_, ldo, hso = _slab(out, "out")
    assert out_ is out
    partial = None
    if d.n_long:
        partial = torch.empty(int(_lib.bot_spmm_workspace_floats(d.n_slots, H, D)), dtype=torch.float32, device=x.device)
    flat = SPMM_LAYOUT == "flat" or (SPMM_LAYOUT is None and getattr(d, "plan_order", "degree") == "xcd")
    _lib.bot_spmm_set_layout(1 if flat else 0)     # thread-local hint; identical results either way (include/bot_gnn.h)
    _check(_timed("spmm", (H, D, w is not None), lambda: _lib.bot_spmm_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, x.data_ptr(), ldx, hsx, _ptr(w), _ptr(_i32(wperm, "wperm")), H, D, out.data_ptr(), ldo, hso,
        _ptr(addend), lda, hsa, _ptr(partial), _stream())), "spmm")
    return out


def spmm_dot_max_d(x):
    """Largest D the fused spmm_dot launch covers for this slab's alignment."""
    return 1024 if (x.shape[2] % 4 == 0 and x.stride(0) % 4 == 0) else (512 if x.shape[2] % 2 == 0 and x.stride(0) % 2 == 0 else 256)


def spmm_dot(d, x, w, wperm, y, out=None, dot=None, absmax=None):
    """Fused backward of u_mul_e_sum on direction `d`:  out[r,h,:] = sum_k w[wperm[k],h] x[indices[k],h,:]  and
    dot[wperm[k],h] = <y[r,h,:], x[indices[k],h,:]>.  Returns (out [n_rows,H,D], dot [nnz,H]).
    `dot`: write into this [E,H] array instead of a fresh one — `d` may be a PART of a larger direction (Graph.halo_split) whose
    entries are reached through `wperm`; the parts of one direction fill disjoint rows of the same array.
    `absmax`: `absmax_slots()` words that receive max|out| as a by-product (include/bot_gnn.h "Maxima as by-products")."""
    _dev(x, w, y, d.indptr)
    x, ldx, hsx = _slab(x, "x")
    y, ldy, hsy = _slab(y, "y")
    H, D = x.shape[1], x.shape[2]
    w = _f32(w, "w").contiguous()
    if out is None:
        out = torch.empty((d.n_rows, H, D), dtype=torch.float32, device=x.device)
    out_, ldo, hso = _slab(out, "out")
    assert out_ is out
    if dot is None:
        dot = torch.empty((d.nnz, H), dtype=torch.float32, device=x.device)
    elif dot.dtype != torch.float32 or not dot.is_contiguous() or dot.dim() != 2 or dot.shape[1] != H:
        raise BotKernelError(f"spmm_dot: dot must be a contiguous float32 [E,{H}] array")
    partial = None
    if d.n_long:
        partial = torch.empty(int(_lib.bot_spmm_workspace_floats(d.n_slots, H, D)), dtype=torch.float32, device=x.device)
    _check(_timed("spmm_dot", (H, D), lambda: _lib.bot_spmm_dot_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, x.data_ptr(), ldx, hsx, w.data_ptr(), _ptr(_i32(wperm, "wperm")), y.data_ptr(), ldy, hsy,
        H, D, out.data_ptr(), ldo, hso, dot.data_ptr(), _ptr(partial), _ptr(absmax), _stream())), "spmm_dot")
    return out, dot


def spmm_dot_halves_fits(x, y, hout, hsh, h2_off) -> bool:
    """Would `spmm_dot_halves` take these operands (x, y: [n, H, D] slabs; hout: the operand's [n, >= h2_off + H hsh] fp16 view)?"""
    x, ldx, hsx = _slab(x, "x")
    y, ldy, hsy = _slab(y, "y")
    return bool(_lib.bot_spmm_dot_halves_fits(x.data_ptr(), ldx, hsx, y.data_ptr(), ldy, hsy, x.shape[1], x.shape[2], hout.data_ptr(), hout.stride(0),
                                              int(hsh), int(h2_off)))


def spmm_dot_halves(d, x, w, wperm, y, hscale, hout, hsh, h2_off, dot=None):
    """`spmm_dot` whose first result leaves the kernel as a LEFT halves operand: hout[r, h * hsh + e] = h1, hout[r, h2_off + h * hsh + e] =
    2^11 h2 of hscale[0] * out[r,h,e] (bot_spmm_dot_halves_f16; all-heads layout only: ask spmm_dot_halves_fits first).  Returns dot [nnz, H]."""
    _dev(x, w, y, d.indptr, hout, hscale)
    x, ldx, hsx = _slab(x, "x")
    y, ldy, hsy = _slab(y, "y")
    H, D = x.shape[1], x.shape[2]
    w = _f32(w, "w").contiguous()
    assert hout.dtype == torch.float16 and hout.stride(1) == 1 and hout.shape[0] == d.n_rows
    if dot is None:
        dot = torch.empty((d.nnz, H), dtype=torch.float32, device=x.device)
    elif dot.dtype != torch.float32 or not dot.is_contiguous() or dot.dim() != 2 or dot.shape[1] != H:
        raise BotKernelError(f"spmm_dot_halves: dot must be a contiguous float32 [E,{H}] array")
    partial = None
    if d.n_long:
        partial = torch.empty(int(_lib.bot_spmm_workspace_floats(d.n_slots, H, D)), dtype=torch.float32, device=x.device)
    _check(_timed("spmm_dot", (H, D), lambda: _lib.bot_spmm_dot_halves_f16(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, x.data_ptr(), ldx, hsx, w.data_ptr(), _ptr(_i32(wperm, "wperm")), y.data_ptr(), ldy, hsy,
        H, D, hscale.data_ptr(), hout.data_ptr(), hout.stride(0), int(hsh), int(h2_off), dot.data_ptr(), _ptr(partial), _stream())), "spmm_dot_halves")
    return dot


def spmm_bcast(d, x, w, wperm=None, head_outer=True):
    """out[r,h,:] = sum_k w[wperm[k],h] * x[indices[k],:]   x: [n_src, D] (row stride allowed), w: [nnz, H<=4].
    Returns [H, n_rows, D] (head_outer, the batched-GEMM layout) or [n_rows, H, D]."""
    _dev(x, w, d.indptr)
    _f32(x, "x")
    if x.stride(1) != 1:
        x = x.contiguous()
    w = _f32(w, "w").contiguous()
    H, D = w.shape[1], x.shape[1]
    if head_outer:
        out = torch.empty((H, d.n_rows, D), dtype=torch.float32, device=x.device)
        ldo, hso = D, d.n_rows * D
    else:
        out = torch.empty((d.n_rows, H, D), dtype=torch.float32, device=x.device)
        ldo, hso = H * D, D
    partial = None
    if d.n_long:
        partial = torch.empty(int(_lib.bot_spmm_workspace_floats(d.n_slots, H, D)), dtype=torch.float32, device=x.device)
    _check(_timed("spmm_bcast", (H, D), lambda: _lib.bot_spmm_bcast_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(_i32(wperm, "wperm")), H, D, out.data_ptr(),
        ldo, hso, _ptr(partial), _stream())), "spmm_bcast")
    return out


def spmm_bcast_halves(d, x, w, wperm, hscale, hout, col0, hsh, h2_off, hpiece):
    """spmm_bcast with the result written as fp16 halves [h1 | 2^11 h2] of hscale[0] * out into the operand buffer `hout` [n_rows, ld]:
    head h's row block at columns col0 + h hsh .. + hpiece - 1 (zeros behind the D = x.shape[1] columns), the second half h2_off columns
    behind the first — the aggregated slab of the aggregate-first GAT layer as a GEMM operand, no fp32 copy (bot_spmm_bcast_halves_f16)."""
    _dev(x, w, d.indptr, hout, hscale)
    _f32(x, "x")
    if x.stride(1) != 1:
        x = x.contiguous()
    w = _f32(w, "w").contiguous()
    H, D = w.shape[1], x.shape[1]
    assert hout.dtype == torch.float16 and hout.dim() == 2 and hout.shape[0] == d.n_rows and hout.stride(1) == 1 and col0 % 4 == 0
    assert col0 + h2_off + (H - 1) * hsh + hpiece <= hout.shape[1]
    partial = None
    if d.n_long:
        partial = torch.empty(int(_lib.bot_spmm_workspace_floats(d.n_slots, H, D)), dtype=torch.float32, device=x.device)
    _check(_timed("spmm_bcast", (H, D), lambda: _lib.bot_spmm_bcast_halves_f16(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(_i32(wperm, "wperm")), H, D, hscale.data_ptr(),
        hout.data_ptr() + 2 * col0, hout.stride(0), hsh, h2_off, hpiece, _ptr(partial), _stream())), "spmm_bcast_halves")
    return hout


def spmm_dot_bcast(d, x, w, wperm, y, out=None):
    """Backward of spmm_bcast on direction `d`: x [H, n, D] head-outer (gradient of the aggregated slab), y [n_rows, D] the
    layer input.  Returns (out [n_rows, D] = sum_k sum_h w x, dot [nnz, H] = <y[r], x[indices[k],h]>); `out` may be a
    row-strided [n_rows, D] view."""
    _dev(x, w, y, d.indptr)
    _f32(x, "x"), _f32(y, "y")
    assert x.dim() == 3 and x.is_contiguous()
    if y.stride(1) != 1:
        y = y.contiguous()
    H, n, D = x.shape
    w = _f32(w, "w").contiguous()
    if out is None:
        out = torch.empty((d.n_rows, D), dtype=torch.float32, device=x.device)
    assert out.stride(1) == 1 and out.shape == (d.n_rows, D)
    dot = torch.empty((d.nnz, H), dtype=torch.float32, device=x.device)
    partial = None
    if d.n_long:
        partial = torch.empty(int(_lib.bot_spmm_workspace_floats(d.n_slots, 1, D)), dtype=torch.float32, device=x.device)
    _check(_timed("spmm_dot_bcast", (H, D), lambda: _lib.bot_spmm_dot_bcast_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, x.data_ptr(), D, n * D, w.data_ptr(), _ptr(_i32(wperm, "wperm")), y.data_ptr(), y.stride(0),
        H, D, out.data_ptr(), out.stride(0), dot.data_ptr(), _ptr(partial), _stream())), "spmm_dot_bcast")
    return out, dot


def sddmm_dot(d, x, y, operm=None, out=None):
    """out[operm[k],h] = <x[indices[k],h,:], y[r,h,:]> for every position k of every row r.  -> [nnz,H]"""
    _dev(x, y, d.indptr)
    x, ldx, hsx = _slab(x, "x")
    y, ldy, hsy = _slab(y, "y")
    H, D = x.shape[1], x.shape[2]
    if out is None:
        out = torch.empty((d.nnz, H), dtype=torch.float32, device=x.device)
    _check(_timed("sddmm_dot", (H, D), lambda: _lib.bot_sddmm_dot_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, x.data_ptr(), ldx, hsx,
        y.data_ptr(), ldy, hsy, H, D, out.data_ptr(), _ptr(_i32(operm, "operm")), 0, _stream())), "sddmm_dot")
    return out


def sddmm_dot_bcast(d, x, y, operm=None):
    """out[operm[k],h] = <x[indices[k],:], y[h,r,:]> — x [n_src, D] (row stride allowed), y [H, n_rows, D] head-outer.  -> [nnz,H]"""
    _dev(x, y, d.indptr)
    _f32(x, "x"), _f32(y, "y")
    if x.stride(1) != 1:
        x = x.contiguous()
    assert y.dim() == 3 and y.is_contiguous()
    H, n, D = y.shape
    out = torch.empty((d.nnz, H), dtype=torch.float32, device=x.device)
    _check(_timed("sddmm_dot_bcast", (H, D), lambda: _lib.bot_sddmm_dot_bcast_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, x.data_ptr(), x.stride(0),
        y.data_ptr(), D, n * D, H, D, out.data_ptr(), _ptr(_i32(operm, "operm")), _stream())), "sddmm_dot_bcast")
    return out


def u_add_v(src, dst, x, y=None):
    """out[e,:] = x[src[e],:] (+ y[dst[e],:]).  x, y: [n,W] float32; src/dst: int32 [E]."""
    _dev(x, y, src)
    x = _f32(x, "x").contiguous()
    y = None if y is None else _f32(y, "y").contiguous()
    E, W = src.numel(), x.shape[1]
    out = torch.empty((E, W), dtype=torch.float32, device=x.device)
    _check(_lib.bot_sddmm_u_add_v_f32(_i32(src, "src").data_ptr(), _ptr(_i32(dst, "dst")), E, x.data_ptr(), _ptr(y), W,
                                      out.data_ptr(), _stream()), "u_add_v")
    return out


def zsign_buffer(d, H, slope):
    """uint8 [nnz] for the forward to record [z > 0] per head (H <= 8, slope != 1), else None: the backward then skips the
    el[src] gather and the ee / edge-id reads."""
    if os.environ.get("BOT_NO_ZSIGN"):  # measurements: the backward re-derives the signs from el / er / ee
        return None
    return torch.empty(d.nnz, dtype=torch.uint8, device=d.indptr.device) if (H <= 8 and slope != 1.0 and d.indptr.is_cuda) else None


def gat_attn_fwd(d, el, er, ee, eperm, keep, slope, H, aperm, zsign=None, drop=None):
    """Fused logits + leaky-ReLU + per-row softmax.  el/er: [n,H]; ee: [nnz,H] via eperm; -> a [nnz,H].
    `zsign`: optional uint8 [nnz] output (see zsign_buffer).  `drop` = (p, seed) with p > 0: also returns
    a_drop = a * keep / (1 - p) (the attention dropout of models.py:544, Philox mask) -> (a, a_drop).
    Non-finite logits: a -inf logit counts as a dropped edge (weight 0; the rest of the row is the softmax without it); a NaN or
    +inf logit makes every kept weight of its (row, head) NaN and touches nothing else.  A stated departure from the reference: a
    (row, head) whose logits are all -inf gives zeros, as an all-dropped row does, where torch's softmax gives NaN."""
    _dev(el, er, ee, d.indptr)
    el = None if el is None else _f32(el, "el").contiguous()
    er = None if er is None else _f32(er, "er").contiguous()
    ee = None if ee is None else _f32(ee, "ee").contiguous()
    if keep is not None and (keep.dtype != torch.uint8 or not keep.is_contiguous()):
        raise BotKernelError("keep must be contiguous uint8")
    a = torch.empty((d.nnz, H), dtype=torch.float32, device=d.indptr.device)
    p, seed = drop if drop is not None else (0.0, 0)
    a_drop = torch.empty_like(a) if p > 0 else None
    _check(_lib.bot_gat_attn_fwd_f32(d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, _ptr(d.long_rows), d.n_long,
                                     d.chunk, _ptr(el), _ptr(er), _ptr(ee), _ptr(_i32(eperm, "eperm")), _ptr(keep),
                                     float(slope), H, a.data_ptr(), _ptr(_i32(aperm, "aperm")), _ptr(zsign), float(p),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _seed_off(p), _ptr(a_drop), _stream()), "gat_attn_fwd")
    return a if drop is None else (a, a_drop if a_drop is not None else a)


def gat_attn_bwd(d, el, er, ee, eperm, slope, H, a, da, aperm, zperm, want_der, zsign=None, drop=None):
    """Backward of gat_attn_fwd -> (dz [nnz,H] at zperm, der [n_rows,H] or None).  `zsign`: what the forward recorded.
    `drop` = the forward's (p, seed): `da` is then the gradient of a_drop."""
    _dev(a, da, d.indptr)
    el = None if el is None else _f32(el, "el").contiguous()
    er = None if er is None else _f32(er, "er").contiguous()
    ee = None if ee is None else _f32(ee, "ee").contiguous()
    a = _f32(a, "a").contiguous()
    da = _f32(da, "da").contiguous()
    dz = torch.empty((d.nnz, H), dtype=torch.float32, device=a.device)
    der = torch.empty((d.n_rows, H), dtype=torch.float32, device=a.device) if want_der else None
    _check(_lib.bot_gat_attn_bwd_f32(d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, _ptr(d.long_rows), d.n_long,
                                     d.chunk, _ptr(el), _ptr(er), _ptr(ee), _ptr(_i32(eperm, "eperm")), float(slope), H,
                                     a.data_ptr(), da.data_ptr(), _ptr(_i32(aperm, "aperm")), dz.data_ptr(),
                                     _ptr(_i32(zperm, "zperm")), _ptr(der), _ptr(zsign), float(drop[0]) if drop else 0.0,
                                     (int(drop[1]) & 0xFFFFFFFFFFFFFFFF) if drop else 0, _seed_off(drop[0]) if drop else None,
                                     _stream()), "gat_attn_bwd")
    return dz, der


def gat_infer(d, x, el=None, er=None, ee=None, ew=None, slope=0.2, addend=None, scale=None, shift=None, relu=False, out=None, absmax=None):
    """Inference-only GAT layer in one sweep (include/bot_gnn.h bot_gat_infer_f32):
        out[r,h,:] = act((sum_k softmax_k(leaky(el[src] + er[r] + ee[k]))[h] * ew[k] * x[src,h,:] + addend[r,h,:]) * scale + shift)
    x: [n_src,H,D] (strided slab); el [n_src,H] / er [n_rows,H]: row-strided views allowed; ee [nnz,H], ew [nnz]: position order;
    addend [n_rows,H,D]; scale / shift [H*D].  el None: plain ew-weighted sum (no softmax).  Returns [n_rows,H,D]."""
    _dev(x, el, er, ee, ew, addend, scale, shift, d.indptr)
    x, ldx, hsx = _slab(x, "x")
    H, D = x.shape[1], x.shape[2]

    def node2(t, name):
        if t is None:
            return None, 0
        _f32(t, name)
        t = t.reshape(t.shape[0], -1) if t.dim() != 2 else t
        if t.shape[1] != H:
            raise BotKernelError(f"{name} must be [n,{H}], got {tuple(t.shape)}")
        if t.stride(1) != 1 and H > 1:
            t = t.contiguous()
        return t, (t.stride(0) if t.shape[0] > 1 else H)
    el, ldel = node2(el, "el")
    er, lder = node2(er, "er")
    if ee is not None:
        ee = _f32(ee, "ee").reshape(-1, H).contiguous()
    if ew is not None:
        ew = _f32(ew, "ew").reshape(-1).contiguous()
    lda = hsa = 0
    if addend is not None:
        addend, lda, hsa = _slab(addend, "addend")
    scale = None if scale is None else _f32(scale, "scale").reshape(-1).contiguous()
    shift = None if shift is None else _f32(shift, "shift").reshape(-1).contiguous()
    if out is None:
        out = torch.empty((d.n_rows, H, D), dtype=torch.float32, device=x.device)
    out_, ldo, hso = _slab(out, "out")
    assert out_ is out
    ws = None
    if d.n_long:
        ws = torch.empty(int(_lib.bot_gat_infer_workspace_floats(d.n_slots, H, D)), dtype=torch.float32, device=x.device)
    _check(_timed("gat_infer", (H, D, el is not None), lambda: _lib.bot_gat_infer_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows),
        _ptr(d.long_ptr), d.n_long, d.n_slots, x.data_ptr(), ldx, hsx, _ptr(el), ldel, _ptr(er), lder, _ptr(ee), _ptr(ew),
        float(slope), H, D, _ptr(addend), lda, hsa, _ptr(scale), _ptr(shift), int(bool(relu)), out.data_ptr(), ldo, hso, _ptr(ws),
        _ptr(absmax), _stream())), "gat_infer")
    return out


def segment_sum(d, vals, perm=None):
    """out[r,:] = sum_k vals[perm[k],:].  vals: [nnz,W] -> [n_rows,W]"""
    _dev(vals, d.indptr)
    vals = _f32(vals, "vals").contiguous()
    W = vals.shape[1]
    out = torch.empty((d.n_rows, W), dtype=torch.float32, device=vals.device)
    _check(_lib.bot_segment_sum_f32(d.indptr.data_ptr(), d.n_rows, d.nnz, _ptr(d.long_rows), d.n_long, d.chunk, vals.data_ptr(),
                                    _ptr(_i32(perm, "perm")), W, out.data_ptr(), _stream()), "segment_sum")
    return out


def gather_rows(x, rows, out=None):
    """out[i,:] = x[rows[i],:]   x: [n,F] float32 (row stride allowed), rows: int32; `out` may be row-strided."""
    _dev(x, rows)
    _f32(x, "x")
    if x.stride(1) != 1:
        x = x.contiguous()
    if out is None:
        out = torch.empty((rows.numel(), x.shape[1]), dtype=torch.float32, device=x.device)
    assert out.stride(1) == 1 and out.shape == (rows.numel(), x.shape[1])
    _check(_lib.bot_gather_rows_f32(x.data_ptr(), x.stride(0), _i32(rows, "rows").data_ptr(), rows.numel(), x.shape[1],
                                    out.data_ptr(), out.stride(0), _stream()), "gather_rows")
    return out


def scatter_add_rows(x, rows, vals):
    """x[rows[i],:] += vals[i,:] in place; rows sorted-unique int32."""
    _dev(x, rows, vals)
    _f32(x, "x"), _f32(vals, "vals")
    assert x.stride(1) == 1
    vals = vals.contiguous()
    _check(_lib.bot_scatter_add_rows_f32(x.data_ptr(), x.stride(0), _i32(rows, "rows").data_ptr(), rows.numel(), x.shape[1],
                                         vals.data_ptr(), vals.stride(0), _stream()), "scatter_add_rows")
    return x


# ------------------------------------------------------------------------------------------------ BatchNorm + ReLU + dropout
# Device word mixed into every fused-dropout Philox key (include/bot_gnn.h `seed_offset`).  None = not used.  A hipGraph-captured
# train step (bot_amd.train.CapturedTrainStep) allocates it and bumps it once per replay, so that replays draw fresh masks.
SEED_OFFSET = None


def _seed_off(p):
    return SEED_OFFSET.data_ptr() if (SEED_OFFSET is not None and p > 0) else None


def _mat(x, name):
    _f32(x, name)
    if x.dim() != 2:
        raise BotKernelError(f"{name} must be [n,F]")
    return x if x.stride(1) == 1 else x.contiguous()


def _bn_ws(F, device):
    return torch.empty(int(_lib.bot_bn_workspace_floats(F)), dtype=torch.float32, device=device)


def colstats(x):
    """Per-column mean and M2 = sum (x - mean)^2 of x [n,F] -> (mean [F], m2 [F])."""
    _dev(x)
    x = _mat(x, "x")
    n, F = x.shape
    mean = torch.empty(F, dtype=torch.float32, device=x.device)
    m2 = torch.empty(F, dtype=torch.float32, device=x.device)
    _check(_lib.bot_colstats_f32(x.data_ptr(), x.stride(0), n, F, mean.data_ptr(), m2.data_ptr(), _bn_ws(F, x.device).data_ptr(),
                                 _stream()), "colstats")
    return mean, m2


def halves_scale(x):
    """scale [2] = (s, 1/s), s = 2^(14 - ceil(log2 max|x|)) of x [n,F] — stays on the device."""
    _dev(x)
    x = _mat(x, "x")
    scale = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(_lib.bot_halves_workspace_floats()), dtype=torch.float32, device=x.device)
    _check(_lib.bot_halves_scale_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], scale.data_ptr(), ws.data_ptr(), _stream()),
           "halves_scale")
    return scale


_SLOT_POOL = {}          # device -> [zeroed block [_SLOT_SETS, slots], next free set]
_SLOT_SETS = 512


def absmax_slots(device):
    """Zeroed words for the producers' max|value| by-products (include/bot_gnn.h "Maxima as by-products").  Handed out from a block zeroed
    by ONE fill per _SLOT_SETS requests (a set is used once: a fill launch per request was 5.7 us of the step each, seven times a step);
    a block lives until its last set is dropped.  Inside a hipGraph capture every request is its own captured fill (a replay must find
    zeros again)."""
    n = int(_lib.bot_absmax_slots())
    dev = torch.device(device)
    if dev.type != "cuda" or torch.cuda.is_current_stream_capturing():
        return torch.zeros(n, dtype=torch.int32, device=dev)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    ent = _SLOT_POOL.get(key)
    if ent is None or ent[1] >= _SLOT_SETS:
        ent = _SLOT_POOL[key] = [torch.zeros((_SLOT_SETS, n), dtype=torch.int32, device=dev), 0]
    ent[1] += 1
    return ent[0][ent[1] - 1]


def absmax_into(x, slots):
    """Fold max|x| of a (row-strided) [n,F] float32 matrix into the slots — for the columns no producer kernel covers."""
    _dev(x, slots)
    x = _mat(x, "x")
    _check(_lib.bot_absmax_slots_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], slots.data_ptr(), _stream()), "absmax_slots")
    return slots


def halves_scale_from_slots(slots, mult=None, cap=None, cap_ratio=1.0):
    """scale [2] = (s, 1/s) from the by-product slots: what halves_scale finds with a pass over the matrix.  `mult`: the scale of mult x
    the slots' maximum (a bound assembled by the caller); `cap`: another (s, 1/s) pair - the result is at most cap[0] * cap_ratio
    (bot_halves_scale_from_slots2_f32)."""
    scale = torch.empty(2, dtype=torch.float32, device=slots.device)
    if mult is None and cap is None:
        _check(_lib.bot_halves_scale_from_slots_f32(slots.data_ptr(), scale.data_ptr(), _stream()), "halves_scale_from_slots")
    else:
        _dev(cap)
        _check(_lib.bot_halves_scale_from_slots2_f32(slots.data_ptr(), float(1.0 if mult is None else mult), _ptr(cap), float(cap_ratio), scale.data_ptr(),
                                                     _stream()), "halves_scale_from_slots2")
    return scale


def halves_tail(segments, scale, out, h2_off):
    """Column segments of the LEFT halves operand `out` [n, ld] (h1 at column c, 2^11 h2 at c + h2_off) from small fp32 sources, or zeroed:
    segments = [(col, width, src [n, width] float32 (row-strided) or None), ...]  (bot_halves_tail_f16)."""
    _dev(out, scale)
    assert out.dtype == torch.float16 and out.stride(1) == 1 and 1 <= len(segments) <= 8
    n = out.shape[0]
    cols = (c_int64 * (2 * len(segments)))()
    srcs = (c_void_p * len(segments))()
    lds = (c_int64 * len(segments))()
    for g, (col, width, src) in enumerate(segments):
        cols[2 * g], cols[2 * g + 1] = int(col), int(width)
        if src is not None:
            _dev(src)
            _f32(src, "segment source")
            if src.shape != (n, width) or src.stride(1) != 1:
                raise BotKernelError(f"halves_tail: segment {g}: source shape {tuple(src.shape)} / stride {tuple(src.stride())} for width {width}")
            srcs[g], lds[g] = src.data_ptr(), src.stride(0)
        else:
            srcs[g], lds[g] = None, 0
    _check(_lib.bot_halves_tail_f16(n, len(segments), cols, srcs, lds, scale.data_ptr(), out.data_ptr(), out.stride(0), int(h2_off), _stream()), "halves_tail")
    return out


def halves_tn_combine(a, b, P, rem_a=None, rem_b=None):
    """out [K, P] = sum_c a[c][:, :P] + (sum_c a[c][:, PP:PP+P] + sum_c b[c][:, :P]) * 2^-11 for a [C, K, 2 PP], b [C, K, PP] contiguous
    (+ remainder chunks rem_a [K, 2 PP] / rem_b [K, PP]) — include/bot_gnn.h bot_halves_tn_combine_f32."""
    _dev(a, b)
    a, b = _f32(a, "a").contiguous(), _f32(b, "b").contiguous()
    if a.dim() == 2:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    C, K, PP2 = a.shape
    PP = PP2 // 2
    assert b.shape == (C, K, PP) and P <= PP
    if rem_a is not None:
        rem_a, rem_b = rem_a.contiguous(), rem_b.contiguous()
        assert rem_a.shape == (K, PP2) and rem_b.shape == (K, PP)
    out = torch.empty((K, P), dtype=torch.float32, device=a.device)
    _check(_lib.bot_halves_tn_combine_f32(a.data_ptr(), b.data_ptr(), C, K, PP, P, _ptr(rem_a), _ptr(rem_b), out.data_ptr(), P, _stream()),
           "halves_tn_combine")
    return out


def halves_split(x, scale, order, piece, out=None):
    """fp16 halves of x [n,F] scaled by scale[0]: [h1|h1|h2] (order 0), [h1|h2|h1] (order 1) or [h1|h2] (order 2: a left operand without
    the duplicate piece), pieces `piece` columns wide."""
    _dev(x, scale)
    x = _mat(x, "x")
    n, F = x.shape
    if out is None:
        out = torch.empty((n, (2 if order == 2 else 3) * piece), dtype=torch.float16, device=x.device)
    _check(_lib.bot_halves_split_f16(x.data_ptr(), x.stride(0), n, F, _ptr(scale), order, out.data_ptr(), out.stride(0), piece, _stream()),
           "halves_split")
    return out


def halves_split_cols(x, scale, order, buf, piece, col, width):
    """Split x [n,F] into columns [col, col + width) of the three pieces of the halves operand `buf` [n, 3 * piece] (zeros behind
    the F columns of x): several matrices side by side as ONE operand under one scale — bot_halves_split_cols_f16.  order 2: the two
    pieces [h1 | 2^11 h2] of a buffer [n, >= 2 * piece], `piece` = the distance of the second half from the first."""
    _dev(x, scale, buf)
    x = _mat(x, "x")
    n, F = x.shape
    assert buf.dtype == torch.float16 and buf.shape[0] == n and buf.shape[1] >= (2 if order == 2 else 3) * piece and buf.stride(1) == 1
    assert col % 2 == 0 and col + width <= piece
    _check(_lib.bot_halves_split_cols_f16(x.data_ptr(), x.stride(0), n, F, _ptr(scale), order, buf.data_ptr() + 2 * col, buf.stride(0), piece,
                                          width, _stream()), "halves_split_cols")
    return buf


def halves_split_heads(x, scale, H, D, DP, out=None):
    """x [n, H * D] (row-strided view allowed) -> the LEFT operand [n, 2 * H * DP] = [h1 | 2^11 h2] with every head's D columns in a block of
    DP (zero padded) — bot_halves_split_heads_f16."""
    _dev(x, scale)
    _f32(x, "x")
    n = x.shape[0]
    assert x.shape[1] == H * D and x.stride(1) == 1
    if out is None:
        out = torch.empty((n, 2 * H * DP), dtype=torch.float16, device=x.device)
    _check(_lib.bot_halves_split_heads_f16(x.data_ptr(), x.stride(0), n, H, D, _ptr(scale), out.data_ptr(), out.stride(0), H * DP, DP, _stream()),
           "halves_split_heads")
    return out


_GEMM_WS = {}
# Kernel choice for shapes without a recorded selection.  0 (default): hipBLASLt's first heuristic choice — no timing runs, no
# synchronisation, the same kernel in every run and on every rank.  Opt-in (maintenance / exploration, NOT bitwise reproducible across
# runs, synchronises on the first call per shape): 1 = fastest of 16 heuristic candidates timed on the caller's buffers, 2 = of all
# solutions (tools/tune_halves_gemm.py, which records the winners in bot_amd/tuning/halves_gemm.json).
GEMM_TUNE = int(os.environ.get("BOT_GEMM_TUNE", "0"))
GEMM_ALGOS = None      # {shape key: hipBLASLt solution index} recorded by tools/tune_halves_gemm.py (bot_amd/tuning/halves_gemm.json)
GEMM_SEEN = None       # tools set this to a dict to collect {shape key: (solution index, ms in the search)} of the launches


def _gemm_algos():
    global GEMM_ALGOS
    if GEMM_ALGOS is None:
        GEMM_ALGOS = {}
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning", "halves_gemm.json")
        if os.environ.get("BOT_GEMM_ALGOS", "1") != "0" and os.path.exists(path):
            import json
            with open(path) as f:
                rec = json.load(f)
            # indices are only meaningful for the library build they were recorded on
            if rec.get("hipblaslt") == _hipblaslt_tag():
                GEMM_ALGOS = {k: int(v["index"]) for k, v in rec.get("shapes", {}).items()}
    return GEMM_ALGOS


def _hipblaslt_tag():
    """Identifies the hipBLASLt build whose solution indices the tuning file holds: torch's version string (it ships the library)."""
    return f"torch {torch.__version__} hip {torch.version.hip}"


def hipblaslt_versions():
    """(compiled-against, running-on) hipBLASLt versions as major * 100000 + minor * 100 + patch; running-on is 0 before the first
    gemm_halves call.  The library is built with /opt/rocm's headers and binds whichever libhipblaslt.so the process loaded first
    — torch's bundled copy when torch is imported (same soname).  A different MAJOR means another struct layout: refuse."""
    c, r = c_int32(0), c_int32(0)
    _lib.bot_gemm_halves_library_version(ctypes.byref(c), ctypes.byref(r))
    return c.value, r.value


_LT_CHECKED = False


def gemm_halves(a, b, alpha, *, trans_a=False, trans_b=False, out=None, batch=1, strides=(0, 0, 0), m=None, n=None, k=None, beta=0.0,
                ldc=None):
    """C[m,n] = alpha[j] * op(a) op(b): a, b fp16 matrices (row-major views, unit column stride), C fp32; `alpha` a device
    vector of n floats (a 1-element tensor is expanded).  beta != 0 accumulates onto `out`; `ldc` overrides out's row pitch
    (batched products written side by side into the columns of one matrix: strides[2] = the column offset per batch).  m / n / k default to the operands' shapes; batch > 1 with element strides (a, b, c) for strided batches."""
    _dev(a, b, alpha)
    if a.dtype != torch.float16 or b.dtype != torch.float16 or a.stride(-1) != 1 or b.stride(-1) != 1:
        raise BotKernelError("gemm_halves: operands must be fp16 with unit column stride")
    if m is None:
        m, k = (a.shape[-1], a.shape[-2]) if trans_a else (a.shape[-2], a.shape[-1])
    if n is None:
        n = b.shape[-2] if trans_b else b.shape[-1]
    if out is None:
        out = torch.empty((m, n) if batch == 1 else (batch, m, n), dtype=torch.float32, device=a.device)
    if alpha.numel() == 1:
        alpha = alpha.reshape(1).expand(n).contiguous()
    if alpha.numel() != n or alpha.dtype != torch.float32:
        raise BotKernelError("gemm_halves: alpha must hold n floats")
    ws = _GEMM_WS.get(a.device)
    if ws is None:
        ws = _GEMM_WS[a.device] = torch.empty(64 << 20, dtype=torch.uint8, device=a.device)
    sa, sb, sc = strides
    if batch > 1 and sc == 0:
        sc = out.stride(0)
    ldc = _ld(out) if ldc is None else ldc
    lda, ldb = _ld(a), _ld(b)
    key = f"{int(trans_a)}{int(trans_b)} m{m} n{n} k{k} lda{lda} ldb{ldb} ldc{ldc} b{batch} s{sa},{sb},{sc}"
    index = _gemm_algos().get(key, -1) if beta == 0.0 else -1
    _check(_timed("gemm_halves", (m, n, k, batch), lambda: _lib.bot_gemm_halves_f32(
        int(trans_a), int(trans_b), m, n, k, alpha.data_ptr(), a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(),
        ldc, batch, sa, sb, sc, float(beta), ws.data_ptr(), ws.numel(), int(GEMM_TUNE), index, _stream())), "gemm_halves")
    global _LT_CHECKED
    if not _LT_CHECKED:
        _LT_CHECKED = True
        c, r = hipblaslt_versions()
        if r and c // 100000 != r // 100000:
            raise BotKernelError(f"libbot_gnn.so was built against hipBLASLt {c} but the process runs on hipBLASLt {r}: rebuild against "
                                 "the headers of the library that is loaded")
    if GEMM_SEEN is not None and key not in GEMM_SEEN:
        idx, ms = ctypes.c_int32(-1), ctypes.c_float(0.0)
        _lib.bot_gemm_halves_last_algo(ctypes.byref(idx), ctypes.byref(ms))
        GEMM_SEEN[key] = (idx.value, ms.value)
    return out


def stream_create(device, high_priority=False):
    """A torch.cuda.ExternalStream over a HIP stream of the library's own (include/bot_gnn.h bot_stream_create): NOT one of torch's pooled
    streams."""
    h = c_void_p()
    with torch.cuda.device(device):
        _check(_lib.bot_stream_create(int(bool(high_priority)), ctypes.byref(h)), "stream_create")
    return torch.cuda.ExternalStream(h.value, device=device)


def debug_abort_trace(path):
    """include/bot_gnn.h bot_debug_abort_trace: a SIGABRT / std::terminate in this process leaves the aborting thread's native frames in
    `path` (diagnostic; armed by tests/conftest.py, never by the product)."""
    _check(_lib.bot_debug_abort_trace(os.fsencode(path)), "debug_abort_trace")


class _BnBwdStats(ctypes.Structure):
    """include/bot_gnn.h bot_bn_bwd_stats_t"""
    _fields_ = [("x", c_void_p), ("ldx", c_int64), ("mean", c_void_p), ("invstd", c_void_p), ("weight", c_void_p), ("bias", c_void_p), ("relu", c_int32),
                ("p", c_float), ("seed", c_uint64), ("seed_offset", c_void_p), ("part", c_void_p), ("pmax", c_void_p)]


class BnBwdStats:
    """The reduce pass of a fused BatchNorm / ReLU / dropout epilogue's backward as a by-product of the NT product that writes the epilogue's
    incoming gradient (include/bot_gnn.h "v18"): x [m, F] the epilogue's input, the statistics / affine vectors, the dropout (p, seed) of its
    forward.  `gemm_halves3_nt(..., bn=this)` fills part / pmax [ceil(m / 256), 2, F]; `sums()` / `bound()` finish them."""

    def __init__(self, x, mean, invstd, weight, bias, relu, p, seed, want_max=True):
        _dev(x, mean, invstd, weight, bias)
        self.x = _mat(x, "x")
        self.mean, self.invstd, self.weight, self.bias = _f32(mean, "mean"), _f32(invstd, "invstd"), weight, bias
        self.relu, self.p, self.seed = bool(relu), float(p), int(seed)
        n, F = self.x.shape
        self.n, self.F, self.nblk = n, F, (n + 255) // 256
        self.part = torch.empty((self.nblk, 2, F), dtype=torch.float32, device=x.device)
        self.pmax = torch.empty((self.nblk, 2, F), dtype=torch.float32, device=x.device) if want_max else None

    def fits(self, m, n, k) -> bool:
        """The product [m, n] of piece width k can carry the by-product: the 256 x 32 form, n = F even, 8-byte aligned x rows."""
        return (m == self.n and n == self.F and self.F % 2 == 0 and self.x.stride(0) % 2 == 0 and self.x.data_ptr() % 8 == 0 and
                _lib.bot_gemm_halves3_nt_bn_rows(int(k)) == 256)

    def struct(self):
        return _BnBwdStats(self.x.data_ptr(), self.x.stride(0), self.mean.data_ptr(), self.invstd.data_ptr(), _ptr(self.weight), _ptr(self.bias),
                           int(self.relu), self.p, self.seed, _seed_off(self.p), self.part.data_ptr(), _ptr(self.pmax))

    def sums(self):
        sg = torch.empty(self.F, dtype=torch.float32, device=self.x.device)
        sgx = torch.empty(self.F, dtype=torch.float32, device=self.x.device)
        _check(_lib.bot_bn_act_bwd_reduce_partials_f32(self.part.data_ptr(), self.nblk, self.F, sg.data_ptr(), sgx.data_ptr(), _stream()),
               "bn_act_bwd_reduce_partials")
        return sg, sgx

    def finish(self, batch_stats, total_count, slots):
        """sums() and bound() in one launch (one rank: the local sums are the final ones) -> (sum_g, sum_gx)"""
        assert self.pmax is not None
        _dev(slots)
        sg = torch.empty(self.F, dtype=torch.float32, device=self.x.device)
        sgx = torch.empty(self.F, dtype=torch.float32, device=self.x.device)
        _check(_lib.bot_bn_bwd_partials_finish_f32(self.part.data_ptr(), self.pmax.data_ptr(), self.nblk, self.F, sg.data_ptr(), sgx.data_ptr(),
                                                   int(bool(batch_stats)), float(total_count), _ptr(self.weight), self.invstd.data_ptr(), slots.data_ptr(),
                                                   _stream()), "bn_bwd_partials_finish")
        return sg, sgx

    def bound(self, sum_g, sum_gx, total_count, slots):
        assert self.pmax is not None
        _dev(slots)
        _check(_lib.bot_bn_bwd_bound_partials_f32(self.F, self.pmax.data_ptr(), self.nblk, _ptr(sum_g), _ptr(sum_gx), float(total_count), _ptr(self.weight),
                                                  self.invstd.data_ptr(), slots.data_ptr(), _stream()), "bn_bwd_bound_partials")
        return slots


def gemm_halves3_nt(a, b, scale_a, scale_b, piece_a, piece_b, k, out=None, mode=0, a2_off=None, scale_a2=None, k_split=0, b_frag=False, n=None, bn=None):
    """out[m, n] = scale_a[1] scale_b[1] (a1 b1^T + a1 b2^T + a2 b1^T) from a LEFT operand buffer a [m, 3 piece_a] (or [m, 2 piece_a]
    without the duplicate piece: a2_off = piece_a) and a RIGHT operand buffer b [n, 3 piece_b] (bot_amd.gemm.Halves.buf / .scale), k =
    the common piece width used (bot_gemm_halves3_nt_f32).  scale_a2 / k_split: a's columns from k_split (a multiple of 32) on were
    written under a second scale (bot_gemm_halves3_nt2_f32).  b_frag: b is a fragment-major right operand (halves_split_frag) of `n` rows."""
    _dev(a, b, scale_a, scale_b, scale_a2)
    m = a.shape[0]
    if n is None:
        assert not b_frag
        n = b.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    # bn (BnBwdStats): out is the gradient arriving at that epilogue - its reduce pass leaves with the tiles (bot_gemm_halves3_nt3_f32)
    st = None
    if bn is not None:
        if not bn.fits(m, n, k):
            raise BotKernelError("gemm_halves3_nt: this product cannot carry the BatchNorm-backward by-product (BnBwdStats.fits)")
        st = bn.struct()
    _check(_timed("gemm_halves", (m, n, 3 * k, 1), lambda: _lib.bot_gemm_halves3_nt3_f32(
        m, n, k, scale_a.data_ptr(), _ptr(scale_a2), int(k_split), scale_b.data_ptr(), a.data_ptr(), _ld(a), 2 * piece_a if a2_off is None else a2_off,
        b.data_ptr(), _ld(b), piece_b, int(bool(b_frag)), out.data_ptr(), _ld(out), ctypes.addressof(st) if st is not None else None, int(mode), _stream())),
        "gemm_halves3_nt")
    return out


def dh_deferred_max_k() -> int:
    return int(_lib.bot_gemm_halves3_nt_bn_deferred_max_k())


def gemm_halves3_nt_bn_reduce(a, b, scale_a, scale_b, piece_b, k, bn, a2_off, scale_a2=None, k_split=0, b_frag=False, n=None, out=None):
    """gemm_halves3_nt(..., bn=bn) WITHOUT its output: only bn.part / bn.pmax are written, the same bits (include/bot_gnn.h "d h recomputed
    in the apply", bot_gemm_halves3_nt_bn_reduce_f32).  The product itself is formed again by gemm_halves3_nt_bn_apply.  `out`: where the
    storing launch would write (tests: it stays untouched); normally None."""
    _dev(a, b, scale_a, scale_b, scale_a2, out)
    m = a.shape[0]
    n = b.shape[0] if n is None else n
    st = bn.struct()
    _check(_timed("gemm_halves", (m, n, 3 * k, 1), lambda: _lib.bot_gemm_halves3_nt_bn_reduce_f32(
        m, n, k, scale_a.data_ptr(), _ptr(scale_a2), int(k_split), scale_b.data_ptr(), a.data_ptr(), _ld(a), a2_off, b.data_ptr(), _ld(b), piece_b,
        int(bool(b_frag)), _ptr(out), _ld(out) if out is not None else 0, ctypes.addressof(st), _stream())), "gemm_halves3_nt_bn_reduce")


def gemm_halves3_nt_bn_apply(a, b, scale_a, scale_b, piece_b, k, bn, a2_off, sum_g, sum_gx, total_count, scale_a2=None, k_split=0, b_frag=False, n=None,
                             out=None, hscale=None, hout=None, hD=2, hDP=2, h2_off=None, absmax=None):
    """bn_act_bwd_apply / bn_act_bwd_apply_halves on the product a b^T, which is formed again tile by tile and never stored
    (bot_gemm_halves3_nt_bn_apply_f32): `out` fp32 dx (optional, may be row-strided), `hout` the LEFT halves operand under `hscale` (optional,
    arguments as bn_act_bwd_apply_halves), `absmax` slots for max|dx|."""
    _dev(a, b, scale_a, scale_b, scale_a2, out, hout, hscale, absmax)
    m = a.shape[0]
    n = b.shape[0] if n is None else n
    assert out is None or (out.stride(1) == 1 and out.dtype == torch.float32 and out.shape == (m, n))
    if hout is not None:
        if h2_off is None:
            h2_off = (n // hD) * hDP
            assert hout.shape == (m, 2 * h2_off)
        assert hout.dtype == torch.float16 and hout.stride(1) == 1 and hout.shape[0] == m
    st = bn.struct()
    _check(_timed("gemm_halves", (m, n, 3 * k, 1), lambda: _lib.bot_gemm_halves3_nt_bn_apply_f32(
        m, n, k, scale_a.data_ptr(), _ptr(scale_a2), int(k_split), scale_b.data_ptr(), a.data_ptr(), _ld(a), a2_off, b.data_ptr(), _ld(b), piece_b,
        int(bool(b_frag)), ctypes.addressof(st), _ptr(sum_g), _ptr(sum_gx), float(total_count), _ptr(out), out.stride(0) if out is not None else 0,
        _ptr(hscale), _ptr(hout), hout.stride(0) if hout is not None else 0, int(h2_off or 0), int(hD), int(hDP), _ptr(absmax), _stream())),
        "gemm_halves3_nt_bn_apply")
    return out, hout


def halves_split_frag(x, scale, piece):
    """x [n, F] scaled by scale[0] as a RIGHT operand in fragment-major layout (include/bot_gnn.h bot_halves_split_frag_f16): a fp16 buffer
    [2 * ceil(n / 16) * piece / 32, 512] - one row per KB fragment block, h1 blocks first, h2 blocks behind them."""
    _dev(x, scale)
    x = _mat(x, "x")
    n, F = x.shape
    assert piece % 64 == 0 and piece >= F
    out = torch.empty((2 * ((n + 15) // 16) * (piece // 32), 512), dtype=torch.float16, device=x.device)
    _check(_lib.bot_halves_split_frag_f16(x.data_ptr(), x.stride(0), n, F, _ptr(scale), out.data_ptr(), piece, _stream()), "halves_split_frag")
    return out


def _table(rows, width):
    flat = [int(v) for r in rows for v in r]
    assert len(flat) == width * len(rows)
    return (ctypes.c_int64 * len(flat))(*flat)


def gemm_halves3_nt_grouped(a, b, scale_a, scale_b, a2_off, b2_off, out, groups, k_seg, mode=0, col_scale=None, col_shift=None, relu=False, absmax=None,
                            stats=None):
    """The grouped NT product (bot_gemm_halves3_nt_grouped_f32): for every group (b_row0, n_valid, a_col0, a_col1, k_steps, c_off)
        out.flat[r * ld + c_off + j] = scale_a[1] scale_b[1] * sum_{t < k_steps} sum_{i < 32} A3[r, (a_col0 if t < k_seg else a_col1) + 32 t + i] . B3[b_row0 + j, 32 t + i]
    for j < n_valid <= 256, over the rows of the left operand buffer a ([h1 at column c, 2^11 h2 at column c + a2_off]) and the right
    operand buffer b ([h1 | h2 at + b2_off]); `out` is a row-major fp32 matrix view whose storage the offsets c_off address (ld = its
    row pitch).  The per-head products of the aggregate-first GAT layer in one launch.  Optional epilogue: out = relu?(out * col_scale[c] +
    col_shift[c]) with c = c_off + j (the eval-mode BatchNorm / bias behind the layer) and max|out| into `absmax` slots."""
    _dev(a, b, out, scale_a, scale_b, col_scale, col_shift, absmax)
    assert a.dtype == torch.float16 and b.dtype == torch.float16 and a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    assert out.dtype == torch.float32 and out.stride(-1) == 1
    tab = _table(groups, 6)
    # (profile key: m, n, k, batch with 2 m n k batch = the fp16 MFMA flops of the valid output columns, three products each)
    # stats = (part [tiles, 2, F], minmax [tiles, 2, F], pivot [tiles, F]): column statistics of the stored values as a by-product (tiles =
    # ceil(m / 256) row blocks, F = the width the groups' output columns c_off + j index; all three WRITTEN: the pivot of a tile is its first
    # stored value - bot_gemm_halves3_nt_grouped2_f32; finished by bn_stats_halves_partials)
    sp = sm = sv = None
    sF = 0
    if stats is not None:
        sp, sm, sv = stats
        _dev(sp, sm, sv)
        sF = sv.shape[1]
        tiles = (a.shape[0] + 255) // 256
        assert sp.shape == (tiles, 2, sF) and sm.shape == (tiles, 2, sF) and sv.shape == (tiles, sF)
        assert sp.is_contiguous() and sm.is_contiguous() and sv.is_contiguous()
        assert sp.dtype == sm.dtype == sv.dtype == torch.float32
    _check(_timed("gemm_halves", (a.shape[0], sum(int(g[1]) * 96 * int(g[4]) for g in groups), 1, 1), lambda: _lib.bot_gemm_halves3_nt_grouped2_f32(
        a.shape[0], b.shape[0], scale_a.data_ptr(), scale_b.data_ptr(), a.data_ptr(), _ld(a), a2_off, b.data_ptr(), _ld(b), b2_off, out.data_ptr(),
        int(out.stride(-2)), len(groups), tab, int(k_seg), _ptr(col_scale), _ptr(col_shift), int(bool(relu)), _ptr(absmax), _ptr(sp), _ptr(sm), _ptr(sv),
        int(sF), int(mode), _stream())), "gemm_halves3_nt_grouped")
    return out


def gemm_halves3_tn_grouped(x, d, scale_x, scale_d, x2_off, d2_off, out, tiles, mode=0):
    """The grouped TN product (bot_gemm_halves3_tn_grouped_f32): for every tile (x_col0, k_valid, d_col0, p_valid, out_off, ldo, transposed)
        out.flat[out_off + k * ldo + p] = scale_x[1] scale_d[1] * sum_n X3[n, x_col0 + k] . D3[n, d_col0 + p],  k < k_valid <= 192, p < p_valid <= 192
    (transposed: out.flat[out_off + p * ldo + k])
    over the rows of two LEFT operand buffers (h1 at column c, 2^11 h2 at c + x2_off / d2_off); `out` is one contiguous fp32 buffer that
    the offsets address.  The weight gradients of the aggregate-first GAT layer (per head, and of its merged projection) in one launch."""
    _dev(x, d, out, scale_x, scale_d)
    assert x.dtype == torch.float16 and d.dtype == torch.float16 and x.stride(1) == 1 and d.stride(1) == 1 and x.shape[0] == d.shape[0]
    assert out.dtype == torch.float32 and out.is_contiguous()
    n = x.shape[0]
    ws = torch.empty(int(_lib.bot_gemm_halves3_tn_grouped_workspace_floats(n, len(tiles))), dtype=torch.float32, device=x.device)
    tab = _table(tiles, 7)
    _check(_timed("gemm_halves", (n, sum(3 * int(t[1]) * int(t[3]) for t in tiles), 1, 1), lambda: _lib.bot_gemm_halves3_tn_grouped_f32(
        n, scale_x.data_ptr(), scale_d.data_ptr(), x.data_ptr(), _ld(x), x2_off, d.data_ptr(), _ld(d), d2_off, out.data_ptr(), len(tiles), tab,
        ws.data_ptr(), int(mode), _stream())), "gemm_halves3_tn_grouped")
    return out


def gemm_halves3_tn(x, d, scale_x, scale_d, piece_x, piece_d, k, p, mode=0, x2_off=None, d2_off=None, scale_d2=None, p_split=0):
    """out[k, p] = scale_x[1] scale_d[1] (x1^T d1 + x1^T d2 + x2^T d1) from two LEFT operand buffers x [n, 3 piece_x], d [n, 3 piece_d]
    (include/bot_gnn.h bot_gemm_halves3_tn_f32): the weight gradient of a projection, reduced over the n rows.  scale_d2 / p_split: d's
    columns from p_split (a multiple of 4) on were written under a second scale (bot_gemm_halves3_tn2_f32)."""
    _dev(x, d, scale_x, scale_d, scale_d2)
    n = x.shape[0]
    out = torch.empty((k, p), dtype=torch.float32, device=x.device)
    ws = torch.empty(int(_lib.bot_gemm_halves3_tn_workspace_floats(n, piece_x, piece_d)), dtype=torch.float32, device=x.device)
    _check(_timed("gemm_halves", (k, p, 3 * n, 1), lambda: _lib.bot_gemm_halves3_tn2_f32(
        n, k, p, piece_x, piece_d, scale_x.data_ptr(), scale_d.data_ptr(), _ptr(scale_d2), int(p_split), x.data_ptr(), _ld(x),
        2 * piece_x if x2_off is None else x2_off, d.data_ptr(), _ld(d), 2 * piece_d if d2_off is None else d2_off,
        out.data_ptr(), _ld(out), ws.data_ptr(), int(mode), _stream())), "gemm_halves3_tn")
    return out


def _idx64(t, name):
    if t.dtype != torch.int64 or not t.is_contiguous() or t.dim() != 1:
        raise BotKernelError(f"{name} must be a contiguous 1-D int64 tensor (got {t.dtype}, stride {tuple(t.stride())})")


def _labels64(labels):
    """[N] or [N, 1..] int64 labels as a 2-D view with unit column stride (the kernels read column 0 at a row stride)."""
    if labels.dtype != torch.int64:
        raise BotKernelError(f"labels must be int64 (got {labels.dtype})")
    lab = labels.reshape(labels.shape[0], -1)
    if lab.shape[1] > 1 and lab.stride(1) != 1:
        lab = lab.contiguous()
    return lab


def label_split(train_idx, labels, mask, mask_rate, seed, use_labels, code, wn):
    """include/bot_gnn.h bot_label_split_f32: writes code / wn at the training nodes, returns count (1-element float tensor on the device)."""
    _dev(train_idx, labels, wn)
    _idx64(train_idx, "train_idx")
    count = torch.empty(1, dtype=torch.float32, device=wn.device)
    ws = torch.empty(128, dtype=torch.int32, device=wn.device)
    lab = _labels64(labels)
    if wn.dtype != torch.float32 or not wn.is_contiguous() or (code is not None and (code.dtype != torch.int32 or not code.is_contiguous())):
        raise BotKernelError("label_split: wn must be contiguous float32, code contiguous int32")
    m = None
    if mask is not None:            # one byte per training node, nonzero = an input-label node (a float 0/1 mask is converted, not reinterpreted)
        _dev(mask)
        m = mask.to(torch.bool).contiguous().view(torch.uint8)
        if m.numel() != train_idx.numel():
            raise BotKernelError("label_split: mask must have one entry per training node")
    _check(_lib.bot_label_split_f32(train_idx.data_ptr(), train_idx.numel(), lab.data_ptr(), lab.stride(0), _ptr(m), float(mask_rate), int(seed),
                                    _seed_off(1.0), int(bool(use_labels)), _ptr(code), wn.data_ptr(), count.data_ptr(), ws.data_ptr(), _stream()), "label_split")
    return count


def build_input(feat, code, n_classes, p, seed):
    """include/bot_gnn.h bot_build_input_f32: dropout_p([feat | onehot(code)]) as a new [N, F + C] tensor."""
    _dev(feat)
    _f32(feat, "feat")
    n, F = feat.shape
    out = torch.empty((n, F + n_classes), dtype=torch.float32, device=feat.device)
    _check(_lib.bot_build_input_f32(feat.data_ptr(), _ld(feat), n, F, n_classes, _ptr(code), float(p), int(seed), _seed_off(p), out.data_ptr(), _ld(out),
                                    _stream()), "build_input")
    return out


REUSE_CALLS = 0     # number of build_input_reuse launches (tests assert the label-reuse passes took the fused path)


def build_input_reuse(feat, code, reuse, pred, n_classes, p, seed, out=None):
    """include/bot_gnn.h bot_build_input_reuse_f32: dropout_p([feat | onehot(code) or softmax(pred) or 0]) as a new [N, F + C] tensor, or into `out`.
    `reuse`: uint8 [N], nonzero = the node takes the previous prediction when it has no input label; None = every node does."""
    global REUSE_CALLS
    _dev(feat, code, reuse, pred, out)
    _f32(feat, "feat"), _f32(pred, "pred"), _f32(out, "out")
    n, F = feat.shape
    if feat.stride(1) != 1 and F > 1:
        feat = feat.contiguous()
    if pred.dim() != 2 or pred.shape[0] != n or pred.shape[1] < n_classes or (pred.stride(1) != 1 and pred.shape[1] > 1):
        raise BotKernelError(f"build_input_reuse: pred must be [{n}, >= {n_classes}] with unit column stride, got {tuple(pred.shape)}")
    if code is None or code.dtype != torch.int32 or not code.is_contiguous() or code.numel() != n:
        raise BotKernelError(f"build_input_reuse: code must be contiguous int32 [{n}]")
    if reuse is not None and (reuse.dtype != torch.uint8 or not reuse.is_contiguous() or reuse.numel() != n):
        raise BotKernelError(f"build_input_reuse: reuse must be contiguous uint8 [{n}]")
    if out is None:
        out = torch.empty((n, F + n_classes), dtype=torch.float32, device=feat.device)
    elif out.shape != (n, F + n_classes) or out.stride(1) != 1:
        raise BotKernelError(f"build_input_reuse: out must be [{n}, {F + n_classes}] with unit column stride")
    _check(_lib.bot_build_input_reuse_f32(feat.data_ptr(), _ld(feat), n, F, n_classes, code.data_ptr(), _ptr(reuse), pred.data_ptr(), _ld(pred), float(p),
                                          int(seed), _seed_off(p), out.data_ptr(), _ld(out), _stream()), "build_input_reuse")
    REUSE_CALLS += 1
    torch.autograd.graph.increment_version(out)     # written behind torch's back: caches keyed by (address, version) must not see the old contents
    return out


LOSS_KINDS = {"logit": 0, "loge": 1, "savage": 2}


def node_loss(x, labels, wn, count, kind, eps, want_grad=True):
    """include/bot_gnn.h bot_node_loss_f32: (y [n_pad] with n_pad = n rounded up to 64, zero beyond n and where wn == 0; dx [n, C] or None)."""
    _dev(x, labels, wn, count)
    _f32(x, "x")
    n, C = x.shape
    n_pad = (n + 63) // 64 * 64
    y = torch.empty(n_pad, dtype=torch.float32, device=x.device)
    dx = torch.empty((n, C), dtype=torch.float32, device=x.device) if want_grad else None
    lab = _labels64(labels)
    if wn.dtype != torch.float32 or not wn.is_contiguous() or count.dtype != torch.float32:
        raise BotKernelError("node_loss: wn / count must be contiguous float32")
    _check(_lib.bot_node_loss_f32(x.data_ptr(), _ld(x), n, C, lab.data_ptr(), lab.stride(0), wn.data_ptr(), count.data_ptr(), LOSS_KINDS[kind], float(eps),
                                  y.data_ptr(), n_pad, _ptr(dx), C, _stream()), "node_loss")
    return y, dx


def node_loss_weighted(x, labels, wn, lw, wsum, kind, eps, want_grad=True):
    """include/bot_gnn.h bot_node_loss_weighted_f32: node_loss with the per-node weights lw [n] and their total over the prediction nodes
    wsum [1]: (y [n_pad] = lw y where wn > 0, dx [n, C] or None)."""
    _dev(x, labels, wn, lw, wsum)
    _f32(x, "x")
    n, C = x.shape
    n_pad = (n + 63) // 64 * 64
    y = torch.empty(n_pad, dtype=torch.float32, device=x.device)
    dx = torch.empty((n, C), dtype=torch.float32, device=x.device) if want_grad else None
    lab = _labels64(labels)
    if wn.dtype != torch.float32 or not wn.is_contiguous() or lw.dtype != torch.float32 or not lw.is_contiguous() or wsum.dtype != torch.float32:
        raise BotKernelError("node_loss_weighted: wn / lw / wsum must be contiguous float32")
    if wn.numel() != n or lw.numel() != n:
        raise BotKernelError(f"node_loss_weighted: wn / lw hold one value per node ({n}), got {wn.numel()} / {lw.numel()}")
    _check(_lib.bot_node_loss_weighted_f32(x.data_ptr(), _ld(x), n, C, lab.data_ptr(), lab.stride(0), wn.data_ptr(), lw.data_ptr(), wsum.data_ptr(),
                                           LOSS_KINDS[kind], float(eps), y.data_ptr(), n_pad, _ptr(dx), C, _stream()), "node_loss_weighted")
    return y, dx


def rmsprop_step(params, grads, square_avgs, lr, alpha, eps, weight_decay, lr_dev=None):
    """include/bot_gnn.h bot_rmsprop_step_f32 over lists of contiguous float32 tensors (48 per launch)."""
    for i in range(0, len(params), 48):
        ps, gs, sq = params[i:i + 48], grads[i:i + 48], square_avgs[i:i + 48]
        k = len(ps)
        for t in (*ps, *gs, *sq):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise BotKernelError("rmsprop_step: contiguous float32 tensors only")
        P = (c_void_p * k)(*[t.data_ptr() for t in ps])
        G = (c_void_p * k)(*[t.data_ptr() for t in gs])
        S = (c_void_p * k)(*[t.data_ptr() for t in sq])
        Nn = (c_int64 * k)(*[t.numel() for t in ps])
        if lr_dev is not None and (lr_dev.dtype != torch.float32 or lr_dev.device != ps[0].device):
            raise BotKernelError("rmsprop_step: a tensor learning rate must be float32 on the parameters' device")
        _check(_lib.bot_rmsprop_step_f32(k, P, G, S, Nn, float(lr), _ptr(lr_dev), float(alpha), float(eps), float(weight_decay), _stream()), "rmsprop_step")


def skinny_gemm(a, b, *, b_is_kn, out, accumulate=False, batch=1, strides=(0, 0, 0), m=None, n=None, k=None, ldc=None):
    """out[m,n] (+)= a[m,k] @ (b if b_is_kn else b^T), k <= 256 (include/bot_gnn.h bot_skinny_gemm_f32): fp32 in and out, bf16x6 MFMA
    products inside.  a, b, out: fp32 row-major views with unit column stride; batch > 1: element strides (a, b, out)."""
    _dev(a, b, out)
    for t, name in ((a, "a"), (b, "b"), (out, "out")):
        _f32(t, name)
        if t.stride(-1) != 1 and t.shape[-1] != 1:
            raise BotKernelError(f"skinny_gemm: {name} must have unit column stride")
    if m is None:
        m, k = a.shape[-2], a.shape[-1]
    if n is None:
        n = b.shape[-1] if b_is_kn else b.shape[-2]
    sa, sb, sc = strides
    _check(_timed("skinny_gemm", (m, n, k, batch), lambda: _lib.bot_skinny_gemm_f32(
        a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), int(b_is_kn), out.data_ptr(), _ld(out) if ldc is None else ldc, m, n, k,
        int(accumulate), batch, sa, sb, sc, _stream())), "skinny_gemm")
    return out


def tn_gemm(x, y, *, out=None, batch=1, strides=(0, 0, 0), n=None, kx=None, ky=None, transpose_out=False):
    """out[kx, ky] = x[n, kx]^T y[n, ky] (include/bot_gnn.h bot_tn_gemm_f32: exact fp32 MFMA, reduction over the n rows);
    transpose_out: out[ky, kx] (workgroup blocks are 256 columns of x by 192 of y: pass the wider operand as x).
    x, y: fp32 row-major views with unit column stride; batch > 1: element strides (x, y, out), out [batch, kx, ky]."""
    _dev(x, y)
    _f32(x, "x"), _f32(y, "y")
    if (x.stride(-1) != 1 and x.shape[-1] != 1) or (y.stride(-1) != 1 and y.shape[-1] != 1):
        raise BotKernelError("tn_gemm: operands must have unit column stride")
    if n is None:
        n, kx, ky = x.shape[-2], x.shape[-1], y.shape[-1]
    if out is None:
        shp = (ky, kx) if transpose_out else (kx, ky)
        out = torch.empty(shp if batch == 1 else (batch,) + shp, dtype=torch.float32, device=x.device)
    sx, sy, so = strides
    if batch > 1 and so == 0:
        so = out.stride(0)
    ws = torch.empty(int(_lib.bot_tn_gemm_workspace_floats(n, kx, ky, batch)), dtype=torch.float32, device=x.device)
    _check(_timed("tn_gemm", (n, kx, ky, batch), lambda: _lib.bot_tn_gemm_f32(
        x.data_ptr(), _ld(x), y.data_ptr(), _ld(y), n, kx, ky, out.data_ptr(), _ld(out), int(transpose_out), batch, sx, sy, so,
        ws.data_ptr(),
        _stream())), "tn_gemm")
    return out


def tn_narrow(x, y, out, transpose_out=False):
    """out[kx, ky] = x[n, kx]^T y[n, ky] for a handful of x columns (kx <= 32, ky <= 256), transpose_out: out[ky, kx] (include/bot_gnn.h
    bot_tn_narrow_f32: fp32 FMAs, deterministic).  x, y, out: fp32 row-major views with unit column stride."""
    _dev(x, y, out)
    _f32(x, "x"), _f32(y, "y"), _f32(out, "out")
    n, kx, ky = x.shape[0], x.shape[1], y.shape[1]
    assert y.shape[0] == n and out.shape == ((ky, kx) if transpose_out else (kx, ky))
    if x.stride(1) != 1 or y.stride(1) != 1 or (out.stride(1) != 1 and out.shape[1] != 1):
        raise BotKernelError("tn_narrow: operands must have unit column stride")
    ws = torch.empty(int(_lib.bot_tn_narrow_workspace_floats(n, kx, ky)), dtype=torch.float32, device=x.device)
    _check(_timed("tn_narrow", (n, kx, ky), lambda: _lib.bot_tn_narrow_f32(
        x.data_ptr(), _ld(x), y.data_ptr(), _ld(y), n, kx, ky, out.data_ptr(), _ld(out), int(transpose_out), ws.data_ptr(), _stream())), "tn_narrow")
    return out


def colsum(x):
    """Per-column sum of x [n,F] -> [F] (two-stage, finished in double)."""
    _dev(x)
    x = _mat(x, "x")
    n, F = x.shape
    out = torch.empty(F, dtype=torch.float32, device=x.device)
    _check(_lib.bot_colsum_f32(x.data_ptr(), x.stride(0), n, F, out.data_ptr(), _bn_ws(F, x.device).data_ptr(), _stream()), "colsum")
    return out


def _written(*ts):
    """The library wrote these tensors through raw pointers: move their autograd version counters, as an in-place torch op
    would, so that anything keyed on `_version` (the inference-path caches of bot_amd.nn.fused, saved-tensor checks) sees it."""
    ts = [t for t in ts if t is not None]
    if ts:
        torch._C._increment_version(ts)


def bn_stats(x, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None):
    """Training-mode statistics step of nn.BatchNorm1d over the rows of x [n,F] in one call: returns (mean, invstd) and updates
    the running statistics / step counter in place (include/bot_gnn.h bot_bn_stats_f32)."""
    _dev(x, running_mean, running_var)
    x = _mat(x, "x")
    n, F = x.shape
    mean = torch.empty(F, dtype=torch.float32, device=x.device)
    invstd = torch.empty(F, dtype=torch.float32, device=x.device)
    _check(_lib.bot_bn_stats_f32(x.data_ptr(), x.stride(0), n, F, float(eps), float(momentum), mean.data_ptr(), invstd.data_ptr(),
                                 _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _bn_ws(F, x.device).data_ptr(),
                                 _stream()), "bn_stats")
    _written(running_mean, running_var, num_batches_tracked)
    return mean, invstd


def bn_stats_halves(x, eps, momentum, running_mean, running_var, num_batches_tracked, weight, bias, p):
    """bn_stats plus hscale [2] = (s, 1/s) bounding the epilogue's output (include/bot_gnn.h bot_bn_stats_halves_f32)."""
    _dev(x, running_mean, running_var, weight, bias)
    x = _mat(x, "x")
    n, F = x.shape
    mean = torch.empty(F, dtype=torch.float32, device=x.device)
    invstd = torch.empty(F, dtype=torch.float32, device=x.device)
    hscale = torch.empty(2, dtype=torch.float32, device=x.device)
    _check(_lib.bot_bn_stats_halves_f32(x.data_ptr(), x.stride(0), n, F, float(eps), float(momentum), mean.data_ptr(), invstd.data_ptr(),
                                        _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(weight), _ptr(bias),
                                        float(p), hscale.data_ptr(), _bn_ws(F, x.device).data_ptr(), _stream()), "bn_stats_halves")
    _written(running_mean, running_var, num_batches_tracked)
    return mean, invstd, hscale


def bn_stats_halves_partials(part, minmax, pivot, n, eps, momentum, running_mean, running_var, num_batches_tracked, weight, bias, p):
    """bn_stats_halves from column partials a producer of x delivered (gemm_halves3_nt_grouped `stats`) instead of a pass over x
    (include/bot_gnn.h bot_bn_stats_halves_partials_f32): -> (mean, invstd, hscale)."""
    _dev(part, minmax, pivot, running_mean, running_var, weight, bias)
    nblk, _, F = part.shape
    assert pivot.shape == (nblk, F) and minmax.shape == part.shape and part.is_contiguous() and minmax.is_contiguous() and pivot.is_contiguous()
    mean = torch.empty(F, dtype=torch.float32, device=part.device)
    invstd = torch.empty(F, dtype=torch.float32, device=part.device)
    hscale = torch.empty(2, dtype=torch.float32, device=part.device)
    ws = torch.empty(F, dtype=torch.float32, device=part.device)
    _check(_lib.bot_bn_stats_halves_partials_f32(part.data_ptr(), minmax.data_ptr(), int(nblk), pivot.data_ptr(), int(n), int(F), float(eps), float(momentum),
                                                 mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                                                 _ptr(weight), _ptr(bias), float(p), hscale.data_ptr(), ws.data_ptr(), _stream()), "bn_stats_halves_partials")
    _written(running_mean, running_var, num_batches_tracked)
    return mean, invstd, hscale


def bn_act_fwd(x, mean, invstd, weight, bias, relu, p, seed, halves=None, want_y=True, out=None):
    """y = dropout_p(relu?((x - mean) * invstd * weight + bias)); Philox mask from `seed`.
    halves = (hscale [2], piece[, pieces]): also returns y's fp16 halves [n, pieces * piece] scaled by hscale[0] -> (y, buf); pieces 3 (default):
    [h1 | h1 | 2^11 h2], 2: [h1 | 2^11 h2].
    want_y=False (with halves): only the halves are written; the returned y is None.
    `out` may be a row-strided [n,F] view that receives y."""
    _dev(x, mean, invstd)
    x = _mat(x, "x")
    n, F = x.shape
    assert out is None or (want_y and out.shape == (n, F) and out.stride(1) == 1 and out.dtype == torch.float32)
    if halves is not None:
        hscale, piece = halves[:2]
        pieces = halves[2] if len(halves) > 2 else 3
        y = (out if out is not None else torch.empty((n, F), dtype=torch.float32, device=x.device)) if want_y else None
        buf = torch.empty((n, pieces * piece), dtype=torch.float16, device=x.device)
        _check(_timed("bn_act_fwd", (F,), lambda: _lib.bot_bn_act_fwd_halves_f32(
            x.data_ptr(), x.stride(0), n, F, mean.data_ptr(), invstd.data_ptr(), _ptr(weight), _ptr(bias), int(relu), float(p),
            int(seed), _seed_off(p), _ptr(y), y.stride(0) if y is not None else F, hscale.data_ptr(), buf.data_ptr(), buf.stride(0), piece, pieces,
            _stream())),
            "bn_act_fwd_halves")
        return y, buf
    y = out if out is not None else torch.empty((n, F), dtype=torch.float32, device=x.device)
    _check(_timed("bn_act_fwd", (F,), lambda: _lib.bot_bn_act_fwd_f32(
        x.data_ptr(), x.stride(0), n, F, mean.data_ptr(), invstd.data_ptr(), _ptr(weight), _ptr(bias), int(relu), float(p),
        int(seed), _seed_off(p), y.data_ptr(), y.stride(0), _stream())), "bn_act_fwd")
    return y


def bn_act_bwd_reduce(dy, x, mean, invstd, weight, bias, relu, p, seed, want_max=False):
    """Column sums (sum_g, sum_gx) of the masked upstream gradient and of g * xhat.  want_max: also the column maxima of |g| and |xhat|,
    left in the returned workspace for bn_bwd_bound -> (sum_g, sum_gx, workspace)."""
    _dev(dy, x)
    dy, x = _mat(dy, "dy"), _mat(x, "x")
    n, F = x.shape
    sg = torch.empty(F, dtype=torch.float32, device=x.device)
    sgx = torch.empty(F, dtype=torch.float32, device=x.device)
    ws = _bn_ws(F, x.device)
    fn = _lib.bot_bn_act_bwd_reduce_max_f32 if want_max else _lib.bot_bn_act_bwd_reduce_f32
    _check(fn(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), n, F, mean.data_ptr(), invstd.data_ptr(), _ptr(weight), _ptr(bias), int(relu),
              float(p), int(seed), _seed_off(p), sg.data_ptr(), sgx.data_ptr(), ws.data_ptr(), _stream()), "bn_act_bwd_reduce")
    return (sg, sgx, ws) if want_max else (sg, sgx)


def bn_bwd_bound(ws, n, sum_g, sum_gx, total_count, weight, invstd, slots):
    """max |dx| of the BatchNorm backward bounded from the reduce pass's column maxima (`ws` of bn_act_bwd_reduce(want_max=True)) and the
    FINAL column sums (None: eval statistics), folded into the by-product `slots` (bot_bn_bwd_bound_f32)."""
    _dev(ws, invstd, slots)
    F = invstd.shape[0]
    _check(_lib.bot_bn_bwd_bound_f32(F, n, ws.data_ptr(), _ptr(sum_g), _ptr(sum_gx), float(total_count), _ptr(weight), invstd.data_ptr(), slots.data_ptr(),
                                     _stream()), "bn_bwd_bound")
    return slots


def bn_act_bwd_apply_halves(dy, x, mean, invstd, weight, bias, relu, p, seed, sum_g, sum_gx, total_count, hscale, hout, hD, hDP, out=None, h2_off=None):
    """bn_act_bwd_apply writing dx as the LEFT halves operand `hout` [n, 2 * (F / hD) * hDP] = [h1 | 2^11 h2] of hscale[0] * dx, the columns in
    blocks of hD every hDP (padding columns untouched); `out`: optionally dx in fp32 as well (bot_bn_act_bwd_apply_halves_f32)."""
    _dev(dy, x, hout, hscale)
    dy, x = _mat(dy, "dy"), _mat(x, "x")
    n, F = x.shape
    if h2_off is None:
        h2_off = (F // hD) * hDP
        assert hout.shape == (n, 2 * h2_off)
    else:       # `hout`: a column range of a wider operand (its first column = the block's first), the second half h2_off columns behind
        assert hout.shape[0] == n and hout.stride(0) >= h2_off + (F // hD) * hDP
    assert hout.dtype == torch.float16 and hout.stride(1) == 1
    assert out is None or (out.stride(1) == 1 and out.dtype == torch.float32)
    _check(_lib.bot_bn_act_bwd_apply_halves_f32(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), n, F, mean.data_ptr(), invstd.data_ptr(), _ptr(weight),
                                                _ptr(bias), int(relu), float(p), int(seed), _seed_off(p), _ptr(sum_g), _ptr(sum_gx), float(total_count),
                                                _ptr(out), out.stride(0) if out is not None else 0, hscale.data_ptr(), hout.data_ptr(), hout.stride(0), h2_off,
                                                hD, hDP, _stream()), "bn_act_bwd_apply_halves")
    return hout


def bn_act_bwd_apply(dy, x, mean, invstd, weight, bias, relu, p, seed, sum_g, sum_gx, total_count, out=None, absmax=None):
    """dx of the fused BatchNorm+ReLU+dropout; sum_g/sum_gx None = statistics were constants (eval mode).
    `out` may be a row-strided [n,F] view (e.g. a column slice of a wider gradient buffer).  `absmax`: `absmax_slots()` words that
    receive max|dx| as a by-product."""
    _dev(dy, x)
    dy, x = _mat(dy, "dy"), _mat(x, "x")
    n, F = x.shape
    dx = out if out is not None else torch.empty((n, F), dtype=torch.float32, device=x.device)
    assert dx.stride(1) == 1 and dx.dtype == torch.float32
    _check(_lib.bot_bn_act_bwd_apply_f32(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), n, F, mean.data_ptr(),
                                         invstd.data_ptr(), _ptr(weight), _ptr(bias), int(relu), float(p), int(seed), _seed_off(p),
                                         _ptr(sum_g), _ptr(sum_gx), float(total_count), dx.data_ptr(), dx.stride(0), _ptr(absmax),
                                         _stream()),
           "bn_act_bwd_apply")
    return dx


# ------------------------------------------------------------------------------------------------ fused edge MLP (ogbn-proteins)
def edge_mlp_supported(I, J, H):
    return I == 8 and J == 16 and 1 <= H <= 8


def random_keep(n, n_keep, seed, device):
    """uint8 [n] mask of a uniformly random subset of exactly n_keep elements (the edge-drop mask), a pure function of
    (n, n_keep, seed)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise BotKernelError("random_keep: the HIP kernels need a GPU device")
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    ws = torch.empty(int(_lib.bot_random_keep_workspace_bytes()), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _check(_lib.bot_random_keep_u8(n, n_keep, seed & 0xFFFFFFFFFFFFFFFF, keep.data_ptr(), ws.data_ptr(), _stream()), "random_keep")
    return keep


def _count_scan_fill(seeds, count, fill, family, k, what):
    """The two neighbour samplers' sequence: `count(n, counts)` launches the per-seed counts, their inclusive scan gives the
    offsets, ONE device->host read takes the total, then `fill(n, offsets, pos)` is launched under `_timed(family, (k,))`.
    Returns (offsets int64 [n_seeds + 1], pos int32 [total])."""
    assert seeds.dtype == torch.int32 and seeds.is_contiguous()
    n = int(seeds.numel())
    dev = seeds.device
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    _check(count(n, counts), what + "_count")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1])
    pos = torch.empty(total, dtype=torch.int32, device=dev)
    _check(_timed(family, (int(k),), lambda: fill(n, offsets, pos)), what)
    return offsets, pos


def sample_neighbors(csc, seeds, k, seed):
    """In-edges of each seed sampled uniformly without replacement (min(deg, k) of them, all for k < 0), as parent CSC positions
    ascending per seed: (offsets int64 [n_seeds+1], positions int32 [offsets[-1]]).  One device->host read (the total)."""
    _dev(csc.indptr, seeds)
    return _count_scan_fill(
        seeds,
        lambda n, counts: _lib.bot_sample_neighbors_count_i32(csc.indptr.data_ptr(), csc.n_rows, _ptr(seeds), n, int(k), _ptr(counts), _stream()),
        lambda n, offsets, pos: _lib.bot_sample_neighbors_i32(csc.indptr.data_ptr(), csc.n_rows, _ptr(seeds), n, int(k), seed & 0xFFFFFFFFFFFFFFFF,
                                                              offsets.data_ptr(), _ptr(pos), _stream()),
        "sample", k, "sample_neighbors")


class PreparedWeights:
    """Edge weights made ready for weighted sampling (bot_sample_weights_prepare_f32): the per-row inclusive prefix of the
    quantised weights, uint64 in CSC position order (kept as int64 [E]; 8 B per edge), and the positive-weight count per row."""

    def __init__(self, prefix, n_pos):
        self.prefix, self.n_pos = prefix, n_pos


def sample_weights_prepare(csc, w):
    """Quantise and scan per-edge weights `w` (float32 [E] or [E, 1], edge-id order, on the CSC's device) for
    sample_neighbors_weighted.  A negative, NaN or infinite weight raises ValueError.  One device->host read (the error flag)."""
    _dev(csc.indptr, w)
    _f32(w, "edge weights")
    E = int(csc.indices.numel())
    if not (w.dim() == 1 or (w.dim() == 2 and w.shape[1] == 1)) or w.shape[0] != E:
        raise ValueError(f"edge weights must be [E] or [E, 1] with E = {E}, got {tuple(w.shape)}")
    w = w.reshape(-1).contiguous()
    dev = w.device
    prefix = torch.empty(E, dtype=torch.int64, device=dev)
    n_pos = torch.empty(csc.n_rows, dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    rc = _lib.bot_sample_weights_prepare_f32(csc.indptr.data_ptr(), csc.eid.data_ptr(), csc.n_rows, E, w.data_ptr(), prefix.data_ptr(),
                                             n_pos.data_ptr(), flag.data_ptr(), _stream())
    if rc == -2:
        raise ValueError(f"edge weights: {_lib.bot_last_error().decode()}")
    _check(rc, "sample_weights_prepare")
    return PreparedWeights(prefix, n_pos)


def sample_neighbors_weighted(csc, prepared, seeds, k, seed):
    """In-edges of each seed sampled without replacement in proportion to the prepared weights (include/bot_gnn.h: min(n_pos, k)
    of them, every positive-weight edge for k < 0), as parent CSC positions ascending per seed: (offsets int64 [n_seeds+1],
    positions int32 [offsets[-1]]).  One device->host read (the total)."""
    _dev(csc.indptr, prepared.prefix, seeds)
    return _count_scan_fill(
        seeds,
        lambda n, counts: _lib.bot_sample_neighbors_weighted_count_i32(prepared.n_pos.data_ptr(), csc.n_rows, _ptr(seeds), n, int(k),
                                                                       _ptr(counts), _stream()),
        lambda n, offsets, pos: _lib.bot_sample_neighbors_weighted_i32(
            csc.indptr.data_ptr(), prepared.prefix.data_ptr(), prepared.n_pos.data_ptr(), csc.n_rows, _ptr(seeds), n, int(k),
            seed & 0xFFFFFFFFFFFFFFFF, offsets.data_ptr(), _ptr(pos), _stream()),
        "sample_weighted", k, "sample_neighbors_weighted")


def _tile_scratch(n_nodes, n_words, dev):
    """The scratch of the scan over the node map (bot_block_mark_i32, bot_saint_nodes_mark_i32): the tile array, int64
    [bot_block_tiles(n_nodes)], and `n_words` zeroed int64 count words that the host reads once."""
    return (torch.empty(max(1, int(_lib.bot_block_tiles(n_nodes))), dtype=torch.int64, device=dev),
            torch.zeros(n_words, dtype=torch.int64, device=dev))


def block_relabel(csc, seeds, pos, node_map):
    """to_block on sampled parent CSC positions: (src_nid int32 [n_src] = seeds then newly reached nodes ascending, local int32 [E]
    block-local source of each sampled edge, parent_eid int32 [E]).  `node_map`: int32 [n_nodes] of -1, left as it was found.
    One device->host read (the number of new sources)."""
    _dev(csc.indptr, seeds, pos, node_map)
    n_seeds, n_pos, n_nodes = int(seeds.numel()), int(pos.numel()), int(node_map.numel())
    dev = seeds.device
    tiles, n_new = _tile_scratch(n_nodes, 1, dev)
    _check(_lib.bot_block_mark_i32(_ptr(seeds), n_seeds, csc.indices.data_ptr(), _ptr(pos), n_pos, node_map.data_ptr(), n_nodes,
                                   tiles.data_ptr(), n_new.data_ptr(), _stream()), "block_mark")
    n_src = n_seeds + int(n_new)
    src_nid = torch.empty(n_src, dtype=torch.int32, device=dev)
    local = torch.empty(n_pos, dtype=torch.int32, device=dev)
    parent_eid = torch.empty(n_pos, dtype=torch.int32, device=dev)
    _check(_lib.bot_block_relabel_i32(_ptr(seeds), n_seeds, csc.indices.data_ptr(), csc.eid.data_ptr(), _ptr(pos), n_pos, node_map.data_ptr(),
                                      n_nodes, tiles.data_ptr(), n_src, _ptr(src_nid), _ptr(local), _ptr(parent_eid), _stream()), "block_relabel")
    return src_nid, local, parent_eid


def node_subgraph(csc, nodes, node_map):
    """The subgraph induced by `nodes` (int32, unique parent ids, numbered in their order) as its CSC: (offsets int64 [n + 1],
    local_src int32 [E_sub], parent_eid int32 [E_sub]); row i = the in-edges of nodes[i] with their source in the set, in parent
    CSC position order (include/bot_gnn.h).  `node_map`: int32 [n_nodes] of -1, left as it was found.  A duplicate or an id out
    of range raises ValueError after the map has been unmarked.  One device->host read (the duplicate count and the edge total
    together)."""
    _dev(csc.indptr, nodes, node_map)
    _i32(nodes, "nodes"), _i32(node_map, "node_map")
    n, n_nodes = int(nodes.numel()), int(node_map.numel())
    dev = nodes.device
    if csc.n_rows != n_nodes:
        raise ValueError(f"node_subgraph takes a square parent: {csc.n_rows} CSC rows, a node map of {n_nodes}")
    if n > n_nodes:
        raise ValueError(f"{n} nodes asked of a graph of {n_nodes}: the set holds a duplicate")
    tail = torch.zeros(n + 2, dtype=torch.int64, device=dev)        # offsets [n + 1], then the duplicate count
    offsets, n_dup = tail[:n + 1], tail[n + 1:]
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if n == 0:
        return offsets, empty, empty.clone()
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    st = _stream()

    def extract():
        rc = _lib.bot_subgraph_mark_i32(nodes.data_ptr(), n, node_map.data_ptr(), n_nodes, n_dup.data_ptr(), st)
        return rc or _lib.bot_subgraph_count_i32(csc.indptr.data_ptr(), csc.indices.data_ptr(), csc.n_rows, nodes.data_ptr(), n,
                                                 node_map.data_ptr(), counts.data_ptr(), st)
    _check(_timed("subgraph", ("count",), extract), "subgraph_mark / subgraph_count")
    torch.cumsum(counts, 0, out=offsets[1:])
    total, bad = (int(x) for x in tail[n:].tolist())                # the one device->host read
    if bad:
        _check(_lib.bot_subgraph_unmark_i32(nodes.data_ptr(), n, node_map.data_ptr(), n_nodes, st), "subgraph_unmark")
        out_of_range, dup = bad >> 32, bad & 0xFFFFFFFF
        raise ValueError(f"node_subgraph: {dup} duplicate and {out_of_range} out-of-range ids among the {n} nodes "
                         f"(ids are unique and in [0, {n_nodes}))")
    local_src = torch.empty(total, dtype=torch.int32, device=dev)
    parent_eid = torch.empty(total, dtype=torch.int32, device=dev)

    def fill():
        rc = 0
        if total:
            rc = _lib.bot_subgraph_fill_i32(csc.indptr.data_ptr(), csc.indices.data_ptr(), csc.eid.data_ptr(), csc.n_rows, nodes.data_ptr(), n,
                                            node_map.data_ptr(), offsets.data_ptr(), local_src.data_ptr(), parent_eid.data_ptr(), st)
        return rc or _lib.bot_subgraph_unmark_i32(nodes.data_ptr(), n, node_map.data_ptr(), n_nodes, st)
    _check(_timed("subgraph", ("fill",), fill), "subgraph_fill / subgraph_unmark")
    return offsets, local_src, parent_eid


def subgraph_tally(csc, nodes, node_map, tally):
    """include/bot_gnn.h bot_subgraph_tally_i32: tally[p] += 1 for every CSC position p of the rows of `nodes` (int32, UNIQUE parent
    ids - not checked here: `saint_nodes` returns distinct ids) whose source is in `nodes` too.  tally: contiguous int32 [nnz], the
    caller's accumulator.  `node_map`: int32 [n_nodes] of -1, left as it was found.  Mark, tally, unmark; no device->host read.
    Returns tally."""
    _dev(csc.indptr, nodes, node_map, tally)
    _i32(nodes, "nodes"), _i32(node_map, "node_map"), _i32(tally, "tally")
    n, n_nodes = int(nodes.numel()), int(node_map.numel())
    if csc.n_rows != n_nodes:
        raise ValueError(f"subgraph_tally takes a square parent: {csc.n_rows} CSC rows, a node map of {n_nodes}")
    if tally.dim() != 1 or int(tally.numel()) != csc.nnz:
        raise BotKernelError(f"subgraph_tally: tally must be int32 [{csc.nnz}], got {tuple(tally.shape)}")
    if n > n_nodes:
        raise ValueError(f"{n} nodes asked of a graph of {n_nodes}: the set holds a duplicate")
    if n == 0 or csc.nnz == 0:
        return tally
    n_dup = torch.empty(1, dtype=torch.int64, device=nodes.device)      # mark's duplicate count: written, never read
    st = _stream()

    def run():
        rc = _lib.bot_subgraph_mark_i32(nodes.data_ptr(), n, node_map.data_ptr(), n_nodes, n_dup.data_ptr(), st)
        rc = rc or _lib.bot_subgraph_tally_i32(csc.indptr.data_ptr(), csc.indices.data_ptr(), csc.n_rows, nodes.data_ptr(), n,
                                               node_map.data_ptr(), tally.data_ptr(), st)
        return rc or _lib.bot_subgraph_unmark_i32(nodes.data_ptr(), n, node_map.data_ptr(), n_nodes, st)
    _check(_timed("subgraph", ("tally",), run), "subgraph_mark / subgraph_tally / subgraph_unmark")
    return tally


def saint_walk(csc, nids, n_roots, length, root_mode, seed):
    """include/bot_gnn.h bot_saint_walk_i32: trace int32 [n_roots, length + 1], walk i from a root drawn from `nids` (int32, or None =
    every node; root_mode 1: in proportion to out-degree) along uniformly drawn in-edges.  No device->host read."""
    _dev(csc.indptr, nids)
    _i32(nids, "nids")
    n_roots, length = int(n_roots), int(length)
    if n_roots < 0 or length < 0:
        raise ValueError(f"saint_walk: n_roots={n_roots} length={length}")
    trace = torch.empty((n_roots, length + 1), dtype=torch.int32, device=csc.indptr.device)
    _check(_timed("saint_walk", (n_roots, length), lambda: _lib.bot_saint_walk_i32(
        csc.indptr.data_ptr(), csc.indices.data_ptr(), csc.n_rows, int(csc.indices.numel()), _ptr(nids), 0 if nids is None else int(nids.numel()),
        n_roots, length, int(root_mode), seed & 0xFFFFFFFFFFFFFFFF, trace.data_ptr(), _stream())), "saint_walk")
    return trace


def saint_nodes(trace, node_map):
    """The distinct entries of `trace` (int32, any shape) in ascending id, int32 [n] (include/bot_gnn.h bot_saint_nodes_*_i32).
    `node_map`: int32 [n_nodes] of -1, left as it was found.  One device->host read (the count; with it the number of entries
    outside [0, n_nodes), which raises ValueError)."""
    _dev(trace, node_map)
    _i32(trace, "trace"), _i32(node_map, "node_map")
    n_trace, n_nodes = int(trace.numel()), int(node_map.numel())
    dev = trace.device
    tiles, n_out = _tile_scratch(n_nodes, 2, dev)
    st = _stream()
    _check(_timed("saint_nodes", ("mark",), lambda: _lib.bot_saint_nodes_mark_i32(
        _ptr(trace), n_trace, node_map.data_ptr(), n_nodes, tiles.data_ptr(), n_out.data_ptr(), st)), "saint_nodes_mark")
    try:
        n, bad = (int(v) for v in n_out.tolist())                   # the one device->host read
        nodes = torch.empty(n, dtype=torch.int32, device=dev)
    except BaseException:
        node_map.fill_(-1)                                          # the map holds -2 marks: never leave them to the next caller
        raise
    _check(_timed("saint_nodes", ("list",), lambda: _lib.bot_saint_nodes_list_i32(
        node_map.data_ptr(), n_nodes, tiles.data_ptr(), n, _ptr(nodes), st)), "saint_nodes_list")
    if bad:
        raise ValueError(f"saint_nodes: {bad} entries of the trace lie outside [0, {n_nodes})")
    return nodes


def rocauc_counts(pred, codes, groups, n_groups):
    """include/bot_gnn.h bot_rocauc_f32: (out int64 [G, T, 3] = (n_pos, n_neg, 2U) per group and task, nan_count int64 [1]).
    pred float32 [n, T] (unit inner stride), codes int8 [n, T] (1 / 0 / anything else = ignored), groups int8 [n] or None.
    Allocates the workspace; no device->host read."""
    _dev(pred, codes, groups)
    _f32(pred, "pred")
    if pred.dim() != 2 or codes.shape != pred.shape or codes.dtype != torch.int8:
        raise BotKernelError(f"rocauc_counts: pred [n, T] float32 and codes [n, T] int8, got {tuple(pred.shape)} and {tuple(codes.shape)} {codes.dtype}")
    n, T = int(pred.shape[0]), int(pred.shape[1])
    G = int(n_groups)
    if (pred.stride(1) != 1 and T > 1) or (n > 1 and pred.stride(0) < T):
        pred = pred.contiguous()
    if (codes.stride(1) != 1 and T > 1) or (n > 1 and codes.stride(0) < T):
        codes = codes.contiguous()
    if groups is not None and (groups.dtype != torch.int8 or groups.dim() != 1 or groups.numel() != n or not groups.is_contiguous()):
        raise BotKernelError(f"rocauc_counts: groups must be contiguous int8 [{n}]")
    size = int(_lib.bot_rocauc_workspace_bytes(n, T, G))
    out = torch.zeros((max(G, 0), T, 3), dtype=torch.int64, device=pred.device)
    nan_count = torch.zeros(1, dtype=torch.int64, device=pred.device)
    ws = torch.empty(max(size, 8) // 8 + 1, dtype=torch.int64, device=pred.device) if n > 0 else None
    _check(_timed("rocauc", (n, T, G), lambda: _lib.bot_rocauc_f32(
        pred.data_ptr(), _ld(pred) if n > 0 else T, codes.data_ptr(), _ld(codes) if n > 0 else T, _ptr(groups), n, T, G, out.data_ptr(),
        nan_count.data_ptr(), _ptr(ws), 0 if ws is None else ws.numel() * 8, _stream())), "rocauc")
    return out, nan_count


def propagate_step(d, y, y0, out, alpha, beta, src_scale, dst_scale, lo, hi, fixed=None, row_abs=None, out_scale=None, partial=None, ew=None):
    """include/bot_gnn.h bot_propagate_step_f32 - with `ew` (contiguous float32 [nnz], CSC position order: every term of the sum times
    ew[k]) bot_propagate_step_w_f32 - on the square direction `d`:
    out[v] = fixed[v] ? y0[v] : clamp(alpha * dst_scale[v] * sum_k src_scale[u_k] * y[u_k] + beta * y0[v], lo, hi);  row_abs[v] = sum |out[v]|;
    with out_scale the row is stored as out_scale[v] * out[v] (the next sweep's pre-scaled iterate, which then takes src_scale=None).
    y, y0, out: float32 [n, C] with unit inner stride (any row stride), out a buffer of its own; src_scale / dst_scale / out_scale / row_abs:
    contiguous float32 [n] or None; fixed: contiguous uint8 [n] or None; partial: the long rows' workspace (allocated when not given).  Returns out."""
    _dev(y, y0, out, src_scale, dst_scale, fixed, row_abs, out_scale, d.indptr)
    n = d.n_rows
    for t, name in ((y, "y"), (y0, "y0"), (out, "out")):
        _f32(t, name)
        if t.dim() != 2 or t.shape[0] != n or t.shape[1] != y.shape[1] or (t.shape[1] > 1 and t.stride(1) != 1):
            raise BotKernelError(f"propagate_step: {name} must be [{n}, C] with unit inner stride, got {tuple(t.shape)} strides {tuple(t.stride())}")
    C = int(y.shape[1])
    for t, name in ((src_scale, "src_scale"), (dst_scale, "dst_scale"), (row_abs, "row_abs"), (out_scale, "out_scale")):
        if t is not None and (_f32(t, name).dim() != 1 or t.numel() != n or not t.is_contiguous()):
            raise BotKernelError(f"propagate_step: {name} must be contiguous float32 [{n}]")
    if fixed is not None and (fixed.dtype != torch.uint8 or fixed.dim() != 1 or fixed.numel() != n or not fixed.is_contiguous()):
        raise BotKernelError(f"propagate_step: fixed must be contiguous uint8 [{n}]")
    if d.n_long and partial is None:
        partial = torch.empty(d.n_slots * C, dtype=torch.float32, device=y.device)
    ld = lambda t: _ld(t) if n > 0 else C
    if ew is not None:
        _dev(ew, y)
        if _f32(ew, "ew").dim() != 1 or ew.numel() != d.nnz or not ew.is_contiguous():
            raise BotKernelError(f"propagate_step: ew must be contiguous float32 [{d.nnz}]")
        _check(_timed("propagate_step", (C, fixed is not None, row_abs is not None, "ew"), lambda: _lib.bot_propagate_step_w_f32(
            d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
            y.data_ptr(), ld(y), y0.data_ptr(), ld(y0), out.data_ptr(), ld(out), C, float(alpha), float(beta), _ptr(src_scale), _ptr(dst_scale),
            float(lo), float(hi), _ptr(fixed), _ptr(row_abs), _ptr(out_scale), _ptr(partial), ew.data_ptr(), _stream())), "propagate_step_w")
        return out
    _check(_timed("propagate_step", (C, fixed is not None, row_abs is not None), lambda: _lib.bot_propagate_step_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        y.data_ptr(), ld(y), y0.data_ptr(), ld(y0), out.data_ptr(), ld(out), C, float(alpha), float(beta), _ptr(src_scale), _ptr(dst_scale),
        float(lo), float(hi), _ptr(fixed), _ptr(row_abs), _ptr(out_scale), _ptr(partial), _stream())), "propagate_step")
    return out


def appnp_step(d, y, out, a, b=0.0, y0=None, src_scale=None, dst_scale=None, out_scale=None, acc_in=None, acc_out=None, ew=None, pos=None,
               p=0.0, seed=0, step=0, partial=None):
    """include/bot_gnn.h bot_appnp_step_f32 on the square direction `d`:
    o[v] = a * dst_scale[v] * sum_k src_scale[u_k] * ew[k] * m_k * y[u_k] + b * y0[v];  acc_out[v] = acc_in[v] + o[v];  out[v] = out_scale[v] * o[v],
    m_k the step's edge-drop factor of position pos[k] (pos None: k), regenerated from (seed, step): 1 / (1 - p) or 0 (p == 0: 1).
    y, y0, out, acc_in, acc_out: float32 [n, C] with unit inner stride (any row stride), out and acc_out buffers other than y; the scales:
    contiguous float32 [n] or None; ew: contiguous float32 [nnz] and pos: contiguous int32 [nnz] in `d`'s position order; partial: the long
    rows' workspace (allocated when not given).  Returns out."""
    _dev(y, y0, out, src_scale, dst_scale, out_scale, acc_in, acc_out, ew, pos, d.indptr)
    n = d.n_rows
    if y.dim() != 2:
        raise BotKernelError(f"appnp_step: y must be [{n}, C], got {tuple(y.shape)}")
    C = int(y.shape[1])
    for t, name in ((y, "y"), (y0, "y0"), (out, "out"), (acc_in, "acc_in"), (acc_out, "acc_out")):
        if t is not None:
            _rows2(t, n, C, name, "appnp_step")
    for t, name in ((src_scale, "src_scale"), (dst_scale, "dst_scale"), (out_scale, "out_scale")):
        if t is not None and (_f32(t, name).dim() != 1 or t.numel() != n or not t.is_contiguous()):
            raise BotKernelError(f"appnp_step: {name} must be contiguous float32 [{n}]")
    if ew is not None and (_f32(ew, "ew").dim() != 1 or ew.numel() != d.nnz or not ew.is_contiguous()):
        raise BotKernelError(f"appnp_step: ew must be contiguous float32 [{d.nnz}]")
    if pos is not None and (_i32(pos, "pos").dim() != 1 or pos.numel() != d.nnz):
        raise BotKernelError(f"appnp_step: pos must be contiguous int32 [{d.nnz}]")
    if d.n_long and partial is None:
        partial = torch.empty(d.n_slots * C, dtype=torch.float32, device=y.device)
    ld = lambda t: C if (t is None or n == 0) else _ld(t)
    _check(_timed("appnp_step", (C, ew is not None, float(p) > 0, acc_out is not None), lambda: _lib.bot_appnp_step_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        y.data_ptr(), ld(y), _ptr(y0), ld(y0), out.data_ptr(), ld(out), C, float(a), float(b), _ptr(src_scale), _ptr(dst_scale),
        _ptr(out_scale), _ptr(acc_in), ld(acc_in), _ptr(acc_out), ld(acc_out), _ptr(partial), _ptr(ew), _ptr(pos), float(p),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), _stream())), "appnp_step")
    return out


def _rows2(t, n, F, name, what, dtype=torch.float32):
    """A [n, F] matrix of `dtype` with unit inner stride (any row stride) -> its row stride."""
    if t.dtype != dtype:
        raise BotKernelError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] != n or t.shape[1] != F or (F > 1 and t.stride(1) != 1):
        raise BotKernelError(f"{what}: {name} must be [{n}, {F}] with unit inner stride, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return _ld(t) if n > 0 else F


def spmm_max(d, x, relu=False, out=None, arg=None, workspace=None):
    """include/bot_gnn.h bot_spmm_max_f32 on the direction `d`: out[r, f] = max_k x[indices[k], f], arg[r, f] = the smallest position k
    that attains it (-1 on an empty row); relu: out = max(out, 0) and arg = -1 where the max is <= 0.  x: float32 [n_src, F] with unit
    inner stride (any row stride); out float32 / arg int32 [n_rows, F] likewise (allocated when not given); workspace: the long rows'
    2 * n_slots * F words (allocated when not given).  Returns (out, arg)."""
    _dev(x, out, arg, d.indptr)
    _f32(x, "x")
    if x.dim() != 2 or x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise BotKernelError(f"spmm_max: x must be [n_src, F >= 1] with unit inner stride, got {tuple(x.shape)} strides {tuple(x.stride())}")
    n, F = d.n_rows, int(x.shape[1])
    if out is None:
        out = torch.empty((n, F), dtype=torch.float32, device=x.device)
    if arg is None:
        arg = torch.empty((n, F), dtype=torch.int32, device=x.device)
    ldx = _ld(x) if x.shape[0] > 0 else F
    ldo, lda = _rows2(out, n, F, "out", "spmm_max"), _rows2(arg, n, F, "arg", "spmm_max", torch.int32)
    if d.n_long and workspace is None:
        workspace = torch.empty(2 * d.n_slots * F, dtype=torch.float32, device=x.device)
    _check(_timed("spmm_max", (F, bool(relu)), lambda: _lib.bot_spmm_max_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, x.data_ptr(), ldx, F, int(bool(relu)), out.data_ptr(), ldo, arg.data_ptr(), lda, _ptr(workspace), _stream())), "spmm_max")
    return out, arg


def spmm_max_bwd(d_t, pos, dout, arg, out=None, partial=None):
    """include/bot_gnn.h bot_spmm_max_bwd_f32 on the transposed direction `d_t` (rows = sources): dx[u, f] = the sum of dout[v, f] over the
    out-edges u -> v whose position pos[j] is arg[v, f].  pos: contiguous int32 [nnz] (Graph.csr2csc); dout float32 / arg int32
    [n_dst, F] with unit inner stride (any row stride); out: float32 [n_rows, F] (allocated when not given).  Returns dx."""
    _dev(dout, arg, pos, out, d_t.indptr)
    _i32(pos, "pos")
    if pos.numel() != d_t.nnz:
        raise BotKernelError(f"spmm_max_bwd: pos holds {pos.numel()} positions, the direction {d_t.nnz}")
    if dout.dim() != 2 or dout.shape[1] < 1:
        raise BotKernelError(f"spmm_max_bwd: dout must be [n_dst, F >= 1], got {tuple(dout.shape)}")
    n, F, n_dst = d_t.n_rows, int(dout.shape[1]), int(dout.shape[0])
    ldd, lda = _rows2(dout, n_dst, F, "dout", "spmm_max_bwd"), _rows2(arg, n_dst, F, "arg", "spmm_max_bwd", torch.int32)
    if out is None:
        out = torch.empty((n, F), dtype=torch.float32, device=dout.device)
    ldx = _rows2(out, n, F, "out", "spmm_max_bwd")
    if d_t.n_long and partial is None:
        partial = torch.empty(d_t.n_slots * F, dtype=torch.float32, device=dout.device)
    _check(_timed("spmm_max_bwd", (F,), lambda: _lib.bot_spmm_max_bwd_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, pos.data_ptr(), dout.data_ptr(), ldd, arg.data_ptr(), lda, F, out.data_ptr(), ldx, _ptr(partial), _stream())),
        "spmm_max_bwd")
    return out


PNA_CODES = {"mean": 0, "sum": 1, "max": 2, "min": 3, "std": 4, "var": 5}      # include/bot_gnn.h "PNA aggregation"


def _pna_codes(aggregators):
    """The aggregator names as the HOST int32 array the entry points read (kept alive by the caller for the call)."""
    return (ctypes.c_int32 * len(aggregators))(*[PNA_CODES[a] for a in aggregators])


def pna_record_sections(aggregators):
    """How many F-wide sections the backward's record of these aggregators has (include/bot_gnn.h bot_pna_bwd_prep_f32)."""
    s = set(aggregators)
    return bool(s & {"mean", "sum"}) + 2 * bool(s & {"std", "var"}) + 2 * ("max" in s) + 2 * ("min" in s)


def _pna_scale(scale, n, dev_like, what):
    if scale is None:
        return 1
    _dev(scale, dev_like)
    if _f32(scale, "scale").dim() != 2 or scale.shape[1] != n or not scale.is_contiguous():
        raise BotKernelError(f"{what}: scale must be contiguous float32 [S, {n}], got {tuple(scale.shape)}")
    return int(scale.shape[0])


def spmm_pna(d, a, b, aggregators, scale=None, tower_width=None, want_saved=False, pivot=True, out=None, saved=None, sarg=None, workspace=None):
    """include/bot_gnn.h bot_spmm_pna_f32 on the direction `d`: the aggregators (names of PNA_CODES) of m_k = a[indices[k]] + b[r] per
    row, each times the rows of `scale` (float32 [S, n_rows], None: one scaler of ones), tower-major in out [n_rows, S*A*F].  a: float32
    [n_src, F], b: float32 [n_rows, F] or None, out likewise - unit inner stride, any row stride (out allocated when not given).
    want_saved (or saved / sarg given): also the backward's saved float32 / sarg int32 [n_rows, 2 F].  pivot=False: the pivot is a's row 0
    (measurements).  workspace: the long rows' 6 * n_slots * F words (allocated when not given).  Returns (out, saved, sarg)."""
    _dev(a, b, out, saved, sarg, d.indptr)
    _f32(a, "a")
    if a.dim() != 2 or a.shape[1] < 1 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise BotKernelError(f"spmm_pna: a must be [n_src, F >= 1] with unit inner stride, got {tuple(a.shape)} strides {tuple(a.stride())}")
    n, F = d.n_rows, int(a.shape[1])
    Ft = F if tower_width is None else int(tower_width)
    S, A = _pna_scale(scale, n, a, "spmm_pna"), len(aggregators)
    W = S * A * F
    codes = _pna_codes(aggregators)
    if out is None:
        out = torch.empty((n, W), dtype=torch.float32, device=a.device)
    if (want_saved or sarg is not None) and saved is None:
        saved = torch.empty((n, 2 * F), dtype=torch.float32, device=a.device)
    if saved is not None and sarg is None:
        sarg = torch.empty((n, 2 * F), dtype=torch.int32, device=a.device)
    lda = _ld(a) if a.shape[0] > 0 else F
    ldb = 0 if b is None else _rows2(b, n, F, "b", "spmm_pna")
    ldo = _rows2(out, n, W, "out", "spmm_pna")
    lds = 0 if saved is None else _rows2(saved, n, 2 * F, "saved", "spmm_pna")
    ldg = 0 if sarg is None else _rows2(sarg, n, 2 * F, "sarg", "spmm_pna", torch.int32)
    if d.n_long and workspace is None:
        workspace = torch.empty(6 * d.n_slots * F, dtype=torch.float32, device=a.device)
    _check(_timed("spmm_pna", (F, Ft, S, A), lambda: _lib.bot_spmm_pna_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, a.data_ptr(), lda, _ptr(b), ldb, F, Ft, ctypes.addressof(codes), A, _ptr(scale), S, int(bool(pivot)), out.data_ptr(), ldo,
        _ptr(saved), lds, _ptr(sarg), ldg, _ptr(workspace), _stream())), "spmm_pna")
    return out, saved, sarg


def pna_bwd_prep(d, dout, aggregators, saved, sarg, scale=None, tower_width=None, want_db=True, db=None, rec=None):
    """include/bot_gnn.h bot_pna_bwd_prep_f32 for the forward direction `d`: dout float32 [n_rows, S*A*F] folded over the scalers into the
    record rec float32 [n_rows, pna_record_sections(aggregators) * F] and db float32 [n_rows, F] (want_db; both allocated when not
    given).  saved / sarg: the forward's.  Returns (rec, db)."""
    _dev(dout, saved, sarg, db, rec, d.indptr)
    n = d.n_rows
    if saved.dim() != 2 or saved.shape[1] % 2:
        raise BotKernelError(f"pna_bwd_prep: saved must be [n_rows, 2 F], got {tuple(saved.shape)}")
    F = int(saved.shape[1]) // 2
    Ft = F if tower_width is None else int(tower_width)
    S, A = _pna_scale(scale, n, dout, "pna_bwd_prep"), len(aggregators)
    codes = _pna_codes(aggregators)
    R = pna_record_sections(aggregators) * F
    if rec is None:
        rec = torch.empty((n, R), dtype=torch.float32, device=dout.device)
    if db is None and want_db:
        db = torch.empty((n, F), dtype=torch.float32, device=dout.device)
    ldd = _rows2(dout, n, S * A * F, "dout", "pna_bwd_prep")
    lds, ldg = _rows2(saved, n, 2 * F, "saved", "pna_bwd_prep"), _rows2(sarg, n, 2 * F, "sarg", "pna_bwd_prep", torch.int32)
    ldb = 0 if db is None else _rows2(db, n, F, "db", "pna_bwd_prep")
    ldr = _rows2(rec, n, R, "rec", "pna_bwd_prep")
    _check(_timed("pna_bwd_prep", (F, Ft, S, A), lambda: _lib.bot_pna_bwd_prep_f32(
        d.indptr.data_ptr(), n, dout.data_ptr(), ldd, _ptr(scale), S, ctypes.addressof(codes), A, F, Ft, saved.data_ptr(), lds, sarg.data_ptr(),
        ldg, _ptr(db), ldb, rec.data_ptr(), ldr, _stream())), "pna_bwd_prep")
    return rec, db


def spmm_pna_bwd(d_t, pos, a, rec, aggregators, out=None, partial=None):
    """include/bot_gnn.h bot_spmm_pna_bwd_f32 on the transposed direction `d_t` (rows = sources): dx[u] = the sum over u's out-edges of
    the destination's record applied to a[u] and the edge's position.  pos: contiguous int32 [nnz] (Graph.csr2csc); a float32
    [n_rows, F]; rec: pna_bwd_prep's; out: float32 [n_rows, F] (allocated when not given).  Returns dx."""
    _dev(a, rec, pos, out, d_t.indptr)
    _i32(pos, "pos")
    if pos.numel() != d_t.nnz:
        raise BotKernelError(f"spmm_pna_bwd: pos holds {pos.numel()} positions, the direction {d_t.nnz}")
    n, F = d_t.n_rows, int(a.shape[1])
    lda = _rows2(a, n, F, "a", "spmm_pna_bwd")
    codes = _pna_codes(aggregators)
    R = pna_record_sections(aggregators) * F
    if rec.dim() != 2:
        raise BotKernelError(f"spmm_pna_bwd: rec must be [n_dst, {R}], got {tuple(rec.shape)}")
    ldr = _rows2(rec, int(rec.shape[0]), R, "rec", "spmm_pna_bwd")
    if out is None:
        out = torch.empty((n, F), dtype=torch.float32, device=a.device)
    ldx = _rows2(out, n, F, "out", "spmm_pna_bwd")
    if d_t.n_long and partial is None:
        partial = torch.empty(d_t.n_slots * F, dtype=torch.float32, device=a.device)
    _check(_timed("spmm_pna_bwd", (F, len(aggregators)), lambda: _lib.bot_spmm_pna_bwd_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, pos.data_ptr(), a.data_ptr(), lda, rec.data_ptr(), ldr, ctypes.addressof(codes), len(aggregators), F, out.data_ptr(), ldx,
        _ptr(partial), _stream())), "spmm_pna_bwd")
    return out


PNA_EDGE_MAX_K = 16         # the widest raw edge feature the PNA edge sweeps take (include/bot_gnn.h)


def _pna_edge_operands(what, d, ef, weight, eperm, F):
    """The per-edge operands of the PNA edge sweeps -> (K, wt): ef float32 contiguous [>= 1 row per position, K], weight float32 [F, K]
    (transposed here to the kernels' [K, F]: K * F floats), eperm contiguous int32 [nnz] or None."""
    _f32(ef, "ef"), _f32(weight, "weight")
    if ef.dim() != 2 or not 1 <= ef.shape[1] <= PNA_EDGE_MAX_K or not ef.is_contiguous():
        raise BotKernelError(f"{what}: ef must be contiguous [E, 1 <= K <= {PNA_EDGE_MAX_K}], got {tuple(ef.shape)} strides {tuple(ef.stride())}")
    K = int(ef.shape[1])
    if tuple(weight.shape) != (F, K):
        raise BotKernelError(f"{what}: weight must be [{F}, {K}], got {tuple(weight.shape)}")
    if eperm is None:
        if ef.shape[0] != d.nnz:
            raise BotKernelError(f"{what}: ef holds {ef.shape[0]} rows, the direction {d.nnz} positions")
    elif _i32(eperm, "eperm").numel() != d.nnz:
        raise BotKernelError(f"{what}: eperm holds {eperm.numel()} positions, the direction {d.nnz}")
    return K, weight.t().contiguous()


def spmm_pna_edge(d, a, b, ef, weight, aggregators, scale=None, tower_width=None, want_saved=False, eperm=None, out=None, saved=None, sarg=None,
                  workspace=None):
    """include/bot_gnn.h bot_spmm_pna_edge_f32 on the direction `d`: `spmm_pna` over the per-edge messages m_k = a[indices[k]] + ef[r] @
    weight.T, r = eperm[k] (contiguous int32 [nnz]; rows of ef, not range-checked) or k, with the split pivot; b enters behind the
    reduce.  ef: contiguous float32 [E, K], K <= 16; weight: float32 [F, K]; the rest as in `spmm_pna`.  Returns (out, saved, sarg)."""
    _dev(a, b, ef, weight, eperm, out, saved, sarg, d.indptr)
    _f32(a, "a")
    if a.dim() != 2 or a.shape[1] < 1 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise BotKernelError(f"spmm_pna_edge: a must be [n_src, F >= 1] with unit inner stride, got {tuple(a.shape)} strides {tuple(a.stride())}")
    n, F = d.n_rows, int(a.shape[1])
    K, wt = _pna_edge_operands("spmm_pna_edge", d, ef, weight, eperm, F)
    Ft = F if tower_width is None else int(tower_width)
    S, A = _pna_scale(scale, n, a, "spmm_pna_edge"), len(aggregators)
    W = S * A * F
    codes = _pna_codes(aggregators)
    if out is None:
        out = torch.empty((n, W), dtype=torch.float32, device=a.device)
    if (want_saved or sarg is not None) and saved is None:
        saved = torch.empty((n, 2 * F), dtype=torch.float32, device=a.device)
    if saved is not None and sarg is None:
        sarg = torch.empty((n, 2 * F), dtype=torch.int32, device=a.device)
    lda = _ld(a) if a.shape[0] > 0 else F
    ldb = 0 if b is None else _rows2(b, n, F, "b", "spmm_pna_edge")
    ldo = _rows2(out, n, W, "out", "spmm_pna_edge")
    lds = 0 if saved is None else _rows2(saved, n, 2 * F, "saved", "spmm_pna_edge")
    ldg = 0 if sarg is None else _rows2(sarg, n, 2 * F, "sarg", "spmm_pna_edge", torch.int32)
    if d.n_long and workspace is None:
        workspace = torch.empty(6 * d.n_slots * F, dtype=torch.float32, device=a.device)
    _check(_timed("spmm_pna_edge", (F, Ft, K, S, A), lambda: _lib.bot_spmm_pna_edge_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, a.data_ptr(), lda, _ptr(b), ldb, F, Ft, ef.data_ptr(), K, _ptr(eperm), wt.data_ptr(), ctypes.addressof(codes), A, _ptr(scale),
        S, out.data_ptr(), ldo, _ptr(saved), lds, _ptr(sarg), ldg, _ptr(workspace), _stream())), "spmm_pna_edge")
    return out, saved, sarg


def spmm_pna_edge_bwd(d_t, pos, a, ef, weight, rec, aggregators, eperm=None, want_dx=True, want_dweight=True, out=None, partial=None,
                      dw_workspace=None):
    """include/bot_gnn.h bot_spmm_pna_edge_bwd_f32 on the transposed direction `d_t` (rows = sources) -> (dx [n_rows, F] or None, dweight
    [F, K] or None): per out-edge dm = the destination's record (pna_bwd_prep's) applied to a[u] + c_e and the edge's position, c_e =
    ef[r] @ weight.T with r = eperm[j] or j (d_t.eid for ef in edge-id order); dx[u] = the sum of dm over the out-edges of u, dweight[f, i]
    = the sum over all edges of ef[r, i] dm[f].  pos: contiguous int32 [nnz] (Graph.csr2csc).  dw_workspace: min(1024, n_items // 16 + 1)
    * K * F floats (allocated when not given)."""
    _dev(a, ef, weight, rec, pos, eperm, out, d_t.indptr)
    _i32(pos, "pos")
    if pos.numel() != d_t.nnz:
        raise BotKernelError(f"spmm_pna_edge_bwd: pos holds {pos.numel()} positions, the direction {d_t.nnz}")
    n, F = d_t.n_rows, int(a.shape[1])
    lda = _rows2(a, n, F, "a", "spmm_pna_edge_bwd")
    K, wt = _pna_edge_operands("spmm_pna_edge_bwd", d_t, ef, weight, eperm, F)
    codes = _pna_codes(aggregators)
    R = pna_record_sections(aggregators) * F
    if rec.dim() != 2:
        raise BotKernelError(f"spmm_pna_edge_bwd: rec must be [n_dst, {R}], got {tuple(rec.shape)}")
    ldr = _rows2(rec, int(rec.shape[0]), R, "rec", "spmm_pna_edge_bwd")
    ldx, dweight, dw_rows = F, None, 0
    if want_dx:
        if out is None:
            out = torch.empty((n, F), dtype=torch.float32, device=a.device)
        ldx = _rows2(out, n, F, "out", "spmm_pna_edge_bwd")
        if d_t.n_long and partial is None:
            partial = torch.empty(d_t.n_slots * F, dtype=torch.float32, device=a.device)
    else:
        out = None
    if want_dweight:
        dweight = torch.empty((F, K), dtype=torch.float32, device=a.device)
        dw_rows = min(1024, d_t.n_items // 16 + 1)
        if dw_workspace is None:
            dw_workspace = torch.empty(dw_rows * K * F, dtype=torch.float32, device=a.device)
        elif dw_workspace.dtype != torch.float32 or not dw_workspace.is_contiguous() or dw_workspace.numel() < dw_rows * K * F:
            raise BotKernelError(f"spmm_pna_edge_bwd: dw_workspace must hold {dw_rows * K * F} contiguous float32")
    _check(_timed("spmm_pna_edge_bwd", (F, K, len(aggregators), want_dx, want_dweight), lambda: _lib.bot_spmm_pna_edge_bwd_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, pos.data_ptr(), a.data_ptr(), lda, ef.data_ptr(), K, _ptr(eperm), wt.data_ptr(), rec.data_ptr(), ldr, ctypes.addressof(codes),
        len(aggregators), F, _ptr(out), ldx, _ptr(partial), _ptr(dweight), _ptr(dw_workspace) if want_dweight else None, dw_rows, _stream())),
        "spmm_pna_edge_bwd")
    return out, dweight


def _beta1(beta, like, what):
    """The one-element float32 device tensor the softmax sweeps read beta from."""
    _dev(beta, like)
    if _f32(beta, "beta").numel() != 1:
        raise BotKernelError(f"{what}: beta must hold one float32, got {tuple(beta.shape)}")
    return beta


def spmm_softmax(d, x, beta, relu=False, eps=0.0, want_q=False, out=None, lse=None, q=None, workspace=None):
    """include/bot_gnn.h bot_spmm_softmax_f32 on the direction `d`: with m = relu ? max(x, 0) + eps : x,  out[r, f] = sum_k a_k m_k,
    a_k = exp(beta m_k - lse[r, f]), lse[r, f] = log sum_k exp(beta m_k) and - with want_q (or q given) - q[r, f] = sum_k a_k m_k^2 over
    the positions k of row r; zeros on an empty row.  x: float32 [n_src, F] with unit inner stride (any row stride); beta: a one-element
    float32 DEVICE tensor (read by the kernel: no host read); out / lse / q float32 [n_rows, F] likewise (allocated when not given);
    workspace: the long rows' (4 if q else 3) * n_slots * F floats (allocated when not given).  Returns (out, lse, q or None)."""
    _dev(x, out, lse, q, d.indptr)
    _f32(x, "x")
    _beta1(beta, x, "spmm_softmax")
    if x.dim() != 2 or x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise BotKernelError(f"spmm_softmax: x must be [n_src, F >= 1] with unit inner stride, got {tuple(x.shape)} strides {tuple(x.stride())}")
    n, F = d.n_rows, int(x.shape[1])
    new = lambda: torch.empty((n, F), dtype=torch.float32, device=x.device)
    out = new() if out is None else out
    lse = new() if lse is None else lse
    if q is None and want_q:
        q = new()
    ldx = _ld(x) if x.shape[0] > 0 else F
    ldo, ldl = _rows2(out, n, F, "out", "spmm_softmax"), _rows2(lse, n, F, "lse", "spmm_softmax")
    ldq = F if q is None else _rows2(q, n, F, "q", "spmm_softmax")
    if d.n_long and workspace is None:
        workspace = torch.empty((3 if q is None else 4) * d.n_slots * F, dtype=torch.float32, device=x.device)
    _check(_timed("spmm_softmax", (F, bool(relu), q is not None), lambda: _lib.bot_spmm_softmax_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, x.data_ptr(), ldx, F, beta.data_ptr(), int(bool(relu)), float(eps), out.data_ptr(), ldo, lse.data_ptr(), ldl, _ptr(q), ldq,
        _ptr(workspace), _stream())), "spmm_softmax")
    return out, lse, q


def spmm_softmax_bwd(d_t, x, beta, relu, eps, dout, out, lse, dx=None, partial=None):
    """include/bot_gnn.h bot_spmm_softmax_bwd_f32 on the transposed direction `d_t` (rows = sources): dx[u, f] = gate * the sum over the
    out-edges u -> v of dout[v, f] exp(beta m_u - lse[v, f]) (1 + beta (m_u - out[v, f])).  x: float32 [n_rows, F]; dout / out / lse: float32
    [n_dst, F], unit inner strides (any row stride); beta as in spmm_softmax; dx: float32 [n_rows, F] (allocated when not given).
    Returns dx."""
    _dev(x, dout, out, lse, dx, d_t.indptr)
    _beta1(beta, x, "spmm_softmax_bwd")
    if dout.dim() != 2 or dout.shape[1] < 1:
        raise BotKernelError(f"spmm_softmax_bwd: dout must be [n_dst, F >= 1], got {tuple(dout.shape)}")
    n, F, n_dst = d_t.n_rows, int(dout.shape[1]), int(dout.shape[0])
    ldx = _rows2(x, n, F, "x", "spmm_softmax_bwd")
    ldd, ldo, ldl = (_rows2(t, n_dst, F, name, "spmm_softmax_bwd") for t, name in ((dout, "dout"), (out, "out"), (lse, "lse")))
    if dx is None:
        dx = torch.empty((n, F), dtype=torch.float32, device=dout.device)
    lddx = _rows2(dx, n, F, "dx", "spmm_softmax_bwd")
    if d_t.n_long and partial is None:
        partial = torch.empty(d_t.n_slots * F, dtype=torch.float32, device=dout.device)
    _check(_timed("spmm_softmax_bwd", (F, bool(relu)), lambda: _lib.bot_spmm_softmax_bwd_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, x.data_ptr(), ldx, beta.data_ptr(), int(bool(relu)), float(eps), dout.data_ptr(), ldd, out.data_ptr(), ldo, lse.data_ptr(),
        ldl, F, dx.data_ptr(), lddx, _ptr(partial), _stream())), "spmm_softmax_bwd")
    return dx


SOFTMAX_EDGE_MAX_K = 16     # the widest raw edge feature the edge sweeps take (include/bot_gnn.h)


def _edge_operands(what, d, ef, weight, bias, eperm, F):
    """The per-edge operands of the edge-feature softmax sweeps -> (K, wt): ef float32 contiguous [>= 1 row per position, K], weight
    float32 [F, K] (transposed here to the kernels' [K, F]: K * F floats), bias float32 [F] or None, eperm contiguous int32 [nnz] or None."""
    _f32(ef, "ef"), _f32(weight, "weight"), _f32(bias, "bias")
    if ef.dim() != 2 or not 1 <= ef.shape[1] <= SOFTMAX_EDGE_MAX_K or not ef.is_contiguous():
        raise BotKernelError(f"{what}: ef must be contiguous [E, 1 <= K <= {SOFTMAX_EDGE_MAX_K}], got {tuple(ef.shape)} strides {tuple(ef.stride())}")
    K = int(ef.shape[1])
    if tuple(weight.shape) != (F, K):
        raise BotKernelError(f"{what}: weight must be [{F}, {K}], got {tuple(weight.shape)}")
    if bias is not None and (tuple(bias.shape) != (F,) or not bias.is_contiguous()):
        raise BotKernelError(f"{what}: bias must be contiguous [{F}], got {tuple(bias.shape)}")
    if eperm is None:
        if ef.shape[0] != d.nnz:
            raise BotKernelError(f"{what}: ef holds {ef.shape[0]} rows, the direction {d.nnz} positions")
    elif _i32(eperm, "eperm").numel() != d.nnz:
        raise BotKernelError(f"{what}: eperm holds {eperm.numel()} positions, the direction {d.nnz}")
    return K, weight.t().contiguous()


def spmm_softmax_edge(d, x, ef, weight, bias, beta, relu=False, eps=0.0, want_q=False, eperm=None, out=None, lse=None, q=None, workspace=None):
    """include/bot_gnn.h bot_spmm_softmax_edge_f32 on the direction `d`: `spmm_softmax` over the per-edge messages of z_k = x[indices[k]] +
    (ef[r] @ weight.T + bias), r = eperm[k] (contiguous int32 [nnz]; rows of ef, not range-checked) or k.  ef: contiguous float32 [E, K],
    K <= 16; weight: float32 [F, K]; bias: float32 [F] or None; the rest as in `spmm_softmax`.  Returns (out, lse, q or None)."""
    _dev(x, ef, weight, bias, eperm, out, lse, q, d.indptr)
    _f32(x, "x")
    _beta1(beta, x, "spmm_softmax_edge")
    if x.dim() != 2 or x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise BotKernelError(f"spmm_softmax_edge: x must be [n_src, F >= 1] with unit inner stride, got {tuple(x.shape)} strides {tuple(x.stride())}")
    n, F = d.n_rows, int(x.shape[1])
    K, wt = _edge_operands("spmm_softmax_edge", d, ef, weight, bias, eperm, F)
    new = lambda: torch.empty((n, F), dtype=torch.float32, device=x.device)
    out = new() if out is None else out
    lse = new() if lse is None else lse
    if q is None and want_q:
        q = new()
    ldx = _ld(x) if x.shape[0] > 0 else F
    ldo, ldl = _rows2(out, n, F, "out", "spmm_softmax_edge"), _rows2(lse, n, F, "lse", "spmm_softmax_edge")
    ldq = F if q is None else _rows2(q, n, F, "q", "spmm_softmax_edge")
    if d.n_long and workspace is None:
        workspace = torch.empty((3 if q is None else 4) * d.n_slots * F, dtype=torch.float32, device=x.device)
    _check(_timed("spmm_softmax_edge", (F, K, bool(relu), q is not None), lambda: _lib.bot_spmm_softmax_edge_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, x.data_ptr(), ldx, F, ef.data_ptr(), K, _ptr(eperm), wt.data_ptr(), _ptr(bias), beta.data_ptr(), int(bool(relu)), float(eps),
        out.data_ptr(), ldo, lse.data_ptr(), ldl, _ptr(q), ldq, _ptr(workspace), _stream())), "spmm_softmax_edge")
    return out, lse, q


def spmm_softmax_edge_bwd(d_t, x, ef, weight, bias, beta, relu, eps, dout, out, lse, eperm=None, want_dx=True, want_dweight=True, dx=None,
                          partial=None, dw_workspace=None):
    """include/bot_gnn.h bot_spmm_softmax_edge_bwd_f32 on the transposed direction `d_t` (rows = sources) -> (dx [n_rows, F] or None,
    dweight [F, K] or None): with z, m of `spmm_softmax_edge` per out-edge (r = eperm[j] or j: d_t.eid for ef in edge-id order), dz = gate
    dout exp(beta m - lse) (1 + beta (m - out)); dx[u] = the sum of dz over the out-edges of u, dweight[f, i] = the sum over all edges of
    ef[r, i] dz[f].  dw_workspace: min(1024, n_items // 16 + 1) * K * F floats (allocated when not given)."""
    _dev(x, ef, weight, bias, eperm, dout, out, lse, dx, d_t.indptr)
    _beta1(beta, x, "spmm_softmax_edge_bwd")
    if dout.dim() != 2 or dout.shape[1] < 1:
        raise BotKernelError(f"spmm_softmax_edge_bwd: dout must be [n_dst, F >= 1], got {tuple(dout.shape)}")
    n, F, n_dst = d_t.n_rows, int(dout.shape[1]), int(dout.shape[0])
    K, wt = _edge_operands("spmm_softmax_edge_bwd", d_t, ef, weight, bias, eperm, F)
    ldx = _rows2(x, n, F, "x", "spmm_softmax_edge_bwd")
    ldd, ldo, ldl = (_rows2(t, n_dst, F, name, "spmm_softmax_edge_bwd") for t, name in ((dout, "dout"), (out, "out"), (lse, "lse")))
    lddx, dweight, dw_rows = F, None, 0
    if want_dx:
        if dx is None:
            dx = torch.empty((n, F), dtype=torch.float32, device=dout.device)
        lddx = _rows2(dx, n, F, "dx", "spmm_softmax_edge_bwd")
        if d_t.n_long and partial is None:
            partial = torch.empty(d_t.n_slots * F, dtype=torch.float32, device=dout.device)
    else:
        dx = None
    if want_dweight:
        dweight = torch.empty((F, K), dtype=torch.float32, device=dout.device)
        dw_rows = min(1024, d_t.n_items // 16 + 1)
        if dw_workspace is None:
            dw_workspace = torch.empty(dw_rows * K * F, dtype=torch.float32, device=dout.device)
        elif dw_workspace.dtype != torch.float32 or not dw_workspace.is_contiguous() or dw_workspace.numel() < dw_rows * K * F:
            raise BotKernelError(f"spmm_softmax_edge_bwd: dw_workspace must hold {dw_rows * K * F} contiguous float32")
    _check(_timed("spmm_softmax_edge_bwd", (F, K, bool(relu), want_dweight), lambda: _lib.bot_spmm_softmax_edge_bwd_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, x.data_ptr(), ldx, ef.data_ptr(), K, _ptr(eperm), wt.data_ptr(), _ptr(bias), beta.data_ptr(), int(bool(relu)), float(eps),
        dout.data_ptr(), ldd, out.data_ptr(), ldo, lse.data_ptr(), ldl, F, _ptr(dx), lddx, _ptr(partial), _ptr(dweight),
        _ptr(dw_workspace) if want_dweight else None, dw_rows, _stream())), "spmm_softmax_edge_bwd")
    return dx, dweight


def _heads3(t, n, H, D, name, what):
    """A float32 [n, H, D] tensor whose rows are H * D contiguous floats (any row stride) -> its row stride."""
    _f32(t, name)
    if t.dim() != 3 or tuple(t.shape) != (n, H, D) or (D > 1 and t.stride(2) != 1) or (H > 1 and t.stride(1) != D):
        raise BotKernelError(f"{what}: {name} must be [{n}, {H}, {D}] with contiguous rows, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return max(int(t.stride(0)), H * D) if n > 1 else H * D


def _gatv2_operands(what, fs, fd, attn, n_src, n_dst):
    if attn.dim() != 2 or attn.shape[0] < 1 or attn.shape[1] < 1 or not attn.is_contiguous():
        raise BotKernelError(f"{what}: attn must be contiguous [H >= 1, D >= 1], got {tuple(attn.shape)}")
    _f32(attn, "attn")
    H, D = int(attn.shape[0]), int(attn.shape[1])
    return H, D, _heads3(fs, n_src, H, D, "fs", what), _heads3(fd, n_dst, H, D, "fd", what)


def _edge_rows(t, E, H, name, what):
    """A float32 [E, H] matrix with unit inner stride -> its row stride."""
    return _rows2(t, E, H, name, what)


def gatv2_logits(d, fs, fd, attn, slope, operm=None, out=None):
    """include/bot_gnn.h bot_gatv2_logits_f32 on the direction `d` (rows = destinations): e[o(k), h] = sum_d attn[h, d] *
    lrelu(fs[indices[k], h, d] + fd[row of k, h, d]) with o(k) = operm[k] (contiguous int32 [nnz]) or k.  fs float32 [n_src, H, D], fd
    float32 [n_rows, H, D] with contiguous rows (any row stride), attn contiguous float32 [H, D]; out: float32 [nnz, H] with unit inner
    stride (allocated when not given).  Returns e."""
    _dev(fs, fd, attn, operm, out, d.indptr)
    H, D, ldfs, ldfd = _gatv2_operands("gatv2_logits", fs, fd, attn, int(fs.shape[0]), d.n_rows)
    if operm is not None and _i32(operm, "operm").numel() != d.nnz:
        raise BotKernelError(f"gatv2_logits: operm holds {operm.numel()} positions, the direction {d.nnz}")
    if out is None:
        out = torch.empty((d.nnz, H), dtype=torch.float32, device=fs.device)
    lde = _edge_rows(out, d.nnz, H, "out", "gatv2_logits")
    _check(_timed("gatv2_logits", (H, D), lambda: _lib.bot_gatv2_logits_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, fs.data_ptr(), ldfs, fd.data_ptr(), ldfd,
        attn.data_ptr(), H, D, float(slope), _ptr(operm), out.data_ptr(), lde, _stream())), "gatv2_logits")
    return out


def gatv2_logits_bwd_dst(d, fs, fd, attn, slope, de, dperm=None, want_dfd=True, want_dattn=True, out=None, workspace=None):
    """include/bot_gnn.h bot_gatv2_logits_bwd_dst_f32 on the direction `d` (rows = destinations) -> (dfd [n_rows, H, D] or None, dattn
    [H, D] or None).  de: float32 [nnz, H] with unit inner stride, read at row dperm[k] (contiguous int32 [nnz]) or k; out: the dfd
    buffer (contiguous rows, any row stride; allocated when not given); workspace: bot_gatv2_logits_bwd_dst_workspace_floats floats
    (allocated when not given)."""
    _dev(fs, fd, attn, de, dperm, out, d.indptr)
    n = d.n_rows
    H, D, ldfs, ldfd = _gatv2_operands("gatv2_logits_bwd_dst", fs, fd, attn, int(fs.shape[0]), n)
    ldde = _edge_rows(de, d.nnz, H, "de", "gatv2_logits_bwd_dst")
    if dperm is not None and _i32(dperm, "dperm").numel() != d.nnz:
        raise BotKernelError(f"gatv2_logits_bwd_dst: dperm holds {dperm.numel()} positions, the direction {d.nnz}")
    dfd = dattn = None
    lddfd = H * D
    if want_dfd:
        dfd = torch.empty((n, H, D), dtype=torch.float32, device=fs.device) if out is None else out
        lddfd = _heads3(dfd, n, H, D, "out", "gatv2_logits_bwd_dst")
    if want_dattn:
        dattn = (torch.empty if n > 0 else torch.zeros)((H, D), dtype=torch.float32, device=fs.device)
    if workspace is None and (want_dattn or (want_dfd and d.n_long)):
        workspace = torch.empty(max(1, int(_lib.bot_gatv2_logits_bwd_dst_workspace_floats(d.n_items, d.n_slots, H, D))), dtype=torch.float32,
                                device=fs.device)
    _check(_timed("gatv2_logits_bwd_dst", (H, D, want_dfd, want_dattn), lambda: _lib.bot_gatv2_logits_bwd_dst_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long, d.n_slots,
        fs.data_ptr(), ldfs, fd.data_ptr(), ldfd, attn.data_ptr(), H, D, float(slope), de.data_ptr(), ldde, _ptr(dperm), _ptr(dfd), lddfd,
        _ptr(dattn), _ptr(workspace), _stream())), "gatv2_logits_bwd_dst")
    return dfd, dattn


def gatv2_logits_bwd_src(d_t, pos, fs, fd, attn, slope, de, out=None, partial=None):
    """include/bot_gnn.h bot_gatv2_logits_bwd_src_f32 on the transposed direction `d_t` (rows = sources) -> dfs [n_rows, H, D].  pos:
    contiguous int32 [nnz], de's row of each entry (Graph.csr2csc for de in CSC position order, the direction's eid for edge-id order); de:
    float32 [nnz, H] with unit inner stride; out: the dfs buffer (allocated when not given); partial: the long rows' n_slots * H * D floats."""
    _dev(fs, fd, attn, de, pos, out, d_t.indptr)
    n = d_t.n_rows
    H, D, ldfs, ldfd = _gatv2_operands("gatv2_logits_bwd_src", fs, fd, attn, n, int(fd.shape[0]))
    ldde = _edge_rows(de, d_t.nnz, H, "de", "gatv2_logits_bwd_src")
    if _i32(pos, "pos").numel() != d_t.nnz:
        raise BotKernelError(f"gatv2_logits_bwd_src: pos holds {pos.numel()} positions, the direction {d_t.nnz}")
    dfs = torch.empty((n, H, D), dtype=torch.float32, device=fs.device) if out is None else out
    lddfs = _heads3(dfs, n, H, D, "out", "gatv2_logits_bwd_src")
    if d_t.n_long and partial is None:
        partial = torch.empty(d_t.n_slots * H * D, dtype=torch.float32, device=fs.device)
    _check(_timed("gatv2_logits_bwd_src", (H, D), lambda: _lib.bot_gatv2_logits_bwd_src_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, pos.data_ptr(), fs.data_ptr(), ldfs, fd.data_ptr(), ldfd, attn.data_ptr(), H, D, float(slope), de.data_ptr(), ldde,
        dfs.data_ptr(), lddfs, _ptr(partial), _stream())), "gatv2_logits_bwd_src")
    return dfs


def _gate_rows(what, k, q, v, n_dst, n_src):
    """The operands of the gate sweeps -> (F, ldk, ldq, ldv): k float32 [n_dst, F], q and v float32 [n_src, F], unit inner strides (any
    row strides: q and v may be the two column blocks of one [n_src, 2F] matrix)."""
    if k.dim() != 2 or k.shape[1] < 1:
        raise BotKernelError(f"{what}: k must be [n_dst, F >= 1], got {tuple(k.shape)}")
    F = int(k.shape[1])
    return F, _rows2(k, n_dst, F, "k", what), _rows2(q, n_src, F, "q", what), _rows2(v, n_src, F, "v", what)


def spmm_gate(d, k, q, v, normalize=False, eps=1e-6, out=None, den=None, workspace=None):
    """include/bot_gnn.h bot_spmm_gate_f32 on the direction `d` (rows = destinations): num[r, f] = sum_j g_j v[indices[j], f] with g_j =
    sigmoid(k[r, f] + q[indices[j], f]), den = sum_j g_j; out = num, or - normalize - num / (den + eps).  k float32 [n_rows, F], q / v
    float32 [n_src, F] with unit inner stride (any row stride); out (and den, normalize only) float32 [n_rows, F] likewise (allocated
    when not given); workspace: the long rows' (2 if normalize else 1) * n_slots * F floats.  Returns (out, den or None)."""
    _dev(k, q, v, out, den, d.indptr)
    n = d.n_rows
    F, ldk, ldq, ldv = _gate_rows("spmm_gate", k, q, v, n, int(q.shape[0]))
    new = lambda: torch.empty((n, F), dtype=torch.float32, device=k.device)
    out = new() if out is None else out
    ldo, ldden = _rows2(out, n, F, "out", "spmm_gate"), F
    if normalize:
        den = new() if den is None else den
        ldden = _rows2(den, n, F, "den", "spmm_gate")
    else:
        den = None
    if d.n_long and workspace is None:
        workspace = torch.empty((2 if normalize else 1) * d.n_slots * F, dtype=torch.float32, device=k.device)
    _check(_timed("spmm_gate", (F, bool(normalize)), lambda: _lib.bot_spmm_gate_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, k.data_ptr(), ldk, q.data_ptr(), ldq, v.data_ptr(), ldv, F, int(bool(normalize)), float(eps), out.data_ptr(), ldo, _ptr(den),
        ldden, _ptr(workspace), _stream())), "spmm_gate")
    return out, den


def spmm_gate_bwd_dst(d, k, q, v, a, b=None, out=None, partial=None):
    """include/bot_gnn.h bot_spmm_gate_bwd_dst_f32 on the direction `d` (rows = destinations) -> dk [n_rows, F]: the sum over the row's
    positions of g' (v[u] a[r] + b[r]), g' the sigmoid's derivative at k[r] + q[u].  a (and b, or None) float32 [n_rows, F]; out: the dk
    buffer (unit inner stride, any row stride; allocated when not given); partial: the long rows' n_slots * F floats."""
    _dev(k, q, v, a, b, out, d.indptr)
    n = d.n_rows
    F, ldk, ldq, ldv = _gate_rows("spmm_gate_bwd_dst", k, q, v, n, int(q.shape[0]))
    lda = _rows2(a, n, F, "a", "spmm_gate_bwd_dst")
    ldb = F if b is None else _rows2(b, n, F, "b", "spmm_gate_bwd_dst")
    dk = torch.empty((n, F), dtype=torch.float32, device=k.device) if out is None else out
    lddk = _rows2(dk, n, F, "out", "spmm_gate_bwd_dst")
    if d.n_long and partial is None:
        partial = torch.empty(d.n_slots * F, dtype=torch.float32, device=k.device)
    _check(_timed("spmm_gate_bwd_dst", (F, b is not None), lambda: _lib.bot_spmm_gate_bwd_dst_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        k.data_ptr(), ldk, q.data_ptr(), ldq, v.data_ptr(), ldv, a.data_ptr(), lda, _ptr(b), ldb, F, dk.data_ptr(), lddk, _ptr(partial),
        _stream())), "spmm_gate_bwd_dst")
    return dk


def spmm_gate_bwd_src(d_t, k, q, v, a, b=None, want_dq=True, want_dv=True, out_dq=None, out_dv=None, partial=None):
    """include/bot_gnn.h bot_spmm_gate_bwd_src_f32 on the transposed direction `d_t` (rows = sources) -> (dq [n_rows, F] or None, dv
    [n_rows, F] or None): dq[u] = the sum over the out-edges u -> w of g' (v[u] a[w] + b[w]), dv[u] = the sum of g a[w].  k, a (and b, or
    None) float32 [n_dst, F]; out_dq / out_dv: the buffers (unit inner stride, any row stride - the two column blocks of one [n_rows, 2F]
    gradient, say; allocated when not given); partial: the long rows' (2 with both outputs, else 1) * n_slots * F floats."""
    _dev(k, q, v, a, b, out_dq, out_dv, d_t.indptr)
    n, n_dst = d_t.n_rows, int(k.shape[0])
    F, ldk, ldq, ldv = _gate_rows("spmm_gate_bwd_src", k, q, v, n_dst, n)
    lda = _rows2(a, n_dst, F, "a", "spmm_gate_bwd_src")
    ldb = F if b is None else _rows2(b, n_dst, F, "b", "spmm_gate_bwd_src")
    new = lambda: torch.empty((n, F), dtype=torch.float32, device=k.device)
    dq = (new() if out_dq is None else out_dq) if want_dq else None
    dv = (new() if out_dv is None else out_dv) if want_dv else None
    lddq = F if dq is None else _rows2(dq, n, F, "out_dq", "spmm_gate_bwd_src")
    lddv = F if dv is None else _rows2(dv, n, F, "out_dv", "spmm_gate_bwd_src")
    if d_t.n_long and partial is None and (want_dq or want_dv):
        partial = torch.empty((int(want_dq) + int(want_dv)) * d_t.n_slots * F, dtype=torch.float32, device=k.device)
    _check(_timed("spmm_gate_bwd_src", (F, b is not None, want_dq, want_dv), lambda: _lib.bot_spmm_gate_bwd_src_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, d_t.n_slots, k.data_ptr(), ldk, q.data_ptr(), ldq, v.data_ptr(), ldv, a.data_ptr(), lda, _ptr(b), ldb, F, _ptr(dq), lddq,
        _ptr(dv), lddv, _ptr(partial), _stream())), "spmm_gate_bwd_src")
    return dq, dv


# The two CSC sweeps' streamed rows (c, e, de, ds) with non-temporal accesses.  Measured both ways (tools/bench_gatedgcn.py, README "GatedGCN
# with an edge stream"): faster beyond both spreads wherever a per-edge row is WRITTEN (the forward that stores e, the backward), a tie
# or slower in the forward without e, which therefore keeps ordinary accesses.  Values and bytes are the same either way.
GATE_EDGE_STREAM_NT = True


def spmm_gate_edge(d, k, q, v, c, normalize=False, eps=1e-6, out=None, den=None, e=None, want_e=True, workspace=None, stream_nt=None):
    """include/bot_gnn.h bot_spmm_gate_edge_f32 on the direction `d` (rows = destinations): s_j = (k[r] + q[indices[j]]) + c[j], e[j] =
    s_j, num[r] = sum_j g(s_j) v[indices[j]], den = sum_j g(s_j); out = num, or - normalize - num / (den + eps).  k float32 [n_rows, F], q
    / v float32 [n_src, F], c float32 [nnz, F] in position order, unit inner strides (any row stride); out (and den, normalize only)
    float32 [n_rows, F] and e float32 [nnz, F] likewise (allocated when not given; e may be c itself; want_e=False: e is not stored);
    workspace: the long rows' (2 if normalize else 1) * n_slots * F floats.  Returns (out, den or None, e or None)."""
    _dev(k, q, v, c, out, den, e, d.indptr)
    n = d.n_rows
    F, ldk, ldq, ldv = _gate_rows("spmm_gate_edge", k, q, v, n, int(q.shape[0]))
    ldc = _rows2(c, d.nnz, F, "c", "spmm_gate_edge")
    new = lambda: torch.empty((n, F), dtype=torch.float32, device=k.device)
    out = new() if out is None else out
    ldo, ldden, lde = _rows2(out, n, F, "out", "spmm_gate_edge"), F, F
    if normalize:
        den = new() if den is None else den
        ldden = _rows2(den, n, F, "den", "spmm_gate_edge")
    else:
        den = None
    if want_e:
        e = torch.empty((d.nnz, F), dtype=torch.float32, device=k.device) if e is None else e
        lde = _rows2(e, d.nnz, F, "e", "spmm_gate_edge")
    else:
        e = None
    if d.n_long and workspace is None:
        workspace = torch.empty((2 if normalize else 1) * d.n_slots * F, dtype=torch.float32, device=k.device)
    nt = (GATE_EDGE_STREAM_NT and e is not None) if stream_nt is None else stream_nt
    _check(_timed("spmm_gate_edge", (F, bool(normalize), e is not None), lambda: _lib.bot_spmm_gate_edge_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, k.data_ptr(), ldk, q.data_ptr(), ldq, v.data_ptr(), ldv, c.data_ptr(), ldc, F, int(bool(normalize)), float(eps),
        out.data_ptr(), ldo, _ptr(den), ldden, _ptr(e), lde, int(bool(nt)), _ptr(workspace), _stream())), "spmm_gate_edge")
    return out, den, e


def spmm_gate_edge_bwd(d, v, e, a, b=None, de=None, want_ds=True, want_dk=True, out_ds=None, out_dk=None, partial=None, stream_nt=None):
    """include/bot_gnn.h bot_spmm_gate_edge_bwd_f32 on the direction `d` (rows = destinations) -> (ds [nnz, F] or None, dk [n_rows, F] or
    None): ds[j] = de[j] + g'(e[j]) (v[indices[j]] a[r] + b[r]), dk[r] = the sum of ds over the row's positions.  e: the forward's stored
    rows; a (and b, or None) float32 [n_rows, F]; de float32 [nnz, F] or None (zero); out_ds / out_dk: the buffers (unit inner stride, any
    row stride; allocated when not given; out_ds may be de itself); partial: the long rows' n_slots * F floats (dk only)."""
    _dev(v, e, a, b, de, out_ds, out_dk, d.indptr)
    n = d.n_rows
    if a.dim() != 2 or a.shape[1] < 1:
        raise BotKernelError(f"spmm_gate_edge_bwd: a must be [n_dst, F >= 1], got {tuple(a.shape)}")
    F = int(a.shape[1])
    lda = _rows2(a, n, F, "a", "spmm_gate_edge_bwd")
    ldv = _rows2(v, int(v.shape[0]), F, "v", "spmm_gate_edge_bwd")
    lde = _rows2(e, d.nnz, F, "e", "spmm_gate_edge_bwd")
    ldb = F if b is None else _rows2(b, n, F, "b", "spmm_gate_edge_bwd")
    ldde = F if de is None else _rows2(de, d.nnz, F, "de", "spmm_gate_edge_bwd")
    ds = (torch.empty((d.nnz, F), dtype=torch.float32, device=a.device) if out_ds is None else out_ds) if want_ds else None
    dk = (torch.empty((n, F), dtype=torch.float32, device=a.device) if out_dk is None else out_dk) if want_dk else None
    ldds = F if ds is None else _rows2(ds, d.nnz, F, "out_ds", "spmm_gate_edge_bwd")
    lddk = F if dk is None else _rows2(dk, n, F, "out_dk", "spmm_gate_edge_bwd")
    if d.n_long and partial is None and want_dk:
        partial = torch.empty(d.n_slots * F, dtype=torch.float32, device=a.device)
    nt = GATE_EDGE_STREAM_NT if stream_nt is None else stream_nt
    _check(_timed("spmm_gate_edge_bwd", (F, b is not None, de is not None, want_ds, want_dk), lambda: _lib.bot_spmm_gate_edge_bwd_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        v.data_ptr(), ldv, e.data_ptr(), lde, a.data_ptr(), lda, _ptr(b), ldb, _ptr(de), ldde, F, _ptr(ds), ldds, _ptr(dk), lddk, int(bool(nt)),
        _ptr(partial), _stream())), "spmm_gate_edge_bwd")
    return ds, dk


def spmm_gate_edge_bwd_src(d_t, pos, e, ds, a, want_dq=True, want_dv=True, out_dq=None, out_dv=None, partial=None):
    """include/bot_gnn.h bot_spmm_gate_edge_bwd_src_f32 on the transposed direction `d_t` (rows = sources) -> (dq [n_rows, F] or None, dv
    [n_rows, F] or None): dq[u] = the sum over the out-edges of ds[pos[j]], dv[u] = the sum of g(e[pos[j]]) a[indices[j]].  pos: contiguous
    int32 [nnz] (Graph.csr2csc); e, ds float32 [nnz, F] in CSC position order (ds may be None without dq; e and a without dv); a float32
    [n_dst, F]; out_dq / out_dv: the buffers (unit inner stride, any row stride; allocated when not given); partial: the long rows' (2 with
    both outputs, else 1) * n_slots * F floats."""
    _dev(e, ds, a, pos, out_dq, out_dv, d_t.indptr)
    n = d_t.n_rows
    first = next((t for t in (ds if want_dq else None, e if want_dv else None) if t is not None), None)
    if first is None:
        if want_dq or want_dv:
            raise BotKernelError("spmm_gate_edge_bwd_src: dq needs ds, dv needs e and a")
        return None, None
    if first.dim() != 2 or first.shape[1] < 1:
        raise BotKernelError(f"spmm_gate_edge_bwd_src: the per-edge rows must be [nnz, F >= 1], got {tuple(first.shape)}")
    F = int(first.shape[1])
    if _i32(pos, "pos").numel() != d_t.nnz:
        raise BotKernelError(f"spmm_gate_edge_bwd_src: pos holds {pos.numel()} positions, the direction {d_t.nnz}")
    ldds = _rows2(ds, d_t.nnz, F, "ds", "spmm_gate_edge_bwd_src") if want_dq else F
    lde, lda = F, F
    if want_dv:
        if e is None or a is None:
            raise BotKernelError("spmm_gate_edge_bwd_src: dv needs e and a")
        lde = _rows2(e, d_t.nnz, F, "e", "spmm_gate_edge_bwd_src")
        lda = _rows2(a, int(a.shape[0]), F, "a", "spmm_gate_edge_bwd_src")
    new = lambda: torch.empty((n, F), dtype=torch.float32, device=first.device)
    dq = (new() if out_dq is None else out_dq) if want_dq else None
    dv = (new() if out_dv is None else out_dv) if want_dv else None
    lddq = F if dq is None else _rows2(dq, n, F, "out_dq", "spmm_gate_edge_bwd_src")
    lddv = F if dv is None else _rows2(dv, n, F, "out_dv", "spmm_gate_edge_bwd_src")
    if d_t.n_long and partial is None:
        partial = torch.empty((int(want_dq) + int(want_dv)) * d_t.n_slots * F, dtype=torch.float32, device=first.device)
    _check(_timed("spmm_gate_edge_bwd_src", (F, want_dq, want_dv), lambda: _lib.bot_spmm_gate_edge_bwd_src_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, d_t.n_slots, pos.data_ptr(), _ptr(e) if want_dv else None, lde, _ptr(ds) if want_dq else None, ldds,
        _ptr(a) if want_dv else None, lda, F, _ptr(dq), lddq, _ptr(dv), lddv, _ptr(partial), _stream())), "spmm_gate_edge_bwd_src")
    return dq, dv


def _rel_operands(what, d, etype, norm, coef, num_rels):
    """The per-position operands of the relation sweeps on the direction `d`, checked -> (B or 0 for one-hot, coefficient columns)."""
    if _i32(etype, "etype").numel() != d.nnz:
        raise BotKernelError(f"{what}: etype holds {etype.numel()} positions, the direction {d.nnz}")
    if norm is not None and (_f32(norm, "norm").numel() != d.nnz or not norm.is_contiguous()):
        raise BotKernelError(f"{what}: norm must be contiguous float32 [{d.nnz}]")
    if coef is None:
        return 0, int(num_rels)
    if _f32(coef, "coef").dim() != 2 or coef.shape[0] != num_rels or not coef.is_contiguous():
        raise BotKernelError(f"{what}: coef must be contiguous float32 [{num_rels}, B], got {tuple(coef.shape)}")
    return int(coef.shape[1]), int(coef.shape[1])


def spmm_rel_expand(d, x, etype, num_rels, coef=None, norm=None, out=None, workspace=None):
    """include/bot_gnn.h bot_spmm_rel_expand_f32 on the direction `d` -> Z float32 [n_rows, B, F]: Z[r, b] = the sum over the row's positions
    j of norm[j] coef[etype[j], b] x[indices[j]].  x float32 [n_src, F] with unit inner stride (any row stride); etype int32 [nnz] and norm
    float32 [nnz] (or None) in `d`'s position order; coef float32 [num_rels, B] or None (one-hot: B = num_rels, the row goes into block
    etype[j] alone); out: the buffer ([n_rows, B, F], rows of unit stride, any row stride; allocated when not given); workspace: the long
    rows' n_slots * B * F floats."""
    _dev(x, etype, norm, coef, out, d.indptr)
    n = d.n_rows
    if x.dim() != 2 or x.shape[1] < 1:
        raise BotKernelError(f"spmm_rel_expand: x must be [n_src, F >= 1], got {tuple(x.shape)}")
    F = int(x.shape[1])
    ldx = _rows2(x, int(x.shape[0]), F, "x", "spmm_rel_expand")
    B, Bc = _rel_operands("spmm_rel_expand", d, etype, norm, coef, num_rels)
    out = torch.empty((n, Bc, F), dtype=torch.float32, device=x.device) if out is None else out
    if out.dim() != 3 or tuple(out.shape) != (n, Bc, F):
        raise BotKernelError(f"spmm_rel_expand: out must be [{n}, {Bc}, {F}], got {tuple(out.shape)}")
    ldo = _rows2(out.view(n, Bc * F) if out.is_contiguous() else out.flatten(1), n, Bc * F, "out", "spmm_rel_expand")
    if d.n_long and workspace is None:
        workspace = torch.empty(d.n_slots * Bc * F, dtype=torch.float32, device=x.device)
    _check(_timed("spmm_rel_expand", (F, int(num_rels), B), lambda: _lib.bot_spmm_rel_expand_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, etype.data_ptr(), _ptr(norm), _ptr(coef), int(num_rels), B, x.data_ptr(), ldx, F, out.data_ptr(), ldo, _ptr(workspace),
        _stream())), "spmm_rel_expand")
    return out


def spmm_rel_contract(d, y, etype, num_rels, coef=None, norm=None, out=None, workspace=None):
    """include/bot_gnn.h bot_spmm_rel_contract_f32 on the direction `d` -> out float32 [n_rows, F]: the sum over the row's positions j of
    norm[j] sum_b coef[etype[j], b] y[indices[j], b].  y float32 [n_src, B, F] (B = num_rels without coef: block etype[j] alone is
    gathered) whose rows [B * F] have unit stride (any row stride); etype, norm, coef as `spmm_rel_expand`; out: the buffer (unit inner
    stride, any row stride; allocated when not given); workspace: the long rows' n_slots * F floats."""
    _dev(y, etype, norm, coef, out, d.indptr)
    n = d.n_rows
    B, Bc = _rel_operands("spmm_rel_contract", d, etype, norm, coef, num_rels)
    if y.dim() != 3 or y.shape[1] != Bc or y.shape[2] < 1:
        raise BotKernelError(f"spmm_rel_contract: y must be [n_src, {Bc}, F >= 1], got {tuple(y.shape)}")
    F, n_src = int(y.shape[2]), int(y.shape[0])
    if y.stride(2) != 1 and F > 1 or (Bc > 1 and y.stride(1) != F):
        raise BotKernelError(f"spmm_rel_contract: the rows of y must be contiguous [{Bc} * {F}], got strides {tuple(y.stride())}")
    ldy = (max(int(y.stride(0)), Bc * F) if n_src == 1 else int(y.stride(0))) if n_src > 0 else Bc * F
    out = torch.empty((n, F), dtype=torch.float32, device=y.device) if out is None else out
    ldo = _rows2(out, n, F, "out", "spmm_rel_contract")
    if d.n_long and workspace is None:
        workspace = torch.empty(d.n_slots * F, dtype=torch.float32, device=y.device)
    _check(_timed("spmm_rel_contract", (F, int(num_rels), B), lambda: _lib.bot_spmm_rel_contract_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr), d.n_long,
        d.n_slots, etype.data_ptr(), _ptr(norm), _ptr(coef), int(num_rels), B, _f32(y, "y").data_ptr(), ldy, F, out.data_ptr(), ldo,
        _ptr(workspace), _stream())), "spmm_rel_contract")
    return out


def sddmm_dot_blocks(d, x, y):
    """out[k, b] = <x[indices[k], :], y[r, b, :]> for every position k of every row r (position order) -> float32 [nnz, B]: x float32
    [n_src, F] (any row stride), y float32 [n_rows, B, F] whose rows are contiguous (any row stride).  bot_sddmm_dot_bcast_f32 on the
    blocks of y as heads, four at a time, where one launch tile holds F; else bot_sddmm_dot_f32 on x repeated per block."""
    _dev(x, y, d.indptr)
    _f32(x, "x"), _f32(y, "y")
    n, B, F = y.shape
    if x.stride(1) != 1 and F > 1:
        x = x.contiguous()
    if y.stride(2) != 1 and F > 1 or (B > 1 and y.stride(1) != F):
        y = y.contiguous()
    ldy = int(y.stride(0)) if n > 1 else B * F
    ldx = int(x.stride(0)) if x.shape[0] > 1 else F
    vec = 4 if F % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 else (2 if F % 2 == 0 and ldx % 2 == 0 and ldy % 2 == 0 else 1)
    if F > 256 * vec or x.data_ptr() % 16 or y.data_ptr() % 16:
        return sddmm_dot(d, x.unsqueeze(1).expand(x.shape[0], B, F).contiguous(), y if y.is_contiguous() else y.contiguous())
    out = torch.empty((d.nnz, B), dtype=torch.float32, device=x.device)
    for b0 in range(0, B, 4):
        H = min(4, B - b0)
        part = out if B <= 4 else torch.empty((d.nnz, H), dtype=torch.float32, device=x.device)
        yb = y[:, b0:b0 + H]
        _check(_timed("sddmm_dot_bcast", (H, F), lambda: _lib.bot_sddmm_dot_bcast_f32(
            d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, x.data_ptr(), ldx,
            yb.data_ptr(), ldy, F, H, F, part.data_ptr(), None, _stream())), "sddmm_dot_bcast")
        if part is not out:
            out[:, b0:b0 + H] = part
    return out


def _dot_keep(keep, nnz, what):
    if keep is not None and _i32(keep, "keep").numel() != nnz:
        raise BotKernelError(f"{what}: keep holds {keep.numel()} positions, the direction {nnz}")
    return keep


DOT_EDGE_MAX_K = 16         # the widest raw edge feature the dot-product edge sweeps take (include/bot_gnn.h)


def _dot_edge_operands(what, d, n, H, D, qe, ef):
    """The edge operands of the dot-product edge sweeps -> (K, ldqe, ldef): qe float32 [n, H, K] with contiguous rows, ef float32
    [nnz, K] in position order with unit inner stride (any row stride)."""
    _f32(ef, "ef")
    if ef.dim() != 2 or ef.shape[0] != d.nnz or not 1 <= ef.shape[1] <= DOT_EDGE_MAX_K:
        raise BotKernelError(f"{what}: ef must be [{d.nnz}, 1 <= K <= {DOT_EDGE_MAX_K}] (one row per position), got {tuple(ef.shape)}")
    K = int(ef.shape[1])
    if D < K:
        raise BotKernelError(f"{what}: a head of D={D} columns has no slot for each of K={K} edge columns (D >= K)")
    return K, _heads3(qe, n, H, K, "qe", what), _rows2(ef, d.nnz, K, "ef", what)


def _dot_plan(d, n_slots=True):
    """The direction's arguments of the sweeps over destinations (bot_dot_attn_bwd_dst_f32 alone takes no n_slots)."""
    return (d.indptr.data_ptr(), d.indices.data_ptr(), d.n_rows, d.nnz, d.items.data_ptr(), d.n_items, _ptr(d.long_rows), _ptr(d.long_ptr),
            d.n_long) + ((d.n_slots,) if n_slots else ())


def _dot_attn(what, d, q, k, v, scale, keep, p, out, lse, workspace, qe=None, ef=None, aef=None):
    """`dot_attn` and, with the edge operands (ef is not None), `dot_attn_edge` -> (out, lse, aef or None)."""
    edge = ef is not None
    _dev(q, k, v, qe, ef, keep, out, lse, aef, d.indptr)
    n = d.n_rows
    if q.dim() != 3 or q.shape[1] < 1 or q.shape[2] < 1:
        raise BotKernelError(f"{what}: q must be [{n}, H >= 1, D >= 1], got {tuple(q.shape)}")
    H, D = int(q.shape[1]), int(q.shape[2])
    n_src = int(k.shape[0])
    qkv = (q.data_ptr(), _heads3(q, n, H, D, "q", what), k.data_ptr(), _heads3(k, n_src, H, D, "k", what), v.data_ptr(),
           _heads3(v, n_src, H, D, "v", what))
    K, ldqe, ldef = _dot_edge_operands(what, d, n, H, D, qe, ef) if edge else (0, 0, 0)
    _dot_keep(keep, d.nnz, what)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=q.device)
    out, lse = new(n, H, D) if out is None else out, new(n, H) if lse is None else lse
    aef = new(n, H, K) if edge and aef is None else aef
    ldo, ldl = _heads3(out, n, H, D, "out", what), _rows2(lse, n, H, "lse", what)
    ldae = _heads3(aef, n, H, K, "aef", what) if edge else 0
    if d.n_long and workspace is None:
        workspace = new(d.n_slots * (H * D + 2 * H + H * K))
    tail = (float(scale), _ptr(keep), float(p), out.data_ptr(), ldo, lse.data_ptr(), ldl)
    if edge:
        launch = lambda: _lib.bot_dot_attn_edge_f32(*_dot_plan(d), *qkv, qe.data_ptr(), ldqe, ef.data_ptr(), ldef, H, D, K, *tail, aef.data_ptr(),
                                                    ldae, _ptr(workspace), _stream())
    else:
        launch = lambda: _lib.bot_dot_attn_f32(*_dot_plan(d), *qkv, H, D, *tail, _ptr(workspace), _stream())
    _check(_timed(what, (H, D, K) if edge else (H, D, k is v), launch), what)
    return out, lse, aef


def _dot_attn_bwd_dst(what, d, q, k, v, scale, keep, p, dout, out, lse, want_dq, dq, pw, ds, partial, qe=None, ef=None, daef=None, aef=None,
                      want_dqe=False, dqe=None):
    """`dot_attn_bwd_dst` and, with the edge operands (ef is not None), `dot_attn_edge_bwd_dst` -> (dq or None, dqe or None, p, ds)."""
    edge = ef is not None
    _dev(q, k, v, qe, ef, keep, dout, daef, out, lse, aef, dq, dqe, d.indptr)
    n, H, D = d.n_rows, int(q.shape[1]), int(q.shape[2])
    n_src = int(k.shape[0])
    qkv = (q.data_ptr(), _heads3(q, n, H, D, "q", what), k.data_ptr(), _heads3(k, n_src, H, D, "k", what), v.data_ptr(),
           _heads3(v, n_src, H, D, "v", what))
    K, ldqe, ldef = _dot_edge_operands(what, d, n, H, D, qe, ef) if edge else (0, 0, 0)
    ldd, ldo, ldl = _heads3(dout, n, H, D, "dout", what), _heads3(out, n, H, D, "out", what), _rows2(lse, n, H, "lse", what)
    ldae, lddae = (_heads3(aef, n, H, K, "aef", what), _heads3(daef, n, H, K, "daef", what)) if edge else (0, 0)
    _dot_keep(keep, d.nnz, what)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=q.device)
    pw, ds = new(d.nnz, H) if pw is None else pw, new(d.nnz, H) if ds is None else ds
    for t, name in ((pw, "p"), (ds, "ds")):
        if _f32(t, name).shape != (d.nnz, H) or not t.is_contiguous():
            raise BotKernelError(f"{what}: {name} must be contiguous [{d.nnz}, {H}], got {tuple(t.shape)}")
    dq = (new(n, H, D) if dq is None else dq) if want_dq else None
    dqe = (new(n, H, K) if dqe is None else dqe) if want_dqe else None
    lddq = _heads3(dq, n, H, D, "dq", what) if want_dq else H * D
    lddqe = _heads3(dqe, n, H, K, "dqe", what) if want_dqe else H * K
    if (want_dq or want_dqe) and d.n_long and partial is None:
        partial = new(d.n_slots * (H * D + H * K))
    grads = (dout.data_ptr(), ldd, out.data_ptr(), ldo, lse.data_ptr(), ldl)
    if edge:
        launch = lambda: _lib.bot_dot_attn_edge_bwd_dst_f32(
            *_dot_plan(d), *qkv, qe.data_ptr(), ldqe, ef.data_ptr(), ldef, H, D, K, float(scale), _ptr(keep), float(p), *grads, aef.data_ptr(),
            ldae, daef.data_ptr(), lddae, pw.data_ptr(), ds.data_ptr(), _ptr(dq), lddq, _ptr(dqe), lddqe, _ptr(partial), _stream())
    else:
        launch = lambda: _lib.bot_dot_attn_bwd_dst_f32(*_dot_plan(d, n_slots=False), *qkv, H, D, float(scale), _ptr(keep), float(p), *grads,
                                                       pw.data_ptr(), ds.data_ptr(), _ptr(dq), lddq, _ptr(partial), _stream())
    _check(_timed(what, (H, D, K, want_dq, want_dqe) if edge else (H, D, k is v, want_dq), launch), what)
    return dq, dqe, pw, ds


def dot_attn(d, q, k, v, scale, keep=None, p=0.0, out=None, lse=None, workspace=None):
    """include/bot_gnn.h bot_dot_attn_f32 on the direction `d` (rows = destinations) -> (out [n_rows, H, D], lse [n_rows, H]): per head
    the softmax over a row's positions of scale * <q[row], k[indices[pos]]>, applied to the v rows.  q float32 [n_rows, H, D], k / v
    float32 [n_src, H, D] with contiguous rows (any row stride; the same tensor: one gather per edge); keep: contiguous int32 [nnz] in
    position order, bit h = head h is kept (then the kept weights are scaled by 1 / (1 - p)); out / lse allocated when not given;
    workspace: the long rows' n_slots * (H * D + 2 H) floats.  A head too wide for one tile raises BotKernelError (rc -2)."""
    return _dot_attn("dot_attn", d, q, k, v, scale, keep, p, out, lse, workspace)[:2]


def dot_attn_bwd_dst(d, q, k, v, scale, keep, p, dout, out, lse, want_dq=True, dq=None, pw=None, ds=None, partial=None):
    """include/bot_gnn.h bot_dot_attn_bwd_dst_f32 on the direction `d` (rows = destinations) -> (dq [n_rows, H, D] or None, p [nnz, H],
    ds [nnz, H]): the kept, scaled attention weights and the logits' gradients per position (what dot_attn_bwd_src reads) and, with
    want_dq, the queries' gradient.  dout / out float32 [n_rows, H, D], lse [n_rows, H] as dot_attn left them."""
    dq, _, pw, ds = _dot_attn_bwd_dst("dot_attn_bwd_dst", d, q, k, v, scale, keep, p, dout, out, lse, want_dq, dq, pw, ds, partial)
    return dq, pw, ds


def dot_attn_bwd_src(d_t, pos, q, dout, pw, ds, scale, want_dk=True, want_dv=True, shared=False, dk=None, dv=None, partial=None):
    """include/bot_gnn.h bot_dot_attn_bwd_src_f32 on the transposed direction `d_t` (rows = sources) -> (dk, dv) [n_rows, H, D] each (None
    where not asked for); shared: ONE tensor that holds dk + dv, returned twice (k and v were the same rows).  pos: contiguous int32 [nnz]
    (Graph.csr2csc); q / dout float32 [n_dst, H, D]; pw / ds float32 [nnz, H] from dot_attn_bwd_dst."""
    _dev(q, dout, pw, ds, pos, dk, dv, d_t.indptr)
    n, H, D, n_dst = d_t.n_rows, int(q.shape[1]), int(q.shape[2]), int(q.shape[0])
    what = "dot_attn_bwd_src"
    ldq, ldd = _heads3(q, n_dst, H, D, "q", what), _heads3(dout, n_dst, H, D, "dout", what)
    if _i32(pos, "pos").numel() != d_t.nnz:
        raise BotKernelError(f"{what}: pos holds {pos.numel()} positions, the direction {d_t.nnz}")
    for t, name in ((pw, "p"), (ds, "ds")):
        if _f32(t, name).shape != (d_t.nnz, H) or not t.is_contiguous():
            raise BotKernelError(f"{what}: {name} must be contiguous [{d_t.nnz}, {H}], got {tuple(t.shape)}")
    new = lambda: torch.empty((n, H, D), dtype=torch.float32, device=q.device)
    if shared:
        dk = dv = (new() if dk is None else dk)
    else:
        dk = (new() if dk is None else dk) if want_dk else None
        dv = (new() if dv is None else dv) if want_dv else None
    if dk is None and dv is None:
        return None, None
    lddk = H * D if dk is None else _heads3(dk, n, H, D, "dk", what)
    lddv = H * D if dv is None else _heads3(dv, n, H, D, "dv", what)
    if d_t.n_long and partial is None:
        partial = torch.empty(2 * d_t.n_slots * H * D, dtype=torch.float32, device=q.device)
    _check(_timed(what, (H, D, bool(shared)), lambda: _lib.bot_dot_attn_bwd_src_f32(
        d_t.indptr.data_ptr(), d_t.indices.data_ptr(), n, d_t.nnz, d_t.items.data_ptr(), d_t.n_items, _ptr(d_t.long_rows), _ptr(d_t.long_ptr),
        d_t.n_long, d_t.n_slots, pos.data_ptr(), q.data_ptr(), ldq, dout.data_ptr(), ldd, pw.data_ptr(), ds.data_ptr(), H, D, float(scale),
        _ptr(dk), lddk, _ptr(dv), lddv, _ptr(partial), _stream())), what)
    return dk, dv


def dot_attn_edge(d, q, k, v, qe, ef, scale, keep=None, p=0.0, out=None, lse=None, aef=None, workspace=None):
    """include/bot_gnn.h bot_dot_attn_edge_f32 on the direction `d` (rows = destinations) -> (out [n_rows, H, D], lse [n_rows, H], aef
    [n_rows, H, K]): `dot_attn` whose logit gains <qe[row, h], ef[pos]> and which also reduces aef = sum p ef.  qe float32 [n_rows, H, K]
    (q times the edge encoder's weights, per head); ef float32 [nnz, K <= 16] in POSITION order; D >= K; the rest as `dot_attn`;
    workspace: the long rows' n_slots * (H * D + 2 H + H * K) floats."""
    return _dot_attn("dot_attn_edge", d, q, k, v, scale, keep, p, out, lse, workspace, qe, ef, aef)


def dot_attn_edge_bwd_dst(d, q, k, v, qe, ef, scale, keep, p, dout, daef, out, lse, aef, want_dq=True, want_dqe=True, dq=None, dqe=None, pw=None,
                          ds=None, partial=None):
    """include/bot_gnn.h bot_dot_attn_edge_bwd_dst_f32 on the direction `d` (rows = destinations) -> (dq [n_rows, H, D] or None, dqe
    [n_rows, H, K] or None, p [nnz, H], ds [nnz, H]).  dout / out float32 [n_rows, H, D], daef / aef float32 [n_rows, H, K], lse
    [n_rows, H] as `dot_attn_edge` left them; p and ds are what `dot_attn_bwd_src` reads.  partial: the long rows' n_slots * (H * D +
    H * K) floats."""
    return _dot_attn_bwd_dst("dot_attn_edge_bwd_dst", d, q, k, v, scale, keep, p, dout, out, lse, want_dq, dq, pw, ds, partial, qe, ef, daef, aef,
                             want_dqe, dqe)


def edge_mlp_fwd(ef, W1, b1, W2):
    """ee[e,:] = W2 . relu(W1 . ef[e,:] + b1)   ef [E,8], W1 [16,8], b1 [16], W2 [H,16] -> [E,H]"""
    _dev(ef, W1, b1, W2)
    ef, W1, b1, W2 = (_f32(t, "edge_mlp operand").contiguous() for t in (ef, W1, b1, W2))
    E, H = ef.shape[0], W2.shape[0]
    out = torch.empty((E, H), dtype=torch.float32, device=ef.device)
    _check(_lib.bot_edge_mlp_fwd_f32(ef.data_ptr(), ef.shape[1], W1.data_ptr(), b1.data_ptr(), W1.shape[0], W2.data_ptr(), H, E,
                                     out.data_ptr(), _stream()), "edge_mlp_fwd")
    return out


def edge_mlp_bwd(ef, W1, b1, W2, dz):
    """Weight gradients (dW1 [16,8], db1 [16], dW2 [H,16]) of edge_mlp_fwd for upstream dz [E,H]."""
    _dev(ef, W1, b1, W2, dz)
    ef, W1, b1, W2, dz = (_f32(t, "edge_mlp operand").contiguous() for t in (ef, W1, b1, W2, dz))
    E, H = ef.shape[0], W2.shape[0]
    dW1, db1, dW2 = torch.empty_like(W1), torch.empty_like(b1), torch.empty_like(W2)
    ws = torch.empty(int(_lib.bot_edge_mlp_workspace_floats()), dtype=torch.float32, device=ef.device)
    _check(_lib.bot_edge_mlp_bwd_f32(ef.data_ptr(), ef.shape[1], W1.data_ptr(), b1.data_ptr(), W1.shape[0], W2.data_ptr(), H,
                                     dz.data_ptr(), E, dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(), ws.data_ptr(), _stream()),
           "edge_mlp_bwd")
    return dW1, db1, dW2


# ------------------------------------------------------------------------------------------------ merged projection weight
def merge_weight_fwd(W, Wres, attn_l, attn_r, H, D, P, with_fc, block=None):
    """[K, P] = [W^T (with_fc) | Wres^T | wl | wr | 0] (include/bot_gnn.h bot_merge_weight_fwd_f32); `block`: column width of the two
    copied blocks (default H*D)."""
    block = H * D if block is None else int(block)
    _dev(W, Wres, attn_l, attn_r)
    W = _f32(W, "W").contiguous()
    Wres = None if Wres is None else _f32(Wres, "Wres").contiguous()
    al = _f32(attn_l, "attn_l").contiguous()
    ar = None if attn_r is None else _f32(attn_r, "attn_r").contiguous()
    K = W.shape[1]
    out = torch.empty((K, P), dtype=torch.float32, device=W.device)
    _check(_lib.bot_merge_weight_fwd_f32(W.data_ptr(), _ptr(Wres), al.data_ptr(), _ptr(ar), H, D, K, P, int(with_fc), block, out.data_ptr(),
                                         _stream()), "merge_weight_fwd")
    return out


def merge_weight_bwd(W, attn_l, attn_r, H, D, P, with_fc, has_res, dm, block=None):
    _dev(W, attn_l, attn_r, dm)
    block = H * D if block is None else int(block)
    W, al, dm = W.contiguous(), attn_l.contiguous(), _f32(dm, "d_merged").contiguous()
    ar = None if attn_r is None else attn_r.contiguous()
    K = W.shape[1]
    dW = torch.empty_like(W)
    dWres = torch.empty_like(W) if has_res else None
    dal = torch.empty_like(al)
    dar = None if ar is None else torch.empty_like(ar)
    _check(_lib.bot_merge_weight_bwd_f32(W.data_ptr(), al.data_ptr(), _ptr(ar), H, D, K, P, int(with_fc), block, dm.data_ptr(), dW.data_ptr(),
                                         _ptr(dWres), dal.data_ptr(), _ptr(dar), _stream()), "merge_weight_bwd")
    return dW, dWres, dal, dar
