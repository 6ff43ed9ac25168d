"""ctypes binding of include/nnc.h (csrc/libnnc_hip.so).

There is NO CPU fallback: if the HIP library is missing or fails to load, every product
entry point raises ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes
import os

from . import build as _build

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_f32 = ctypes.c_float
c_size = ctypes.c_size_t

NNC_OK = 0
NNC_KMAX = 1040
NNC_CHUNK = 8192
FOLD_SUM, FOLD_MEAN, FOLD_STD = 0, 1, 2
NNC_KM_TWO_LAUNCH = 1   # nnc_kmeans_params.flags: iterate launch by launch (include/nnc.h)
NNC_KM_LOOP = 2         # ... inside one resident workgroup whatever K
NNC_KM_MASS_IN_PLACE = 4  # ... nnc_kmeans_fit: mass empty-cluster events settled by the finalize step (experiment; include/nnc.h)
NNC_KM_LOOP_KMAX = 64  # up to here the library takes the loop by itself
CBMM_NONE, CBMM_STREAM, CBMM_TILED, CBMM_BIAS = 0, 1, 2, 3   # nnc_cbmm_plan: the path a call takes (include/nnc.h)
CBMM_PLAN_LEN = 12
CBMM_PLAN_FIELDS = ("path", "vb", "mt", "copies", "entries", "splits", "rps", "aligned", "lds", "col_tiles", "row_tiles", "workspace")
CBMM_ZERO = 4   # nnc_cbmm_dx_plan / nnc_cbmm_dc_plan: the output is zero-filled (include/nnc.h)
CBMM_MFMA = 5   # nnc_cbmm_h16_plan: m > 16 runs k_cbmm_mfma
DT_F32, DT_BF16, DT_F16 = 0, 1, 2   # NNC_DT_*: the activation / output types of nnc_cbmm_h16
CBMM_H16_PLAN_LEN = 13
CBMM_H16_PLAN_FIELDS = CBMM_PLAN_FIELDS + ("dtype",)
CBMM_GROUPED_PLAN_LEN = 16   # nnc_cbmm_grouped_plan: the h16 fields, then the groups
CBMM_GROUPED_PLAN_FIELDS = CBMM_H16_PLAN_FIELDS + ("group_rows", "groups", "max_groups_per_split")
CBDX_PLAN_LEN = 12
CBDX_PLAN_FIELDS = ("path", "vb", "mt", "copies", "entries", "splits", "cps", "aligned", "lds", "col_tiles", "row_tiles", "workspace")
CBDC_PLAN_LEN = 12
CBDC_PLAN_FIELDS = ("path", "vb", "mt", "copies", "splits", "rps", "aligned", "lds", "col_tiles", "row_tiles", "terms_log2", "workspace")
CBGRAD_GROUPED_PLAN_LEN = 16   # nnc_cbmm_grouped_dx_plan / nnc_cbmm_grouped_dc_plan: the ungrouped fields, then the groups
_CBGRAD_GROUPED_TAIL = ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup")
CBDX_GROUPED_PLAN_FIELDS = CBDX_PLAN_FIELDS + _CBGRAD_GROUPED_TAIL
CBDC_GROUPED_PLAN_FIELDS = CBDC_PLAN_FIELDS + _CBGRAD_GROUPED_TAIL
CBGRAD_H16_PLAN_LEN = 13   # nnc_cbmm_dx_h16_plan / nnc_cbmm_dc_h16_plan: the float32 fields, then the dtype
CBDX_H16_PLAN_FIELDS = CBDX_PLAN_FIELDS + ("dtype",)
CBDC_H16_PLAN_FIELDS = CBDC_PLAN_FIELDS + ("dtype",)
CBSP_ROWSUM_NONE, CBSP_ROWSUM_FUSED, CBSP_ROWSUM_PASS = 0, 1, 2   # nnc_cbsp_plan: how the row sums of x are formed (include/nnc.h)
CBSP_PLAN_LEN = 11
CBSP_PLAN_FIELDS = ("path", "mt", "copies", "entries", "splits", "rps", "rowsum", "lds", "col_tiles", "row_tiles", "workspace")
CBSP_GROUPED_PLAN_LEN = 14   # nnc_cbsp_grouped_plan (include/nnc_cbsp_grouped.h): the sparse fields, then the groups
CBSP_GROUPED_PLAN_FIELDS = CBSP_PLAN_FIELDS + ("group_rows", "groups", "max_groups_per_split")
CBSP_GROUPED_H16_PLAN_LEN = 15   # nnc_cbsp_grouped_h16_plan (include/nnc_cbsp_grouped_h16.h): the grouped sparse fields, then the dtype; path is CBMM_MFMA for m > 16
CBSP_GROUPED_H16_PLAN_FIELDS = CBSP_GROUPED_PLAN_FIELDS + ("dtype",)
CBSP_H16_PLAN_LEN = 12   # nnc_cbsp_h16_plan (include/nnc_cbsp_h16.h): path is CBMM_MFMA for m > 16
CBSP_H16_PLAN_FIELDS = CBSP_PLAN_FIELDS + ("dtype",)
CBPK_TABLE_NONE, CBPK_TABLE_BANKED = 0, 1   # nnc_cbpk_plan: the layout of the lookup table (include/nnc.h)
CBPK_PLAN_LEN = 14
CBPK_PLAN_FIELDS = ("path", "vb", "mt", "cols", "xrows", "table", "copies", "entries", "splits", "rps", "lds", "col_tiles", "row_tiles", "workspace")
CBPK_GROUPED_PLAN_LEN = 19   # nnc_cbpk_grouped_plan: the packed fields, then the dtype, the groups and the tables in LDS
CBPK_GROUPED_PLAN_FIELDS = CBPK_PLAN_FIELDS + ("dtype", "group_rows", "groups", "max_groups_per_split", "tables")
CBPKDX_PLAN_LEN = 12   # nnc_cbpk_dx_plan / nnc_cbpk_dc_plan (include/nnc.h)
CBPKDX_PLAN_FIELDS = ("path", "vb", "mt", "cols", "copies", "entries", "splits", "cps", "lds", "col_tiles", "row_tiles", "workspace")
CBPKDC_PLAN_LEN = 12
CBPKDC_PLAN_FIELDS = ("path", "vb", "mt", "cols", "copies", "splits", "rps", "lds", "col_tiles", "row_tiles", "terms_log2", "workspace")
CBPKGRAD_GROUPED_PLAN_LEN = 17   # nnc_cbpk_grouped_dx_plan / nnc_cbpk_grouped_dc_plan: the ungrouped packed fields, then the groups
_CBPKGRAD_GROUPED_TAIL = _CBGRAD_GROUPED_TAIL + ("held",)   # dx: the tables held in LDS; dc: the per-group sets of bins
CBPKDX_GROUPED_PLAN_FIELDS = CBPKDX_PLAN_FIELDS + _CBPKGRAD_GROUPED_TAIL
CBPKDC_GROUPED_PLAN_FIELDS = CBPKDC_PLAN_FIELDS + _CBPKGRAD_GROUPED_TAIL
CBSPDX_PLAN_LEN = 11   # nnc_cbsp_dx_plan / nnc_cbsp_dc_plan (include/nnc.h)
CBSPDX_PLAN_FIELDS = ("path", "mt", "segs", "copies", "entries", "splits", "cps", "lds", "col_tiles", "row_tiles", "workspace")
CBSPDC_PLAN_LEN = 11
CBSPDC_PLAN_FIELDS = ("path", "mt", "segs", "copies", "splits", "rps", "lds", "col_tiles", "row_tiles", "terms_log2", "workspace")
CBSPGRAD_H16_PLAN_LEN = 12   # nnc_cbsp_dx_h16_plan / nnc_cbsp_dc_h16_plan (include/nnc_cbspgrad_h16.h): the float32 sparse fields, then the dtype
CBSPDX_H16_PLAN_FIELDS = CBSPDX_PLAN_FIELDS + ("dtype",)
CBSPDC_H16_PLAN_FIELDS = CBSPDC_PLAN_FIELDS + ("dtype",)
# nnc_cbsp_grouped_dx_plan / nnc_cbsp_grouped_dc_plan (include/nnc_cbspgrad_grouped.h): the float32 sparse fields, then the groups
CBSPDX_GROUPED_PLAN_LEN = 16
CBSPDX_GROUPED_PLAN_FIELDS = CBSPDX_PLAN_FIELDS + ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup", "tables")
CBSPDC_GROUPED_PLAN_LEN = 15
CBSPDC_GROUPED_PLAN_FIELDS = CBSPDC_PLAN_FIELDS + ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup")
CBPK_H16_PLAN_LEN = 15   # nnc_cbpk_h16_plan (include/nnc_cbpk_h16.h): the float32 packed fields, then the dtype; path is CBMM_MFMA for m > 16
CBPK_H16_PLAN_FIELDS = CBPK_PLAN_FIELDS + ("dtype",)
CBGRAD_GROUPED_H16_PLAN_LEN = 18   # nnc_cbmm_grouped_*_h16_plan and nnc_cbpk_grouped_*_h16_plan: the ungrouped half fields, then the groups and the tables / sets held in LDS
_CBGRAD_GROUPED_H16_TAIL = _CBGRAD_GROUPED_TAIL + ("held",)
CBDX_GROUPED_H16_PLAN_FIELDS = CBDX_H16_PLAN_FIELDS + _CBGRAD_GROUPED_H16_TAIL
CBDC_GROUPED_H16_PLAN_FIELDS = CBDC_H16_PLAN_FIELDS + _CBGRAD_GROUPED_H16_TAIL
CBPKGRAD_H16_PLAN_LEN = 13   # nnc_cbpk_dx_h16_plan / nnc_cbpk_dc_h16_plan: the float32 packed fields, then the dtype
CBPKDX_H16_PLAN_FIELDS = CBPKDX_PLAN_FIELDS + ("dtype",)
CBPKDC_H16_PLAN_FIELDS = CBPKDC_PLAN_FIELDS + ("dtype",)
# nnc_cbpk_grouped_dx_h16_plan / _dc_h16_plan: the ungrouped packed half fields, then the groups (CBGRAD_GROUPED_H16_PLAN_LEN values too)
CBPKDX_GROUPED_H16_PLAN_FIELDS = CBPKDX_H16_PLAN_FIELDS + _CBGRAD_GROUPED_H16_TAIL
CBPKDC_GROUPED_H16_PLAN_FIELDS = CBPKDC_H16_PLAN_FIELDS + _CBGRAD_GROUPED_H16_TAIL


class NativeLibraryError(RuntimeError):
    pass


class NncError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"nnc error {code}: {message}")
        self.code = code


class KMeansParams(ctypes.Structure):
    _fields_ = [
        ("n", c_i64), ("n_total", c_i64), ("k", c_i32), ("max_iter", c_i32), ("fix_shift", c_i32),
        ("grid_log2", c_i32), ("replicas_log2", c_i32), ("flags", c_i32),
        ("x_mean", c_f32), ("tol", c_f32), ("lo", c_f32), ("hi", c_f32),
        ("prefix_dev", c_void_p),
    ]


class KMeansStatus(ctypes.Structure):
    _fields_ = [
        ("iter", c_i32), ("done", c_i32), ("paused", c_i32), ("n_empty", c_i32),
        ("shift_tot", c_f32), ("tol", c_f32), ("k", c_i32), ("same_counts", c_i32),
        ("reloc_ties", c_i32), ("reloc_multi", c_i32), ("n_relocated", c_i32), ("n_unproven", c_i32),
        ("n_in_place", c_i32), ("n_reloc_null", c_i32),
    ]


class LayerParams(ctypes.Structure):
    _fields_ = [("q", c_f32), ("prune", c_i32), ("std_smooth", c_i32), ("bits", c_i32), ("mode", c_i32), ("want_values", c_i32),
                ("km_flags", c_i32), ("reserved", c_i32)]


class LayerResult(ctypes.Structure):
    _fields_ = [
        ("status", c_i32), ("k", c_i32), ("label_bytes", c_i32), ("arith", c_i32),
        ("n_iter", c_i32), ("stop", c_i32), ("n_relocations", c_i32), ("n_reloc_windowed", c_i32), ("reloc_ties", c_i32), ("reloc_multi", c_i32),
        ("sigma", c_f32), ("threshold", c_f32),
        ("n_zeroed", c_i64), ("total_bits", c_i64),
        ("centers", c_f32 * NNC_KMAX), ("counts", c_i64 * NNC_KMAX), ("code_lengths", ctypes.c_uint8 * NNC_KMAX),
    ]


# name -> (restype, argtypes); every symbol include/nnc.h declares
SIGNATURES = {
    "nnc_version": (c_int, []),
    "nnc_last_error": (ctypes.c_char_p, []),
    "nnc_device_info": (c_int, [ctypes.c_char_p, c_size, ctypes.POINTER(c_int)]),
    "nnc_chunk_sums_f32": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p]),
    "nnc_fold_f32": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p]),
    "nnc_prune_workspace_bytes": (c_size, [c_i64]),
    "nnc_prune_f32": (c_int, [c_void_p, c_i64, c_f32, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_sort_pruned_bounded_bits": (c_i32, [c_f32, c_f32, c_f32, c_i64, c_i64]),
    "nnc_sort_pruned_bounded_workspace_bytes": (c_size, [c_i64]),
    "nnc_sort_pruned_bounded_flag": (c_void_p, [c_void_p, c_i64]),
    "nnc_sort_pruned_bounded_f32": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_f32, c_f32, c_f32, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_sort_threshold_keys_workspace_bytes": (c_size, [c_i64]),
    "nnc_sort_threshold_keys_f32": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p, c_void_p]),
    "nnc_prune_stats_workspace_bytes": (c_size, [c_i64]),
    "nnc_prune_stats_f32": (c_int, [c_void_p, c_i64, c_f32, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_threshold_mask_f32": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nnc_apply_mask_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_minmax_workspace_bytes": (c_size, [c_i64]),
    "nnc_minmax_f32": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_minmax_signs_f32": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_layer_stats_workspace_bytes": (c_size, [c_i64]),
    "nnc_layer_stats_f32": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_rank_sorted_f32": (c_int, [c_void_p, c_i64, c_void_p, c_i32, c_void_p, c_void_p]),
    "nnc_hist31_f32": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p]),
    "nnc_sort_workspace_bytes": (c_size, [c_i64]),
    "nnc_sort_f32": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_sort_pruned_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "nnc_sort_pruned_f32": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_fix_shift": (c_i32, [c_f32, c_i64]),
    "nnc_kmeans_workspace_bytes": (c_size, [c_i32]),
    "nnc_kmeans_prefix_bytes": (c_size, [c_i64]),
    "nnc_kmeans_loop_stats": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nnc_kmeans_prefix_build": (c_int, [c_void_p, ctypes.POINTER(KMeansParams), c_void_p, c_void_p]),
    "nnc_kmeans_init": (c_int, [c_void_p, c_size, ctypes.POINTER(KMeansParams), c_void_p, c_void_p]),
    "nnc_kmeans_set_centers": (c_int, [c_void_p, ctypes.POINTER(KMeansParams), c_void_p, c_int, c_void_p]),
    "nnc_kmeans_accumulate": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_void_p]),
    "nnc_kmeans_partials": (c_void_p, [c_void_p]),
    "nnc_kmeans_finalize": (c_int, [c_void_p, c_int, c_void_p]),
    "nnc_kmeans_iterate": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p]),
    "nnc_kmeans_status_async": (c_int, [c_void_p, ctypes.POINTER(KMeansStatus), c_void_p]),
    "nnc_kmeans_status_publish": (c_int, [c_void_p, c_void_p, ctypes.c_uint64, c_void_p]),
    "nnc_kmeans_iterate_publish": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p, ctypes.c_uint64, c_void_p]),
    "nnc_kmeans_fit": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_i32, c_void_p, c_size, c_void_p,
                               ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(KMeansStatus), ctypes.POINTER(c_i32), c_void_p]),
    "nnc_kmeans_fit_sharded": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(KMeansParams), ctypes.c_int64, c_i32, c_i32, c_void_p, c_size,
                                       c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(KMeansStatus), ctypes.POINTER(c_i32), c_void_p]),
    "nnc_kmeans_set_done": (c_int, [c_void_p, c_i32, c_void_p]),
    "nnc_kmeans_label_counts": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_int, c_void_p, c_void_p]),
    "nnc_kmeans_get_centers": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "nnc_kmeans_assign": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nnc_topm_hist_f32": (c_int, [c_void_p, c_i64, c_i32, c_i32, c_i32, ctypes.c_uint32, c_void_p, c_void_p]),
    "nnc_topm_compact_f32": (c_int, [c_void_p, c_void_p, c_i64, ctypes.c_uint32, c_void_p, c_i64, c_void_p, c_void_p]),
    "nnc_kmeans_relocate": (c_int, [c_void_p, c_void_p, c_i32, c_void_p]),
    "nnc_kmeans_reloc_candidates": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p, c_i64, c_void_p, c_void_p, c_void_p]),
    "nnc_kmeans_relocate_checked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i32, c_void_p, c_void_p]),
    "nnc_kmeans_reloc_window": (c_i32, [c_i64, c_i32]),
    "nnc_kmeans_reloc_scratch_bytes": (c_size, [c_i32, c_i32]),
    "nnc_kmeans_relocate_windowed": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p, c_size, c_void_p]),
    "nnc_kmeans_reloc_select_local": (c_int, [c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p, c_size, c_void_p, c_void_p]),
    "nnc_kmeans_reloc_flag": (c_void_p, [c_void_p]),
    "nnc_kmeans_relocate_if_proven": (c_int, [c_void_p, c_void_p, c_i32, c_void_p]),
    "nnc_labels_equal": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    "nnc_ref_sums_f32": (c_int, [c_void_p, c_i64, ctypes.c_float, c_void_p, c_i32, c_i32, c_void_p, c_void_p, c_void_p]),
    "nnc_kmeans_set_done_if": (c_int, [c_void_p, c_void_p, c_i32, c_void_p]),
    "nnc_bincount": (c_int, [c_void_p, c_int, c_i64, c_i32, c_void_p, c_void_p]),
    "nnc_kmeans_fit_reference_f32": (c_int, [c_void_p, c_i32, c_void_p, c_i32, c_i32, c_f32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nnc_compress_layer_workspace_bytes": (c_size, [c_i64, c_i32]),
    "nnc_compress_layer_host_bytes": (c_size, []),
    "nnc_compress_layer_f32": (c_int, [c_void_p, c_i64, ctypes.POINTER(LayerParams), c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p, c_size,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(LayerResult), c_void_p]),
    "nnc_host_linspace_f32": (c_int, [c_f32, c_f32, c_i32, c_void_p]),
    "nnc_host_cdf": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "nnc_host_density_init": (c_int, [c_void_p, c_void_p, c_i32, c_void_p]),
    "nnc_kmeanspp_trials": (c_i32, [c_i32]),
    "nnc_kmeanspp_workspace_bytes": (c_size, [c_i64, c_i32]),
    "nnc_kmeanspp_seed_f32": (c_int, [c_void_p, c_i64, c_f32, c_i32, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "nnc_centroid_grad_f32": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i32, c_i32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nnc_gather_f32": (c_int, [c_void_p, c_i32, c_void_p, c_int, c_i64, c_void_p, c_void_p]),
    "nnc_cbmm_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbmm_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_int, c_i64, c_void_p, c_i32, c_void_p, c_i32, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_cbmm_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbmm_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_int, c_i64, c_void_p, c_i32, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_i64,
                             c_void_p]),
    "nnc_cbmm_grouped_workspace_bytes": (c_i64, [c_int, c_i64, c_i64, c_i64]),
    "nnc_cbmm_grouped_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_grouped": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_i64,
                                 c_void_p]),
    "nnc_cbmm_dx_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbmm_dx_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_dx_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_int, c_i64, c_void_p, c_i32, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_cbmm_dc_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32]),
    "nnc_cbmm_dc_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_dc_f32": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_int, c_i64, c_i32, c_void_p, c_i32, c_void_p, c_i64, c_void_p]),
    "nnc_cbsp_pack_bytes": (c_i64, [c_i64, c_i64, c_int, c_i64]),
    "nnc_cbsp_pack": (c_int, [c_void_p, c_int, c_i64, c_i64, c_i32, c_void_p, c_i64, c_void_p, c_void_p]),
    "nnc_cbsp_unpack": (c_int, [c_void_p, c_i64, c_int, c_i64, c_i64, c_i32, c_i64, c_void_p, c_void_p]),
    "nnc_cbsp_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbsp_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_i32, c_void_p,
                             c_void_p, c_i64, c_void_p]),
    "nnc_cbsp_dx_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbsp_dx_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_dx_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_void_p, c_i64,
                                c_void_p]),
    "nnc_cbsp_dc_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32]),
    "nnc_cbsp_dc_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_dc_f32": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_i32, c_void_p, c_i32, c_void_p,
                                c_i64, c_void_p]),
    "nnc_cbpk_row_bytes": (c_i64, [c_i64, c_int]),
    "nnc_cbpk_pack_bytes": (c_i64, [c_i64, c_i64, c_int]),
    "nnc_cbpk_pack": (c_int, [c_void_p, c_int, c_i64, c_i64, c_int, c_void_p, c_i64, c_void_p, c_void_p]),
    "nnc_cbpk_unpack": (c_int, [c_void_p, c_i64, c_int, c_i64, c_i64, c_void_p, c_int, c_void_p]),
    "nnc_cbpk_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_void_p, c_i32, c_void_p, c_void_p, c_i64,
                             c_void_p]),
    "nnc_cbpk_grouped_workspace_bytes": (c_i64, [c_int, c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_grouped_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_grouped": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_int,
                                 c_void_p, c_i64, c_void_p]),
    "nnc_cbpk_dx_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_dx_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_dx_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_cbpk_dc_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32]),
    "nnc_cbpk_dc_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_dc_f32": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_void_p, c_i32, c_void_p, c_i64, c_void_p]),
    "nnc_huffman_codes": (c_int, [ctypes.POINTER(ctypes.c_uint8), c_i32, ctypes.POINTER(ctypes.c_uint32)]),
    "nnc_codec_chunks": (c_size, [c_i64]),
    "nnc_huffman_chunk_offsets": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_i32, c_void_p, c_void_p]),
    "nnc_huffman_encode": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_i32, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_huffman_decode_tables_bytes": (c_size, []),
    "nnc_huffman_decode_tables": (c_int, [ctypes.POINTER(ctypes.c_uint8), c_i32, c_void_p, c_size]),
    "nnc_huffman_decode": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_void_p]),
    "nnc_sparse_entry_offsets": (c_int, [c_void_p, c_int, c_i64, c_i32, c_i32, c_void_p, c_void_p]),
    "nnc_sparse_emit": (c_int, [c_void_p, c_int, c_i64, c_i32, c_i32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nnc_sparse_expand": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_i64, c_i32, c_void_p, c_void_p, c_void_p]),
    "nnc_comm_unique_id": (c_int, [c_void_p, c_size]),
    "nnc_comm_init": (c_int, [ctypes.POINTER(c_void_p), c_void_p, c_size, c_i32, c_i32]),
    "nnc_comm_destroy": (c_int, [c_void_p]),
    "nnc_comm_rank": (c_int, [c_void_p]),
    "nnc_comm_world": (c_int, [c_void_p]),
    "nnc_comm_allreduce": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_i32, c_void_p]),
    "nnc_comm_allgather": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_kmeans_iterate_sharded": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p, ctypes.c_uint64, c_void_p]),
    "nnc_merge_keys": (c_int, [c_void_p, c_i32, c_i32, c_void_p, c_i32, c_void_p]),
    "nnc_kmeans_reloc_scratch_bytes_sharded": (c_size, [c_i32, c_i32, c_i32]),
    "nnc_kmeans_relocate_windowed_sharded": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(KMeansParams), c_i32, c_void_p, c_size, c_void_p]),
    "nnc_comm_available": (c_int, []),
    "nnc_profile_tags": (c_int, [ctypes.c_uint32]),
    "nnc_profile_begin": (c_int, [c_i32]),
    "nnc_profile_end": (c_int, [ctypes.POINTER(c_f32), ctypes.POINTER(c_i32), c_i64, ctypes.POINTER(c_i64)]),
    "nnc_huffman_lengths": (c_int, [ctypes.POINTER(c_i64), c_i32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbgrad_grouped.h declares (the part of the ABI nnc.h includes from a header
# of its own: the backward pass of the group-wise layer).  Required and bound by load() as SIGNATURES are.
GROUPED_GRAD_SIGNATURES = {
    "nnc_cbmm_grouped_dx_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "nnc_cbmm_grouped_dx_plan": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_grouped_dx_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_cbmm_grouped_dc_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_i32, c_i64]),
    "nnc_cbmm_grouped_dc_plan": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_grouped_dc_f32": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_i64, c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbgrad_h16.h declares (the backward pass of the byte form on bf16 / fp16
# activations, a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
H16_GRAD_SIGNATURES = {
    "nnc_cbmm_dx_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbmm_dx_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_dx_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_int, c_i64, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    "nnc_cbmm_dc_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32]),
    "nnc_cbmm_dc_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_dc_h16": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_int, c_i64, c_i32, c_void_p, c_i32, c_void_p, c_i64, c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbpkgrad_grouped.h declares (the backward pass of the group-wise packed layer,
# again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
GROUPED_PACKED_GRAD_SIGNATURES = {
    "nnc_cbpk_grouped_dx_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_grouped_dx_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_grouped_dx_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_void_p, c_i64, c_void_p]),
    "nnc_cbpk_grouped_dc_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32, c_i64]),
    "nnc_cbpk_grouped_dc_plan": (c_int, [c_i64, c_i64, c_i64, c_int, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_grouped_dc_f32": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_i64,
                                        c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbsp_h16.h declares (the bitmap-sparse layer on bf16 / fp16 activations, again a
# header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
SPARSE_H16_SIGNATURES = {
    "nnc_cbsp_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbsp_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_i32, c_void_p, c_int,
                             c_void_p, c_i64, c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbspgrad_h16.h declares (the backward pass of the bitmap-sparse layer on bf16 /
# fp16 activations, again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
SPARSE_H16_GRAD_SIGNATURES = {
    "nnc_cbsp_dx_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbsp_dx_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_dx_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_i64,
                                c_void_p]),
    "nnc_cbsp_dc_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32]),
    "nnc_cbsp_dc_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_dc_h16": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_i32, c_void_p, c_i32, c_void_p, c_i64,
                                c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbpk_h16.h declares (the 2- / 4-bit packed layer on bf16 / fp16 activations, forward
# and backward, again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
PACKED_H16_SIGNATURES = {
    "nnc_cbpk_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_i64,
                             c_void_p]),
    "nnc_cbpk_dx_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_dx_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_dx_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    "nnc_cbpk_dc_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32]),
    "nnc_cbpk_dc_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_dc_h16": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_void_p, c_i32, c_void_p, c_i64, c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbgrad_grouped_h16.h declares (the backward pass of the group-wise layers, byte and
# packed indices, on bf16 / fp16 activations, again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
GROUPED_H16_GRAD_SIGNATURES = {
    "nnc_cbmm_grouped_dx_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "nnc_cbmm_grouped_dx_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_grouped_dx_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    "nnc_cbmm_grouped_dc_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_i32, c_i64]),
    "nnc_cbmm_grouped_dc_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.c_uint64, ctypes.POINTER(c_i64)]),
    "nnc_cbmm_grouped_dc_h16": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_i64, c_void_p]),
    "nnc_cbpk_grouped_dx_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "nnc_cbpk_grouped_dx_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_grouped_dx_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_int, c_void_p, c_i64,
                                        c_void_p]),
    "nnc_cbpk_grouped_dc_h16_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_int, c_i32, c_i64]),
    "nnc_cbpk_grouped_dc_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbpk_grouped_dc_h16": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_int, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p, c_i64,
                                        c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbsp_grouped.h declares (the bitmap-sparse form of the group-wise layer, float32
# activations, again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
GROUPED_SPARSE_SIGNATURES = {
    "nnc_cbsp_grouped_pack": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "nnc_cbsp_grouped_unpack": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p]),
    "nnc_cbsp_grouped_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "nnc_cbsp_grouped_plan": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_grouped_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_i32, c_void_p,
                                     c_void_p, c_i64, c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbsp_grouped_h16.h declares (the bitmap-sparse form of the group-wise layer on
# bf16 / fp16 activations, again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
GROUPED_SPARSE_H16_SIGNATURES = {
    "nnc_cbsp_grouped_h16_workspace_bytes": (c_i64, [c_int, c_i64, c_i64, c_i64]),
    "nnc_cbsp_grouped_h16_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_grouped_h16": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_i32, c_void_p,
                                     c_int, c_void_p, c_i64, c_void_p]),
}

# name -> (restype, argtypes); every symbol include/nnc_cbspgrad_grouped.h declares (the backward pass of the group-wise layer from the
# bitmap-sparse form, float32 activations, again a header of its own that nnc.h includes).  Required and bound by load() as SIGNATURES are.
GROUPED_SPARSE_GRAD_SIGNATURES = {
    "nnc_cbsp_grouped_dx_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "nnc_cbsp_grouped_dx_plan": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_grouped_dx_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i32, c_i64, c_void_p, c_void_p, c_i64,
                                        c_void_p]),
    "nnc_cbsp_grouped_dc_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_i32, c_i64]),
    "nnc_cbsp_grouped_dc_plan": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i64, c_i32, ctypes.POINTER(c_i64)]),
    "nnc_cbsp_grouped_dc_f32": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i32, c_i64, c_void_p, c_i32, c_void_p,
                                        c_i64, c_void_p]),
}

# exported only by the diagnostics build (NNC_DIAG=1: libnnc_hip_diag.so, see build.py); bound when present
DIAG_SIGNATURES = {
    "nnc_debug_set_ablation": (c_int, [c_int]),
    "nnc_debug_set_trace": (c_int, [c_void_p]),
    "nnc_debug_clock": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "nnc_debug_reloc_fail": (c_int, [c_void_p, ctypes.POINTER(c_i32)]),
    "nnc_debug_kl_trace": (c_int, [c_void_p, c_void_p]),
    "nnc_debug_os_trace": (c_int, [c_void_p]),
}

_lib = None


def lib_path() -> str:
    return _build.LIB


def load():
    """Load libnnc_hip.so (must have been built: ``__graft_entry__.build()`` or
    ``python -m neural_network_compression_amd.build``).  Raises NativeLibraryError."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{path} is missing: the HIP extension has not been built "
            "(run `python -m neural_network_compression_amd.build`); there is no CPU fallback")
    try:
        L = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise NativeLibraryError(f"cannot load {path}: {e}; there is no CPU fallback") from e
    for name, (res, args) in list(SIGNATURES.items()) + list(GROUPED_GRAD_SIGNATURES.items()) + list(H16_GRAD_SIGNATURES.items()) + list(GROUPED_PACKED_GRAD_SIGNATURES.items()) + list(SPARSE_H16_SIGNATURES.items()) + list(SPARSE_H16_GRAD_SIGNATURES.items()) + list(PACKED_H16_SIGNATURES.items()) + list(GROUPED_H16_GRAD_SIGNATURES.items()) + list(GROUPED_SPARSE_SIGNATURES.items()) + list(GROUPED_SPARSE_H16_SIGNATURES.items()) + list(GROUPED_SPARSE_GRAD_SIGNATURES.items()):
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{path} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in DIAG_SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = L
    return L


def check(rc: int):
    if rc != NNC_OK:
        raise NncError(rc, load().nnc_last_error().decode("utf-8", "replace"))
