"""ctypes binding of libaicp_hip.so (include/aicp_hip.h).

The HIP library is the product: importing this module loads it and raises if it is missing
or does not export the declared entry points. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AICP_HIP_LIB") or os.path.join(PKG_DIR, "libaicp_hip.so")  # override: A/B builds

AICP_OK = 0
AICP_ERR_CONVERGENCE = 1
AICP_ERR_INVALID = 2
AICP_ERR_HIP = 3
AICP_ERR_UNSUPPORTED = 4
AICP_ERR_TRANSFORMATION = 5

AICP_RUN_OVERLAP = 1
AICP_RUN_ICP = 2
AICP_RUN_TIME_NN = 4
AICP_SEQ_DEBUG = 8  # aicp_sequence_params.flags: App's "debug" working_mode
AICP_MON_PAIRED = 1  # aicp_monitor_params.flags: also the chain matcher's paired mean distance
AICP_LOC_MERGE = 16  # aicp_localization_params.flags: merge_aligned_clouds_to_map

EXPORTS = [
    "aicp_hip_create", "aicp_hip_destroy", "aicp_hip_last_error", "aicp_hip_version",
    "aicp_hip_default_config", "aicp_hip_parse_pm_yaml", "aicp_hip_replace_ratio_config_file",
    "aicp_hip_autotune_ratio", "aicp_hip_register", "aicp_hip_register_batch",
    "aicp_hip_overlap", "aicp_hip_overlap_batch", "aicp_hip_align_batch", "aicp_hip_transform", "aicp_hip_crop_box",
    "aicp_hip_batch_upload", "aicp_hip_batch_run", "aicp_hip_batch_free",
    "aicp_hip_last_nn_timing", "aicp_hip_last_phase_ms", "aicp_hip_knn", "aicp_hip_normals",
    "aicp_hip_dists_quantile", "aicp_hip_solve6", "aicp_hip_default_prefilter", "aicp_hip_prefilter",
    "aicp_hip_last_prefilter_stats", "aicp_hip_map_create", "aicp_hip_map_free", "aicp_hip_map_size",
    "aicp_hip_map_download", "aicp_hip_map_crop", "aicp_hip_map_merge", "aicp_hip_map_prefilter",
    "aicp_hip_default_sequence_params", "aicp_hip_sequence_run", "aicp_hip_last_sequence_timing",
    "aicp_hip_map_register_batch", "aicp_hip_multi_create", "aicp_hip_multi_destroy", "aicp_hip_multi_size",
    "aicp_hip_multi_context", "aicp_hip_multi_last_error", "aicp_hip_multi_align_batch",
    "aicp_hip_reference_cache_stats", "aicp_hip_default_options", "aicp_hip_set_options", "aicp_hip_get_options",
    "aicp_hip_test_force_scan_stall", "aicp_hip_sequence_run_raw", "aicp_hip_build_info",
    "aicp_hip_fov_overlap", "aicp_hip_cluster_match", "aicp_hip_alignment_features",
    "aicp_hip_default_risk_params", "aicp_hip_last_risk_stats", "aicp_hip_test_select", "aicp_hip_test_step",
    "aicp_hip_test_step_p2p",
    "aicp_hip_default_monitor_params", "aicp_hip_monitor", "aicp_hip_monitor_batch", "aicp_hip_last_monitor_stats",
    "aicp_hip_default_localization_params", "aicp_hip_localization_window", "aicp_hip_map_sequence_run",
    "aicp_hip_last_localization_timing",
    "aicp_hip_map_align_batch", "aicp_hip_map_capacity", "aicp_hip_default_built_map_params",
    "aicp_hip_built_map_window", "aicp_hip_built_map_sequence_run", "aicp_hip_last_built_map_timing",
    "aicp_hip_map_sequence_run_raw", "aicp_hip_built_map_sequence_run_raw", "aicp_hip_test_ingest",
    "aicp_hip_test_tree", "aicp_hip_test_nn", "aicp_hip_test_normals",
    "aicp_hip_test_overlap", "aicp_hip_test_key_bound",
    "aicp_hip_svm_load", "aicp_hip_svm_free", "aicp_hip_svm_info", "aicp_hip_svm_predict", "aicp_hip_pipeline",
    "aicp_hip_sequence_run_risk",
    "aicp_hip_default_accum_params", "aicp_hip_accum_create", "aicp_hip_accum_free", "aicp_hip_accum_push",
    "aicp_hip_accum_state", "aicp_hip_accum_clear", "aicp_hip_accum_download", "aicp_hip_accum_prefilter",
    "aicp_hip_accum_pose_matrix", "aicp_hip_motion_gate",
    "aicp_hip_session_create", "aicp_hip_session_free", "aicp_hip_session_start", "aicp_hip_session_start_accum",
    "aicp_hip_session_process", "aicp_hip_session_process_accum", "aicp_hip_session_state",
    "aicp_hip_session_reference", "aicp_hip_session_last_timing",
    "aicp_hip_session_create_risk", "aicp_hip_session_start_pose", "aicp_hip_session_start_accum_pose",
    "aicp_hip_session_process_risk", "aicp_hip_session_process_accum_risk", "aicp_hip_session_reference_pose",
    "aicp_hip_map_session_create", "aicp_hip_map_session_free", "aicp_hip_map_session_start",
    "aicp_hip_map_session_process", "aicp_hip_map_session_process_accum", "aicp_hip_map_session_state",
    "aicp_hip_map_session_last_timing",
    "aicp_hip_session_set_monitor", "aicp_hip_session_last_monitor", "aicp_hip_session_monitor_counters",
    "aicp_hip_mapsession_set_monitor", "aicp_hip_mapsession_last_monitor",
    "aicp_hip_mapsession_monitor_counters", "aicp_hip_test_monitor_resident",
    "aicp_hip_mapsession_create_risk", "aicp_hip_mapsession_process_risk", "aicp_hip_mapsession_process_accum_risk",
    "aicp_hip_session_keep_aligned_map", "aicp_hip_session_aligned_map", "aicp_hip_session_take_aligned_map",
    "aicp_hip_mapsession_start_go_back", "aicp_hip_session_start_on_map", "aicp_hip_test_promote_map",
    "aicp_hip_parse_pm_chain", "aicp_hip_chain_uniform", "aicp_hip_chain_filter", "aicp_hip_register_chain",
    "aicp_hip_align_chain_batch", "aicp_hip_test_chain_batch",
]


_NEWEST = {"aicp_hip_reference_cache_stats", "aicp_hip_default_options", "aicp_hip_set_options",
           "aicp_hip_get_options", "aicp_hip_test_force_scan_stall",
           "aicp_hip_sequence_run_raw", "aicp_hip_build_info",  # added in r05 / r06
           "aicp_hip_fov_overlap", "aicp_hip_cluster_match", "aicp_hip_alignment_features",
           "aicp_hip_default_risk_params", "aicp_hip_last_risk_stats",  # the alignment-risk features
           "aicp_hip_test_select", "aicp_hip_test_step",
           "aicp_hip_default_monitor_params", "aicp_hip_monitor", "aicp_hip_monitor_batch",
           "aicp_hip_last_monitor_stats",  # the registration quality monitor
           "aicp_hip_default_localization_params", "aicp_hip_localization_window", "aicp_hip_map_sequence_run",
           "aicp_hip_last_localization_timing",  # the localization stream
           "aicp_hip_map_align_batch", "aicp_hip_map_capacity", "aicp_hip_default_built_map_params",
           "aicp_hip_built_map_window", "aicp_hip_built_map_sequence_run",
           "aicp_hip_last_built_map_timing",  # the built-map localization stream
           "aicp_hip_test_step_p2p",  # the point-to-point chains
           "aicp_hip_map_sequence_run_raw", "aicp_hip_built_map_sequence_run_raw",
           "aicp_hip_test_ingest",  # raw readings in the two map streams
           "aicp_hip_test_tree",  # the kd-tree build, node for node
           "aicp_hip_test_nn",  # the NN search, query by query
           "aicp_hip_test_normals",  # the SurfaceNormal chain, point by point
           "aicp_hip_test_overlap", "aicp_hip_test_key_bound",  # the overlap, set by set
           "aicp_hip_svm_load", "aicp_hip_svm_free", "aicp_hip_svm_info", "aicp_hip_svm_predict",
           "aicp_hip_pipeline", "aicp_hip_sequence_run_risk",  # the classifier and the risk gate
           "aicp_hip_default_accum_params", "aicp_hip_accum_create", "aicp_hip_accum_free", "aicp_hip_accum_push",
           "aicp_hip_accum_state", "aicp_hip_accum_clear", "aicp_hip_accum_download", "aicp_hip_accum_prefilter",
           "aicp_hip_accum_pose_matrix", "aicp_hip_motion_gate",  # the sweep accumulator
           "aicp_hip_session_create", "aicp_hip_session_free", "aicp_hip_session_start",
           "aicp_hip_session_start_accum", "aicp_hip_session_process", "aicp_hip_session_process_accum",
           "aicp_hip_session_state", "aicp_hip_session_reference", "aicp_hip_session_last_timing",  # the live session
           "aicp_hip_map_session_create", "aicp_hip_map_session_free", "aicp_hip_map_session_start",
           "aicp_hip_map_session_process", "aicp_hip_map_session_process_accum", "aicp_hip_map_session_state",
           "aicp_hip_map_session_last_timing",  # the live map sessions
           "aicp_hip_session_create_risk", "aicp_hip_session_start_pose", "aicp_hip_session_start_accum_pose",
           "aicp_hip_session_process_risk", "aicp_hip_session_process_accum_risk",
           "aicp_hip_session_reference_pose",  # the live session with the risk gate
           "aicp_hip_session_set_monitor", "aicp_hip_session_last_monitor", "aicp_hip_session_monitor_counters",
           "aicp_hip_mapsession_set_monitor", "aicp_hip_mapsession_last_monitor",
           "aicp_hip_mapsession_monitor_counters",
           "aicp_hip_test_monitor_resident",  # the quality monitor per reading in the live sessions
           "aicp_hip_mapsession_create_risk", "aicp_hip_mapsession_process_risk",
           "aicp_hip_mapsession_process_accum_risk",  # the live map sessions with the risk gate
           "aicp_hip_session_keep_aligned_map", "aicp_hip_session_aligned_map", "aicp_hip_session_take_aligned_map",
           "aicp_hip_mapsession_start_go_back", "aicp_hip_session_start_on_map",
           "aicp_hip_test_promote_map",  # the mapping session's built map, the go-back, the start on a map
           "aicp_hip_parse_pm_chain", "aicp_hip_chain_uniform", "aicp_hip_chain_filter",
           "aicp_hip_register_chain",  # the sampled chains
           "aicp_hip_align_chain_batch", "aicp_hip_test_chain_batch"}  # and their batch form


class IcpConfig(C.Structure):
    _fields_ = [
        ("knn_normals", C.c_int32),
        ("nn_epsilon", C.c_float),
        ("nn_max_dist", C.c_float),
        ("trimmed_ratio", C.c_float),
        ("max_iter", C.c_int32),
        ("min_diff_rot", C.c_float),
        ("min_diff_trans", C.c_float),
        ("smooth_length", C.c_int32),
        ("bucket_size", C.c_int32),
        ("knn_match", C.c_int32),
    ]


class IcpStats(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("iterations", C.c_int32),
        ("converged", C.c_int32),
        ("degenerate_normals", C.c_int32),
        ("inlier_ratio", C.c_float),
        ("trimmed_ratio", C.c_float),
        ("overlap_percent", C.c_float),
        ("tree_depth", C.c_int32),
        ("nn_points_touched", C.c_uint64),
        ("nn_nodes_touched", C.c_uint64),
        ("overlap_keys", C.c_uint64 * 3),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "overlap_keys"}
        d["overlap_keys"] = [int(x) for x in self.overlap_keys]
        return d


class Pair(C.Structure):
    _fields_ = [
        ("ref", C.POINTER(C.c_float)),
        ("n_ref", C.c_uint64),
        ("ref_stride", C.c_uint64),
        ("read", C.POINTER(C.c_float)),
        ("n_read", C.c_uint64),
        ("read_stride", C.c_uint64),
        ("init_T", C.POINTER(C.c_float)),
        ("ref_origin", C.c_double * 3),
        ("read_origin", C.c_double * 3),
    ]


AICP_CHAIN_MAX_FILTERS = 4
AICP_CHAIN_REFERENCE, AICP_CHAIN_READING = 0, 1
AICP_FILTER_NONE, AICP_FILTER_SURFACE_NORMAL, AICP_FILTER_MIN_DIST = 0, 1, 2
AICP_FILTER_RANDOM_SAMPLING, AICP_FILTER_MAX_DENSITY = 3, 4
AICP_OUTLIER_TRIMMED_DIST, AICP_OUTLIER_MAX_DIST = 0, 1


class ChainFilter(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("knn", C.c_int32),
        ("keep_densities", C.c_int32),
        ("dim", C.c_int32),
        ("min_dist", C.c_float),
        ("prob", C.c_float),
        ("max_density", C.c_float),
        ("pad", C.c_int32),
    ]


class Chain(C.Structure):
    """aicp_chain: per side (reference, reading) a list of at most 4 data-point filters, the
    outlier rule and the draws' seed. Chain() is "no filters, TrimmedDist"."""
    _fields_ = [
        ("filters", (ChainFilter * AICP_CHAIN_MAX_FILTERS) * 2),
        ("n_filters", C.c_int32 * 2),
        ("outlier", C.c_int32),
        ("outlier_limit_d2", C.c_float),
        ("seed", C.c_uint64),
    ]

    def add(self, side, kind, **kw):
        """Appends a filter to a side's list: libpointmatcher's defaults, then the keywords."""
        n = self.n_filters[side]
        if n >= AICP_CHAIN_MAX_FILTERS:
            raise ValueError("at most 4 filters on a side")
        f = self.filters[side][n]
        f.kind, f.knn, f.keep_densities, f.dim = kind, 5, 0, -1
        f.min_dist, f.prob, f.max_density = 1.0, 0.75, 10.0
        for k, v in kw.items():
            if not hasattr(f, k):
                raise AttributeError(f"aicp_chain_filter has no field {k}")
            setattr(f, k, v)
        self.n_filters[side] = n + 1
        return self

    def side(self, side):
        """The side's list as dicts: the kind and the parameters that kind reads."""
        names = {AICP_FILTER_SURFACE_NORMAL: ("knn", "keep_densities"), AICP_FILTER_MIN_DIST: ("dim", "min_dist"),
                 AICP_FILTER_RANDOM_SAMPLING: ("prob",), AICP_FILTER_MAX_DENSITY: ("max_density",)}
        out = []
        for q in range(self.n_filters[side]):
            f = self.filters[side][q]
            out.append(dict(kind=f.kind, **{k: getattr(f, k) for k in names.get(f.kind, ())}))
        return out


class ChainStats(C.Structure):
    _fields_ = [
        ("n_in", C.c_uint64 * 2),
        ("n_out", (C.c_uint64 * AICP_CHAIN_MAX_FILTERS) * 2),
        ("n_kept", C.c_uint64 * 2),
    ]

    def as_dict(self):
        return {"n_in": [int(x) for x in self.n_in], "n_out": [[int(x) for x in row] for row in self.n_out],
                "n_kept": [int(x) for x in self.n_kept]}


class PrefilterParams(C.Structure):
    _fields_ = [
        ("leaf_size", C.c_float),
        ("normal_k", C.c_int32),
        ("neighbours", C.c_int32),
        ("min_cluster_size", C.c_int32),
        ("max_cluster_size", C.c_int32),
        ("smoothness_rad", C.c_float),
        ("curvature_threshold", C.c_float),
        ("viewpoint", C.c_float * 3),
    ]


class PrefilterStats(C.Structure):
    _fields_ = [
        ("voxel_ms", C.c_double),
        ("normals_ms", C.c_double),
        ("segment_ms", C.c_double),
        ("device_ms", C.c_double),
        ("wall_ms", C.c_double),
        ("knn_ms", C.c_double),
        ("knn_queries", C.c_uint64),
        ("knn_points_touched", C.c_uint64),
        ("knn_nodes_touched", C.c_uint64),
        ("propagation_passes", C.c_int32),
        ("pad", C.c_int32),
    ]


class RiskParams(C.Structure):
    """aicp_risk_params (include/aicp_hip.h)."""
    _fields_ = [
        ("range", C.c_float),
        ("angular_view", C.c_float),
        ("max_angle_deg", C.c_float),
        ("box_scale", C.c_float * 3),
        ("prefilter", PrefilterParams),
    ]


class RiskBox(C.Structure):
    _fields_ = [("centre", C.c_double * 3), ("rot", C.c_double * 9), ("half", C.c_double * 3)]


class RiskResult(C.Structure):
    _fields_ = [
        ("fov_overlap", C.c_float),
        ("alignability", C.c_float),
        ("accepted_a", C.c_uint64),
        ("accepted_b", C.c_uint64),
        ("sampled_a", C.c_uint32),
        ("sampled_b", C.c_uint32),
        ("clusters_a", C.c_int32),
        ("clusters_b", C.c_int32),
        ("n_matches", C.c_int32),
        ("pad", C.c_int32),
        ("eigenvalues", C.c_double * 3),
        ("eigenvectors", C.c_double * 9),
        ("centroid", C.c_double * 3),
    ]


class RiskStats(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fov_ms", "prefilter_a_ms", "prefilter_b_ms", "clusters_ms", "counts_ms",
                                          "match_ms", "device_ms", "wall_ms")]


class MonitorParams(C.Structure):
    """aicp_monitor_params (include/aicp_hip.h)."""
    _fields_ = [("quantile", C.c_float), ("max_accepted_dist", C.c_double), ("flags", C.c_int32)]


class MonitorResult(C.Structure):
    """aicp_monitor_result: 56 bytes without implicit padding, so bytes(result) compares results."""
    _fields_ = [
        ("hausdorff", C.c_float),
        ("hausdorff_quantile", C.c_float),
        ("max_d2", C.c_float * 2),
        ("quantile_d2", C.c_float * 2),
        ("knn_mean_dist", C.c_float),
        ("pad", C.c_int32),
        ("knn_valid", C.c_uint64),
        ("paired_mean_dist", C.c_float),
        ("paired_limit_d2", C.c_float),
        ("paired_kept", C.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("pad", "max_d2", "quantile_d2")}
        d["max_d2"] = [float(x) for x in self.max_d2]
        d["quantile_d2"] = [float(x) for x in self.quantile_d2]
        d["bytes"] = bytes(self)
        return d


class MonitorStats(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("trees_ms", "nn_ms", "reduce_ms", "device_ms", "wall_ms")]


class TestOverlapOut(C.Structure):
    """aicp_test_overlap_out: what ran, and the caller's arrays the entry fills."""
    _ip, _up = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    _fields_ = [
        ("path", C.c_int32), ("filter", C.c_int32), ("wide", C.c_int32), ("n_groups", C.c_int32),
        ("pair_group", _ip), ("cloud_keys", _up), ("cloud_err", _ip), ("cloud_bbox", _ip),
        ("pair_counts", _up), ("pair_percent", C.POINTER(C.c_float)), ("pair_ratio", C.POINTER(C.c_float)),
        ("pair_err", _ip), ("desc_min", _ip), ("desc_dim", _ip), ("desc_off", _up), ("desc_bytes", _up),
        ("arena", C.POINTER(C.c_uint8)), ("arena_cap", C.c_uint64), ("arena_bytes", C.c_uint64),
        ("key_counts", C.POINTER(C.c_uint32)), ("key_offsets", _up), ("points_cap", C.c_uint64),
        ("n_points", C.c_uint64), ("words", _up), ("words_cap", C.c_uint64), ("n_words", C.c_uint64),
        ("cloud_bound", _up), ("list_off", _up), ("list_cap", _up), ("dirty", C.c_uint64),
    ]


class Cloud(C.Structure):
    _fields_ = [
        ("pts", C.POINTER(C.c_float)),
        ("n", C.c_uint64),
        ("stride", C.c_uint64),
        ("origin", C.c_double * 3),
    ]


class SequenceParams(C.Structure):
    _fields_ = [
        ("reference_update_frequency", C.c_int32),
        ("max_correction_magnitude", C.c_float),
        ("resolution", C.c_double),
        ("flags", C.c_int32),
    ]


class SequenceResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("accepted", C.c_int32),
        ("reference", C.c_int32),
        ("is_reference", C.c_int32),
        ("corrected_origin", C.c_double * 3),
        ("icp", IcpStats),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("status", "accepted", "reference", "is_reference")}
        d["corrected_origin"] = [float(x) for x in self.corrected_origin]
        d["icp"] = self.icp.as_dict()
        return d


class SvmInfo(C.Structure):
    """aicp_svm_info (include/aicp_hip.h)."""
    _fields_ = [
        ("format", C.c_int32),
        ("var_count", C.c_int32),
        ("class_count", C.c_int32),
        ("sv_total", C.c_int32),
        ("sv_count", C.c_int32),
        ("has_index", C.c_int32),
        ("degree", C.c_double),
        ("gamma", C.c_double),
        ("coef0", C.c_double),
        ("rho", C.c_double),
    ]


class PipelineRecord(C.Structure):
    """aicp_pipeline_record (include/aicp_hip.h)."""
    _fields_ = [
        ("n_read", C.c_uint64),
        ("fov_overlap", C.c_float),
        ("octree_overlap", C.c_float),
        ("alignability", C.c_float),
        ("raw", C.c_float),
        ("risk", C.c_double),
        ("registered", C.c_int32),
        ("trimmed_ratio", C.c_float),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Options(C.Structure):
    """aicp_hip_options (include/aicp_hip.h): a context's engine and schedule switches."""
    _fields_ = [
        ("profile", C.c_int32),
        ("nn_engine", C.c_int32),
        ("overlap_path", C.c_int32),
        ("normals_knn_engine", C.c_int32),
        ("select_pair", C.c_int32),
        ("select_fused_from", C.c_int32),
        ("raw_tree_first", C.c_int32),
        ("raw_first_at", C.c_int32),
        ("no_early_exit", C.c_int32),
        ("tree_plan", C.c_int32),
        ("tree_lvl_min", C.c_uint32),
        ("reference_cache", C.c_int32),
        ("oneshot_keep_mib", C.c_uint32),
        ("early_reference", C.c_int32),
        ("read_order_min", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SequenceTiming(C.Structure):
    _fields_ = [
        ("windows", C.c_int32),
        ("replans", C.c_int32),
        ("wall_ms", C.c_double),
        ("device_ms", C.c_double),
    ]


class LocalizationParams(C.Structure):
    """aicp_localization_params: App's localization stream on the prior map."""
    _fields_ = [
        ("reference_update_frequency", C.c_int32),
        ("map_refilter_every", C.c_int32),
        ("max_correction_magnitude", C.c_float),
        ("crop_min", C.c_float),
        ("crop_max", C.c_float),
        ("flags", C.c_int32),
    ]


class LocalizationResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("accepted", C.c_int32),
        ("merged", C.c_int32),
        ("refiltered", C.c_int32),
        ("map_points", C.c_uint64),
        ("crop_points", C.c_uint64),
        ("corrected_origin", C.c_double * 3),
        ("icp", IcpStats),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("status", "accepted", "merged", "refiltered", "map_points", "crop_points")}
        d["corrected_origin"] = [float(x) for x in self.corrected_origin]
        d["icp"] = self.icp.as_dict()
        return d


class LocalizationTiming(C.Structure):
    _fields_ = [
        ("windows", C.c_int32),
        ("merges", C.c_int32),
        ("refilters", C.c_int32),
        ("pad", C.c_int32),
        ("wall_ms", C.c_double),
        ("device_ms", C.c_double),
    ]


class BuiltMapParams(C.Structure):
    """aicp_built_map_params: App's localization stream on the map it has built itself."""
    _fields_ = [
        ("reference_update_frequency", C.c_int32),
        ("max_correction_magnitude", C.c_float),
        ("crop_min", C.c_float),
        ("crop_max", C.c_float),
        ("resolution", C.c_double),
        ("flags", C.c_int32),
        ("pad", C.c_int32),
    ]


class BuiltMapResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("accepted", C.c_int32),
        ("is_reference", C.c_int32),
        ("pad", C.c_int32),
        ("map_points", C.c_uint64),
        ("crop_points", C.c_uint64),
        ("corrected_origin", C.c_double * 3),
        ("icp", IcpStats),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("status", "accepted", "is_reference", "map_points", "crop_points")}
        d["corrected_origin"] = [float(x) for x in self.corrected_origin]
        d["icp"] = self.icp.as_dict()
        return d


class BuiltMapTiming(C.Structure):
    _fields_ = [
        ("windows", C.c_int32),
        ("appends", C.c_int32),
        ("wall_ms", C.c_double),
        ("device_ms", C.c_double),
    ]


class AccumParams(C.Structure):
    _fields_ = [
        ("batch_size", C.c_int32),
        ("crop_min", C.c_float),
        ("crop_max", C.c_float),
    ]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        # (an AICP_HIP_LIB override may be an older build in an A/B run: the newest entry points only)
        if not hasattr(L, name) and not (os.environ.get("AICP_HIP_LIB") and name in _NEWEST):
            raise ImportError(f"{LIB_PATH} does not export {name}")
    vp = C.c_void_p
    fp = C.POINTER(C.c_float)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    up = C.POINTER(C.c_uint64)
    cfgp = C.POINTER(IcpConfig)
    stp = C.POINTER(IcpStats)
    pp = C.POINTER(Pair)
    sz = C.c_size_t
    L.aicp_hip_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.aicp_hip_destroy.argtypes = [vp]
    L.aicp_hip_destroy.restype = None
    L.aicp_hip_last_error.argtypes = [vp]
    L.aicp_hip_last_error.restype = C.c_char_p
    L.aicp_hip_version.restype = C.c_char_p
    if hasattr(L, "aicp_hip_build_info"):
        L.aicp_hip_build_info.restype = C.c_char_p
    L.aicp_hip_default_config.argtypes = [cfgp]
    L.aicp_hip_default_config.restype = None
    L.aicp_hip_parse_pm_yaml.argtypes = [C.c_char_p, cfgp]
    if hasattr(L, "aicp_hip_parse_pm_chain"):
        chp = C.POINTER(Chain)
        L.aicp_hip_parse_pm_chain.argtypes = [C.c_char_p, cfgp, chp]
        L.aicp_hip_chain_uniform.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.aicp_hip_chain_uniform.restype = C.c_float
        L.aicp_hip_chain_filter.argtypes = [vp, chp, C.c_int, fp, sz, sz, up, up, ip, fp, fp]
        L.aicp_hip_register_chain.argtypes = [vp, cfgp, chp, pp, fp, stp, C.POINTER(ChainStats)]
    if hasattr(L, "aicp_hip_align_chain_batch"):
        L.aicp_hip_align_chain_batch.argtypes = [vp, cfgp, C.POINTER(Chain), pp, sz, C.c_double, C.c_int, fp, stp,
                                                 C.POINTER(ChainStats)]
        L.aicp_hip_test_chain_batch.argtypes = [vp, C.POINTER(Chain), C.c_int32, sz, C.POINTER(C.c_uint32), fp, up, up,
                                                ip, fp, fp]
    L.aicp_hip_replace_ratio_config_file.argtypes = [C.c_char_p, C.c_char_p, C.c_float]
    L.aicp_hip_autotune_ratio.argtypes = [C.c_float]
    L.aicp_hip_autotune_ratio.restype = C.c_float
    L.aicp_hip_register.argtypes = [vp, cfgp, pp, fp, stp]
    L.aicp_hip_register_batch.argtypes = [vp, cfgp, pp, sz, fp, stp]
    L.aicp_hip_overlap.argtypes = [vp, pp, C.c_double, fp]
    L.aicp_hip_overlap_batch.argtypes = [vp, pp, sz, C.c_double, fp, stp]
    L.aicp_hip_align_batch.argtypes = [vp, cfgp, pp, sz, C.c_double, C.c_int, fp, stp]
    L.aicp_hip_transform.argtypes = [vp, fp, fp, sz, sz, fp]
    L.aicp_hip_crop_box.argtypes = [vp, fp, sz, sz, C.c_float, C.c_float, fp, fp, C.POINTER(C.c_size_t), fp]
    L.aicp_hip_batch_upload.argtypes = [vp, pp, sz, C.POINTER(vp)]
    L.aicp_hip_batch_run.argtypes = [vp, vp, cfgp, C.c_double, C.c_int, fp, stp]
    L.aicp_hip_batch_free.argtypes = [vp, vp]
    L.aicp_hip_batch_free.restype = None
    L.aicp_hip_last_nn_timing.argtypes = [vp, C.POINTER(C.c_int), dp, dp, up]
    L.aicp_hip_last_phase_ms.argtypes = [vp, dp]
    L.aicp_hip_knn.argtypes = [vp, fp, sz, sz, fp, sz, sz, C.c_int, C.c_float, C.c_float, ip, fp, up]
    L.aicp_hip_normals.argtypes = [vp, fp, sz, sz, C.c_int, fp, ip]
    L.aicp_hip_dists_quantile.argtypes = [vp, fp, sz, C.c_float, fp]
    L.aicp_hip_solve6.argtypes = [vp, dp, dp, dp, ip]
    L.aicp_hip_default_prefilter.argtypes = [C.POINTER(PrefilterParams)]
    L.aicp_hip_default_prefilter.restype = None
    L.aicp_hip_prefilter.argtypes = [vp, C.POINTER(PrefilterParams), fp, sz, sz, fp, C.POINTER(C.c_size_t), fp, ip,
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.aicp_hip_last_prefilter_stats.argtypes = [vp, C.POINTER(PrefilterStats)]
    szp = C.POINTER(C.c_size_t)
    L.aicp_hip_map_create.argtypes = [vp, fp, sz, sz, C.POINTER(vp)]
    L.aicp_hip_map_free.argtypes = [vp, vp]
    L.aicp_hip_map_free.restype = None
    L.aicp_hip_map_size.argtypes = [vp, szp]
    L.aicp_hip_map_download.argtypes = [vp, vp, fp, sz, szp]
    L.aicp_hip_map_crop.argtypes = [vp, vp, C.c_float, C.c_float, fp, fp, sz, szp]
    L.aicp_hip_map_merge.argtypes = [vp, vp, fp, sz, sz, fp]
    L.aicp_hip_map_prefilter.argtypes = [vp, vp, C.POINTER(PrefilterParams)]
    L.aicp_hip_default_sequence_params.argtypes = [C.POINTER(SequenceParams)]
    L.aicp_hip_default_sequence_params.restype = None
    L.aicp_hip_sequence_run.argtypes = [vp, cfgp, C.POINTER(SequenceParams), C.POINTER(Cloud), C.POINTER(Cloud), sz,
                                        fp, C.POINTER(SequenceResult), C.POINTER(C.c_size_t)]
    L.aicp_hip_last_sequence_timing.argtypes = [vp, C.POINTER(SequenceTiming)]
    if hasattr(L, "aicp_hip_sequence_run_raw"):
        L.aicp_hip_sequence_run_raw.argtypes = [vp, cfgp, C.POINTER(SequenceParams), C.POINTER(PrefilterParams),
                                                C.POINTER(Cloud), C.POINTER(Cloud), sz, fp, C.POINTER(SequenceResult),
                                                C.POINTER(C.c_size_t)]
    L.aicp_hip_map_register_batch.argtypes = [vp, cfgp, vp, C.c_float, C.c_float, C.POINTER(Cloud), fp, sz, C.c_int,
                                              fp, stp]
    if hasattr(L, "aicp_hip_reference_cache_stats"):
        L.aicp_hip_reference_cache_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "aicp_hip_set_options"):
        L.aicp_hip_default_options.argtypes = [C.POINTER(Options)]
        L.aicp_hip_default_options.restype = None
        L.aicp_hip_set_options.argtypes = [vp, C.POINTER(Options)]
        L.aicp_hip_get_options.argtypes = [vp, C.POINTER(Options)]
        L.aicp_hip_test_force_scan_stall.argtypes = [C.c_int]
    L.aicp_hip_multi_create.argtypes = [ip, C.c_int, C.POINTER(vp)]
    L.aicp_hip_multi_destroy.argtypes = [vp]
    L.aicp_hip_multi_destroy.restype = None
    L.aicp_hip_multi_size.argtypes = [vp]
    L.aicp_hip_multi_context.argtypes = [vp, C.c_int]
    L.aicp_hip_multi_context.restype = vp
    L.aicp_hip_multi_last_error.argtypes = [vp]
    L.aicp_hip_multi_last_error.restype = C.c_char_p
    L.aicp_hip_multi_align_batch.argtypes = [vp, cfgp, pp, sz, C.c_double, C.c_int, fp, stp, ip]
    if hasattr(L, "aicp_hip_alignment_features"):
        clp = C.POINTER(Cloud)
        u32p = C.POINTER(C.c_uint32)
        boxp = C.POINTER(RiskBox)
        L.aicp_hip_default_risk_params.argtypes = [C.POINTER(RiskParams)]
        L.aicp_hip_default_risk_params.restype = None
        L.aicp_hip_fov_overlap.argtypes = [vp, clp, clp, dp, dp, C.c_float, C.c_float, fp, fp, szp, fp, szp]
        L.aicp_hip_cluster_match.argtypes = [vp, fp, ip, sz, fp, ip, sz, C.c_float, fp, fp, ip, ip, fp, fp, dp, dp, dp,
                                             boxp, boxp, u32p, u32p]
        L.aicp_hip_alignment_features.argtypes = [vp, C.POINTER(RiskParams), clp, clp, dp, dp, C.POINTER(RiskResult),
                                                  fp, szp, fp, szp, sz]
        L.aicp_hip_last_risk_stats.argtypes = [vp, C.POINTER(RiskStats)]
    if hasattr(L, "aicp_hip_monitor"):
        clp = C.POINTER(Cloud)
        mpp, mrp = C.POINTER(MonitorParams), C.POINTER(MonitorResult)
        L.aicp_hip_default_monitor_params.argtypes = [mpp]
        L.aicp_hip_default_monitor_params.restype = None
        L.aicp_hip_monitor.argtypes = [vp, mpp, cfgp, clp, clp, fp, mrp, fp, fp]
        L.aicp_hip_monitor_batch.argtypes = [vp, mpp, cfgp, pp, sz, fp, mrp]
        L.aicp_hip_last_monitor_stats.argtypes = [vp, C.POINTER(MonitorStats)]
    if hasattr(L, "aicp_hip_map_sequence_run"):
        lpp = C.POINTER(LocalizationParams)
        L.aicp_hip_default_localization_params.argtypes = [lpp]
        L.aicp_hip_default_localization_params.restype = None
        L.aicp_hip_localization_window.argtypes = [C.c_uint64, lpp, sz]
        L.aicp_hip_localization_window.restype = sz
        L.aicp_hip_map_sequence_run.argtypes = [vp, cfgp, lpp, C.POINTER(PrefilterParams), vp, C.POINTER(Cloud), fp, sz,
                                                fp, C.POINTER(LocalizationResult), szp]
        L.aicp_hip_last_localization_timing.argtypes = [vp, C.POINTER(LocalizationTiming)]
    if hasattr(L, "aicp_hip_built_map_sequence_run"):
        bpp = C.POINTER(BuiltMapParams)
        L.aicp_hip_map_align_batch.argtypes = [vp, cfgp, vp, C.c_float, C.c_float, C.POINTER(Cloud), fp, sz, C.c_double,
                                               C.c_int, fp, stp]
        L.aicp_hip_map_capacity.argtypes = [vp, szp]
        L.aicp_hip_default_built_map_params.argtypes = [bpp]
        L.aicp_hip_default_built_map_params.restype = None
        L.aicp_hip_built_map_window.argtypes = [C.c_uint64, bpp, sz]
        L.aicp_hip_built_map_window.restype = sz
        L.aicp_hip_built_map_sequence_run.argtypes = [vp, cfgp, bpp, vp, C.POINTER(Cloud), fp, sz, fp,
                                                      C.POINTER(BuiltMapResult), szp]
        L.aicp_hip_last_built_map_timing.argtypes = [vp, C.POINTER(BuiltMapTiming)]
    if hasattr(L, "aicp_hip_test_select"):
        u32p = C.POINTER(C.c_uint32)
        L.aicp_hip_test_select.argtypes = [vp, sz, u32p, fp, C.POINTER(C.c_uint8), sz, ip, fp, fp, ip, ip, u32p, u32p,
                                           up]
    if hasattr(L, "aicp_hip_test_step"):
        u32p, u8p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        L.aicp_hip_test_step.argtypes = [vp, sz, u32p, u32p, u32p, sz, fp, fp, fp, fp, u8p, C.c_int32, C.c_int32,
                                         C.c_float, C.c_float, sz, fp, ip, fp, u32p, dp, fp, ip, fp, up, dp, up]
    if hasattr(L, "aicp_hip_test_step_p2p"):  # (aicp_hip_test_step's without ref_nrm)
        u32p, u8p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        L.aicp_hip_test_step_p2p.argtypes = [vp, sz, u32p, u32p, u32p, sz, fp, fp, fp, u8p, C.c_int32, C.c_int32,
                                             C.c_float, C.c_float, sz, fp, ip, fp, u32p, dp, fp, ip, fp, up, dp, up]
    if hasattr(L, "aicp_hip_map_sequence_run_raw"):  # (the pre-filtered streams' plus pf_read and out_kept)
        u32p, pfp, clp = C.POINTER(C.c_uint32), C.POINTER(PrefilterParams), C.POINTER(Cloud)
        L.aicp_hip_map_sequence_run_raw.argtypes = [vp, cfgp, C.POINTER(LocalizationParams), pfp, pfp, vp, clp, fp, sz,
                                                    fp, C.POINTER(LocalizationResult), u32p, szp]
        L.aicp_hip_built_map_sequence_run_raw.argtypes = [vp, cfgp, C.POINTER(BuiltMapParams), pfp, vp, clp, fp, sz, fp,
                                                          C.POINTER(BuiltMapResult), u32p, szp]
        L.aicp_hip_test_ingest.argtypes = [vp, fp, sz, sz, fp, fp]
    if hasattr(L, "aicp_hip_test_tree"):
        u32p = C.POINTER(C.c_uint32)
        L.aicp_hip_test_tree.argtypes = [vp, sz, u32p, fp, C.c_int32, C.c_int32, u32p, u32p, ip, fp, u32p, fp, u32p]
    if hasattr(L, "aicp_hip_test_nn"):
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        L.aicp_hip_test_nn.argtypes = [vp, sz, u32p, fp, C.c_int32, sz, u32p, u32p, fp, sz, fp, u8p, C.c_float,
                                       C.c_float, ip, fp, u32p, ip, ip, up]
    if hasattr(L, "aicp_hip_test_normals"):
        u32p = C.POINTER(C.c_uint32)
        L.aicp_hip_test_normals.argtypes = [vp, sz, u32p, fp, C.c_int32, C.c_int32, ip, ip, ip, fp, ip, up, fp, ip, ip, up]
    if hasattr(L, "aicp_hip_test_overlap"):
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        L.aicp_hip_test_overlap.argtypes = [vp, sz, u32p, fp, sz, u32p, u32p, fp, dp, dp, C.c_double, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_int32, up, C.c_int32, C.POINTER(TestOverlapOut)]
        L.aicp_hip_test_key_bound.argtypes = [fp, sz, dp, C.c_double, C.c_int32, up, up]
    if hasattr(L, "aicp_hip_svm_load"):
        dp, clp, pfp = C.POINTER(C.c_double), C.POINTER(Cloud), C.POINTER(PrefilterParams)
        rpp, prp = C.POINTER(RiskParams), C.POINTER(PipelineRecord)
        L.aicp_hip_svm_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.aicp_hip_svm_free.argtypes = [vp]
        L.aicp_hip_svm_free.restype = None
        L.aicp_hip_svm_info.argtypes = [vp, C.POINTER(SvmInfo), fp, dp, ip]
        L.aicp_hip_svm_predict.argtypes = [vp, vp, fp, sz, fp, dp]
        L.aicp_hip_pipeline.argtypes = [vp, cfgp, rpp, vp, C.c_double, pp, dp, dp, C.c_double, fp, prp, stp]
        L.aicp_hip_sequence_run_risk.argtypes = [vp, cfgp, C.POINTER(SequenceParams), pfp, rpp, vp, C.c_double, clp, dp,
                                                 clp, dp, sz, fp, C.POINTER(SequenceResult), prp, szp]
    if hasattr(L, "aicp_hip_accum_create"):
        u32p, dp, pfp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(PrefilterParams)
        L.aicp_hip_default_accum_params.argtypes = [C.POINTER(AccumParams)]
        L.aicp_hip_default_accum_params.restype = None
        L.aicp_hip_accum_create.argtypes = [vp, C.POINTER(AccumParams), sz, C.POINTER(vp)]
        L.aicp_hip_accum_free.argtypes = [vp, vp]
        L.aicp_hip_accum_free.restype = None
        L.aicp_hip_accum_push.argtypes = [vp, vp, fp, sz, sz, dp]
        L.aicp_hip_accum_state.argtypes = [vp, vp, ip, ip, szp, u32p]
        L.aicp_hip_accum_clear.argtypes = [vp, vp]
        L.aicp_hip_accum_download.argtypes = [vp, vp, fp, sz, szp]
        L.aicp_hip_accum_prefilter.argtypes = [vp, vp, pfp, fp, fp, sz, szp]
        L.aicp_hip_accum_pose_matrix.argtypes = [dp, fp]
        L.aicp_hip_accum_pose_matrix.restype = None
        L.aicp_hip_motion_gate.argtypes = [dp, dp, C.c_double, C.c_double]
    if hasattr(L, "aicp_hip_session_create"):
        u32p, dp, clp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(Cloud)
        srp = C.POINTER(SequenceResult)
        L.aicp_hip_session_create.argtypes = [vp, cfgp, C.POINTER(SequenceParams), C.POINTER(PrefilterParams),
                                              C.POINTER(vp)]
        L.aicp_hip_session_free.argtypes = [vp, vp]
        L.aicp_hip_session_free.restype = None
        L.aicp_hip_session_start.argtypes = [vp, vp, clp]
        L.aicp_hip_session_start_accum.argtypes = [vp, vp, vp, dp]
        L.aicp_hip_session_process.argtypes = [vp, vp, clp, fp, srp, u32p]
        L.aicp_hip_session_process_accum.argtypes = [vp, vp, vp, dp, fp, srp, u32p]
        L.aicp_hip_session_state.argtypes = [vp, vp, up, ip, szp, fp, ip]
        L.aicp_hip_session_reference.argtypes = [vp, vp, fp, sz, szp, dp]
        L.aicp_hip_session_last_timing.argtypes = [vp, dp, dp]
    if hasattr(L, "aicp_hip_session_create_risk"):
        u32p, dp, clp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(Cloud)
        srp, prp = C.POINTER(SequenceResult), C.POINTER(PipelineRecord)
        L.aicp_hip_session_create_risk.argtypes = [vp, cfgp, C.POINTER(SequenceParams), C.POINTER(PrefilterParams),
                                                   C.POINTER(RiskParams), vp, C.c_double, C.POINTER(vp)]
        L.aicp_hip_session_start_pose.argtypes = [vp, vp, clp, dp]
        L.aicp_hip_session_start_accum_pose.argtypes = [vp, vp, vp, dp]
        L.aicp_hip_session_process_risk.argtypes = [vp, vp, clp, dp, fp, srp, prp, u32p]
        L.aicp_hip_session_process_accum_risk.argtypes = [vp, vp, vp, dp, fp, srp, prp, u32p]
        L.aicp_hip_session_reference_pose.argtypes = [vp, vp, dp]
    if hasattr(L, "aicp_hip_map_session_create"):  # (out: LocalizationResult or BuiltMapResult, one layout)
        u32p, dp, clp, pfp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(Cloud), C.POINTER(PrefilterParams)
        L.aicp_hip_map_session_create.argtypes = [vp, cfgp, C.POINTER(LocalizationParams), C.POINTER(BuiltMapParams),
                                                  pfp, pfp, C.POINTER(vp)]
        L.aicp_hip_map_session_free.argtypes = [vp, vp]
        L.aicp_hip_map_session_free.restype = None
        L.aicp_hip_map_session_start.argtypes = [vp, vp, vp]
        L.aicp_hip_map_session_process.argtypes = [vp, vp, clp, fp, fp, vp, u32p]
        L.aicp_hip_map_session_process_accum.argtypes = [vp, vp, vp, fp, fp, vp, u32p]
        L.aicp_hip_map_session_state.argtypes = [vp, vp, up, ip, fp, ip]
        L.aicp_hip_map_session_last_timing.argtypes = [vp, dp, dp]
    if hasattr(L, "aicp_hip_mapsession_create_risk"):  # (out: as aicp_hip_map_session_process)
        u32p, dp, clp, pfp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(Cloud), C.POINTER(PrefilterParams)
        prp = C.POINTER(PipelineRecord)
        L.aicp_hip_mapsession_create_risk.argtypes = [vp, cfgp, C.POINTER(LocalizationParams),
                                                      C.POINTER(BuiltMapParams), pfp, pfp, C.POINTER(RiskParams), vp,
                                                      C.c_double, C.POINTER(vp)]
        L.aicp_hip_mapsession_process_risk.argtypes = [vp, vp, clp, dp, fp, vp, prp, u32p]
        L.aicp_hip_mapsession_process_accum_risk.argtypes = [vp, vp, vp, dp, fp, vp, prp, u32p]
    if hasattr(L, "aicp_hip_session_keep_aligned_map"):
        L.aicp_hip_session_keep_aligned_map.argtypes = [vp, vp, C.c_int]
        L.aicp_hip_session_aligned_map.argtypes = [vp, vp, C.POINTER(vp)]
        L.aicp_hip_session_take_aligned_map.argtypes = [vp, vp, C.POINTER(vp)]
        L.aicp_hip_mapsession_start_go_back.argtypes = [vp, vp, vp, vp]
        L.aicp_hip_session_start_on_map.argtypes = [vp, vp, vp, fp, C.c_float, C.c_float]
        L.aicp_hip_test_promote_map.argtypes = [vp, C.c_int32, fp, sz, sz, C.c_int32, vp, fp, fp, up]
    if hasattr(L, "aicp_hip_session_set_monitor"):
        mpp, mrp = C.POINTER(MonitorParams), C.POINTER(MonitorResult)
        for kind in ("session", "mapsession"):
            getattr(L, f"aicp_hip_{kind}_set_monitor").argtypes = [vp, vp, mpp]
            getattr(L, f"aicp_hip_{kind}_last_monitor").argtypes = [vp, mrp, ip]
            getattr(L, f"aicp_hip_{kind}_monitor_counters").argtypes = [vp, up]
        L.aicp_hip_test_monitor_resident.argtypes = [vp, mpp, cfgp, fp, sz, fp, sz, fp, C.c_int32, mrp, up, up]
    return L


lib = _load()


def build_info() -> str:
    """The loaded library's provenance line (aicp_hip_build_info): "src <hash> arch <gfx> extra
    <flags>", or "" for a library older than the call."""
    return lib.aicp_hip_build_info().decode() if hasattr(lib, "aicp_hip_build_info") else ""


def source_hash(csrc: str = os.path.join(PKG_DIR, "csrc")) -> str:
    """The hash the Makefile embeds: sha256 over its SRCS_HIP, SRCS_CPP and HDRS files and the
    Makefile itself, in that order (first 16 hex digits)."""
    mk = os.path.join(csrc, "Makefile")
    lists = {}
    text = open(mk).read().replace("\\\n", " ")
    for line in text.splitlines():
        for key in ("SRCS_HIP", "SRCS_CPP", "HDRS"):
            if line.startswith(key + " ="):
                lists[key] = line.split("=", 1)[1].split()
    h = hashlib.sha256()
    for f in lists["SRCS_HIP"] + lists["SRCS_CPP"] + lists["HDRS"] + ["Makefile"]:
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def provenance() -> dict:
    """Whether the loaded library was built from this tree's sources (bench lines carry it)."""
    info = build_info()
    src = info.split()[1] if info.startswith("src ") else ""
    try:
        tree = source_hash()
    except OSError:
        tree = ""
    return {"library": os.path.abspath(LIB_PATH), "build_info": info, "tree_source_hash": tree,
            "built_from_tree": bool(src) and src == tree}


class AicpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"aicp_hip error {code}: {msg}")
        self.code = code


class ConvergenceError(AicpError):
    """Maps PM::ConvergenceError (uncaught in the reference, app.cpp:210)."""


class TransformationError(AicpError):
    """Maps PM::TransformationError: RigidTransformation::checkParameters rejected a transform
    applied to the reading (|1 - det R| > 0.001)."""


def default_options(**kw) -> Options:
    """aicp_hip_default_options (the product path) with keyword overrides."""
    o = Options()
    lib.aicp_hip_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(f"aicp_hip_options has no field {k}")
        setattr(o, k, v)
    return o


def test_force_scan_stall(on: bool) -> int:
    """aicp_hip_test_force_scan_stall (test hook, the calling thread's device)."""
    return lib.aicp_hip_test_force_scan_stall(1 if on else 0)


def default_config(point_to_point=False, **kw) -> IcpConfig:
    """The default chain's parameters, with fields replaced by name. point_to_point=True asks for
    PointToPointErrorMinimizer without SurfaceNormal on the reference (knn_normals = 0,
    include/aicp_hip.h); every other element of the chain stays."""
    c = IcpConfig()
    lib.aicp_hip_default_config(C.byref(c))
    if point_to_point:
        c.knn_normals = 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def parse_pm_yaml(path: str):
    c = IcpConfig()
    rc = lib.aicp_hip_parse_pm_yaml(path.encode(), C.byref(c))
    return rc, c


def parse_pm_chain(path: str):
    """aicp_hip_parse_pm_chain: (rc, IcpConfig, Chain). The chain's seed is 0."""
    c, ch = IcpConfig(), Chain()
    rc = lib.aicp_hip_parse_pm_chain(path.encode(), C.byref(c), C.byref(ch))
    return rc, c, ch


def chain_uniform(seed: int, slot: int, i: int) -> float:
    """aicp_hip_chain_uniform: the sampled chains' draw, k * 2^-24 in [0, 1)."""
    return float(lib.aicp_hip_chain_uniform(int(seed), int(slot), int(i)))


def autotune_ratio(overlap_percent: float) -> float:
    return float(lib.aicp_hip_autotune_ratio(overlap_percent))


def replace_ratio_config_file(in_path: str, out_path: str, ratio: float) -> int:
    return lib.aicp_hip_replace_ratio_config_file(in_path.encode(), out_path.encode(), ratio)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def as_points(p) -> np.ndarray:
    """float32 array of shape (N, W), C-contiguous, xyz in the first 3 floats of each row:
    W = 3 packed, 4 = pcl::PointXYZ (16 B), 8 = PointXYZRGB (32 B), 12 = PointXYZRGBNormal (48 B)
    (the point types of the registerClouds overloads, abstract_registrator.hpp:10-12; the
    XYZRGBNormal overload is a no-op in the reference, see registration.HipRegistration). The
    row stride is passed through the C-ABI, so no copy is made for these layouts."""
    a = np.ascontiguousarray(p, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] not in (3, 4, 8, 12):
        raise ValueError("points must be (N, 3|4|8|12) float32 rows (PointXYZ / XYZRGB / XYZRGBNormal)")
    return a


def key_bound(points, origin, resolution, rigid=0):
    """aicp_hip_test_key_bound (host only): the stream's bound of a cloud's key-list words, and the
    cap of one point's share. Returns (bound, point_cap)."""
    a = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(origin, np.float64).reshape(3)
    bound, cap = C.c_uint64(), C.c_uint64()
    rc = lib.aicp_hip_test_key_bound(_fptr(a), a.shape[0], o.ctypes.data_as(C.POINTER(C.c_double)),
                                     float(resolution), int(rigid), C.byref(bound), C.byref(cap))
    if rc:
        raise ValueError(f"aicp_hip_test_key_bound: {rc}")
    return int(bound.value), int(cap.value)


def make_pair(ref, read, ref_origin=(0, 0, 0), read_origin=(0, 0, 0), init_T=None):
    """Returns (Pair, keepalive). init_T: 4x4 row-major numpy -> column-major float[16]."""
    ref = as_points(ref)
    read = as_points(read)
    keep = [ref, read]
    p = Pair()
    p.ref = _fptr(ref)
    p.n_ref = ref.shape[0]
    p.ref_stride = ref.shape[1] * 4
    p.read = _fptr(read)
    p.n_read = read.shape[0]
    p.read_stride = read.shape[1] * 4
    if init_T is not None:
        t = np.ascontiguousarray(np.asarray(init_T, np.float32).reshape(4, 4).T.reshape(16))
        keep.append(t)
        p.init_T = _fptr(t)
    for k in range(3):
        p.ref_origin[k] = float(ref_origin[k])
        p.read_origin[k] = float(read_origin[k])
    return p, keep


def default_sequence_params(**kw) -> SequenceParams:
    """App's stream settings (aicp_hip_default_sequence_params): reference every 5 accepted
    readings, max_correction_magnitude 1.0, octomap 0.2 m, per-reading overlap auto-tune."""
    p = SequenceParams()
    lib.aicp_hip_default_sequence_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_localization_params(**kw) -> LocalizationParams:
    """App's localization settings (aicp_hip_default_localization_params): a merge every 5 accepted
    readings, a re-filter every 30, max_correction_magnitude 1.0, crop -15..15, merging on.
    Keyword overrides; merge=/debug= set or clear AICP_LOC_MERGE / AICP_SEQ_DEBUG in flags."""
    p = LocalizationParams()
    lib.aicp_hip_default_localization_params(C.byref(p))
    for k, v in kw.items():
        if k in ("merge", "debug"):
            bit = AICP_LOC_MERGE if k == "merge" else AICP_SEQ_DEBUG
            p.flags = (p.flags | bit) if v else (p.flags & ~bit)
        elif not hasattr(p, k):
            raise AttributeError(f"aicp_localization_params has no field {k}")
        else:
            setattr(p, k, v)
    return p


def localization_window(n_clouds: int, params: LocalizationParams, remaining: int) -> int:
    """aicp_hip_localization_window (host only): the length of the next window of the stream."""
    return int(lib.aicp_hip_localization_window(int(n_clouds), C.byref(params), int(remaining)))


def default_built_map_params(**kw) -> BuiltMapParams:
    """App's settings for localization against the map it built (aicp_hip_default_built_map_params):
    a reference every 5 accepted readings, max_correction_magnitude 1.0, crop -15..15, octomap
    0.2 m, per-reading overlap auto-tune. Keyword overrides; overlap=/debug=/time_nn= set or clear
    AICP_RUN_OVERLAP / AICP_SEQ_DEBUG / AICP_RUN_TIME_NN in flags."""
    p = BuiltMapParams()
    lib.aicp_hip_default_built_map_params(C.byref(p))
    bits = {"overlap": AICP_RUN_OVERLAP, "debug": AICP_SEQ_DEBUG, "time_nn": AICP_RUN_TIME_NN}
    for k, v in kw.items():
        if k in bits:
            p.flags = (p.flags | bits[k]) if v else (p.flags & ~bits[k])
        elif not hasattr(p, k) or k == "pad":
            raise AttributeError(f"aicp_built_map_params has no field {k}")
        else:
            setattr(p, k, v)
    return p


def built_map_window(acc: int, params: BuiltMapParams, remaining: int) -> int:
    """aicp_hip_built_map_window (host only): the length of the next window of the stream."""
    return int(lib.aicp_hip_built_map_window(int(acc), C.byref(params), int(remaining)))


def make_cloud(pts, origin=(0, 0, 0)):
    """Returns (Cloud, keepalive) for (N, 3|4|8|12) float32 rows."""
    a = as_points(pts)
    c = Cloud()
    c.pts = _fptr(a)
    c.n = a.shape[0]
    c.stride = a.shape[1] * 4
    for k in range(3):
        c.origin[k] = float(origin[k])
    return c, a


def default_prefilter(**kw) -> PrefilterParams:
    """filteringUtils.cpp:12,22,27-34 (aicp_hip_default_prefilter); keyword overrides."""
    p = PrefilterParams()
    lib.aicp_hip_default_prefilter(C.byref(p))
    for k, v in kw.items():
        if k == "viewpoint":
            for i in range(3):
                p.viewpoint[i] = float(v[i])
        else:
            setattr(p, k, v)
    return p


def default_risk_params(**kw) -> RiskParams:
    """aicp_hip_default_risk_params: range 100 m, view 360 deg, 20 deg between mean normals, box
    scale (1, 1, 3) (filteringUtils.cpp:258, 520-528) and the pre-filter defaults; keyword
    overrides (box_scale: 3 values, prefilter: a PrefilterParams)."""
    p = RiskParams()
    lib.aicp_hip_default_risk_params(C.byref(p))
    for k, v in kw.items():
        if k == "box_scale":
            for i in range(3):
                p.box_scale[i] = float(v[i])
        elif not hasattr(p, k):
            raise AttributeError(f"aicp_risk_params has no field {k}")
        else:
            setattr(p, k, v)
    return p


def default_monitor_params(**kw) -> MonitorParams:
    """aicp_hip_default_monitor_params: quantile 0.60 (icpMonitor.cpp:31), max_accepted_dist 0.20
    (:128), no flags; keyword overrides."""
    p = MonitorParams()
    lib.aicp_hip_default_monitor_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(f"aicp_monitor_params has no field {k}")
        setattr(p, k, v)
    return p


MONITOR_COUNTERS = ("readings", "trees", "reference_reuses", "chain_trees")


def monitor_argument(monitor):
    """The sessions' monitor= argument as aicp_monitor_params, or None for off: None / False (off),
    True (the defaults), a MonitorParams, or a dict of quantile, max_accepted_dist and paired (bool:
    AICP_MON_PAIRED, the paired mean distance through the session's chain)."""
    if monitor is None or monitor is False:
        return None
    if monitor is True:
        return default_monitor_params()
    if isinstance(monitor, MonitorParams):
        return MonitorParams.from_buffer_copy(monitor)
    if not isinstance(monitor, dict):
        raise TypeError(f"monitor: None, True, MonitorParams or dict, got {type(monitor).__name__}")
    unknown = set(monitor) - {"quantile", "max_accepted_dist", "paired"}
    if unknown:
        raise ValueError(f"monitor: dict(quantile=, max_accepted_dist=, paired=), got {sorted(unknown)}")
    kw = {k: monitor[k] for k in ("quantile", "max_accepted_dist") if k in monitor}
    p = default_monitor_params(**kw)
    if monitor.get("paired"):
        p.flags |= AICP_MON_PAIRED
    return p


class SessionMonitor:
    """set_monitor / last_monitor / monitor_counters of a live session (AppSession: kind "session",
    MapSession: "mapsession"); the class has ctx and h."""
    _monitor_kind = "session"

    def _mon(self, name):
        return getattr(lib, f"aicp_hip_{self._monitor_kind}_{name}")

    def set_monitor(self, monitor=True) -> None:
        """Switch the per-reading quality monitor on (True, a MonitorParams or a dict: see
        monitor_argument) or off (None / False), any time after the session was made."""
        p = monitor_argument(monitor)
        self.ctx.check(self._mon("set_monitor")(self.ctx.h, self.h, None if p is None else C.byref(p)))

    def last_monitor(self) -> dict:
        """The last process call's result as Context.monitor's dict ("bytes": the 56 bytes) with
        "valid": True after a call that registered its reading with the monitor on; otherwise False
        and all zero bytes."""
        res, valid = MonitorResult(), C.c_int32(0)
        self.ctx.check(self._mon("last_monitor")(self.h, C.byref(res), C.byref(valid)))
        d = res.as_dict()
        d["valid"] = bool(valid.value)
        return d

    def monitor_counters(self) -> dict:
        """readings (valid results), trees (bucket-8 trees built), reference_reuses (readings that
        reused the session's reference tree), chain_trees (trees at the chain matcher's bucket size)."""
        c = (C.c_uint64 * 4)()
        self.ctx.check(self._mon("monitor_counters")(self.h, c))
        return dict(zip(MONITOR_COUNTERS, (int(x) for x in c)))


def _pose16(pose):
    """4x4 row-major pose -> column-major double[16] (Eigen::Isometry3d::data())."""
    return np.ascontiguousarray(np.asarray(pose, np.float64).reshape(4, 4).T.reshape(16))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class SvmModel:
    """One aicp_hip_svm: the classifier's OpenCV model XML, parsed on the host (no device needed).
    Raises AicpError with AICP_ERR_UNSUPPORTED / AICP_ERR_INVALID as aicp_hip_svm_load returns them."""

    def __init__(self, path: str):
        self.h = None
        h = C.c_void_p()
        rc = lib.aicp_hip_svm_load(os.fsencode(path), C.byref(h))
        if rc != AICP_OK:
            raise AicpError(rc, f"aicp_hip_svm_load({path}) failed")
        self.h = h

    def info(self) -> dict:
        """aicp_hip_svm_info: the scalar fields, support_vectors (sv_total, 2) float32, alpha
        float64[sv_count], index int32[sv_count]."""
        i = SvmInfo()
        rc = lib.aicp_hip_svm_info(self.h, C.byref(i), None, None, None)
        if rc != AICP_OK:
            raise AicpError(rc, "aicp_hip_svm_info failed")
        sv = np.zeros((i.sv_total, 2), np.float32)
        alpha = np.zeros(i.sv_count, np.float64)
        index = np.zeros(i.sv_count, np.int32)
        lib.aicp_hip_svm_info(self.h, C.byref(i), _fptr(sv), _dptr(alpha), index.ctypes.data_as(C.POINTER(C.c_int32)))
        d = {k: getattr(i, k) for k, _ in SvmInfo._fields_}
        d.update(support_vectors=sv, alpha=alpha, index=index)
        return d

    def close(self):
        if getattr(self, "h", None):
            lib.aicp_hip_svm_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


# aicp_hip_options overrides every new Context starts with (bench.py --opt k=v); empty: the
# library's defaults
CONTEXT_OPTIONS: dict = {}


class Context:
    """One aicp_hip_ctx: a HIP stream + device arena on one GPU."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        rc = lib.aicp_hip_create(int(device), C.byref(h))
        if rc != AICP_OK:
            raise AicpError(rc, f"aicp_hip_create(device={device}) failed (no HIP device?)")
        self.h = h
        self.device = device
        if CONTEXT_OPTIONS:
            self.set_options(**CONTEXT_OPTIONS)

    def close(self):
        if getattr(self, "h", None):
            lib.aicp_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def last_error(self) -> str:
        return lib.aicp_hip_last_error(self.h).decode()

    def get_options(self) -> Options:
        o = Options()
        self.check(lib.aicp_hip_get_options(self.h, C.byref(o)))
        return o

    def set_options(self, opt: Options = None, **kw) -> Options:
        """aicp_hip_set_options: `opt` (default: the context's current options) with keyword
        overrides. Returns the options in force before the call."""
        old = self.get_options()
        new = Options.from_buffer_copy(opt if opt is not None else old)
        for k, v in kw.items():
            if not hasattr(new, k):
                raise AttributeError(f"aicp_hip_options has no field {k}")
            setattr(new, k, v)
        self.check(lib.aicp_hip_set_options(self.h, C.byref(new)))
        return old

    def options(self, **kw):
        """with ctx.options(overlap_path=1): ... -- the overrides for the block only."""
        ctx = self

        class _Scope:
            def __enter__(self):
                self.old = ctx.set_options(**kw)
                return ctx

            def __exit__(self, *exc):
                ctx.set_options(self.old)
                return False

        return _Scope()

    def check(self, rc):
        if rc == AICP_ERR_CONVERGENCE:
            raise ConvergenceError(rc, self.last_error())
        if rc == AICP_ERR_TRANSFORMATION:
            raise TransformationError(rc, self.last_error())
        if rc != AICP_OK:
            raise AicpError(rc, self.last_error())

    # -------------------------------------------------------------- batch pipeline ----------
    def align_batch(self, pairs, cfg=None, resolution=0.2, flags=AICP_RUN_ICP, raise_on_error=True):
        """pairs: list of dict(ref, read, ref_origin, read_origin, init_T). Returns (T[n,4,4]
        row-major float32, list of stats dicts, rc)."""
        cfg = cfg or default_config()
        arr = (Pair * len(pairs))()
        keep = []
        for i, pr in enumerate(pairs):
            p, k = make_pair(pr["ref"], pr["read"], pr.get("ref_origin", (0, 0, 0)),
                             pr.get("read_origin", (0, 0, 0)), pr.get("init_T"))
            arr[i] = p
            keep.append(k)
        outT = np.zeros((len(pairs), 16), np.float32)
        st = (IcpStats * len(pairs))()
        rc = lib.aicp_hip_align_batch(self.h, C.byref(cfg), arr, len(pairs), float(resolution),
                                      int(flags), _fptr(outT), st)
        if raise_on_error and rc != AICP_OK:
            self.check(rc)
        T = outT.reshape(-1, 4, 4).transpose(0, 2, 1).copy()
        return T, [s.as_dict() for s in st], rc

    def register(self, ref, read, cfg=None):
        """aicp_hip_register (registerClouds: one pair, identity initial T, the chain's ratio):
        returns (T 4x4 row-major, stats dict)."""
        cfg = cfg or default_config()
        p, keep = make_pair(ref, read)
        outT = np.zeros(16, np.float32)
        st = IcpStats()
        self.check(lib.aicp_hip_register(self.h, C.byref(cfg), C.byref(p), _fptr(outT), C.byref(st)))
        return outT.reshape(4, 4).T.copy(), st.as_dict()

    def chain_filter(self, chain, side, pts, indices=True, densities=False, normals=False):
        """aicp_hip_chain_filter (DataPointsFilters::apply of one side's list): a dict with `n`
        (kept points), `counts` (points after each filter of the list) and, as asked, `index` (the
        kept points' input indices), `densities` (at the SurfaceNormal's position, for the cloud
        there) and `normals` (of the kept points)."""
        pts = as_points(pts)
        n = pts.shape[0]
        out_n = C.c_uint64()
        counts = (C.c_uint64 * AICP_CHAIN_MAX_FILTERS)()
        idx = np.zeros(n, np.int32) if indices else None
        dens = np.zeros(n, np.float32) if densities else None
        nrm = np.zeros((n, 3), np.float32) if normals else None
        self.check(lib.aicp_hip_chain_filter(
            self.h, C.byref(chain), int(side), _fptr(pts), n, pts.shape[1] * 4, C.byref(out_n), counts,
            idx.ctypes.data_as(C.POINTER(C.c_int32)) if indices else None, _fptr(dens) if densities else None,
            _fptr(nrm) if normals else None))
        k = int(out_n.value)
        nf = chain.n_filters[side]
        out = {"n": k, "counts": [int(counts[q]) for q in range(nf)]}
        if indices:
            out["index"] = idx[:k].copy()
        if densities:
            # the cloud at the SurfaceNormal: what the filters before it left
            sn = next(q for q in range(nf) if chain.filters[side][q].kind == AICP_FILTER_SURFACE_NORMAL)
            out["densities"] = dens[:(out["counts"][sn - 1] if sn else n)].copy()
        if normals:
            out["normals"] = nrm[:k].copy()
        return out

    def register_chain(self, ref, read, cfg, chain, raise_on_error=True):
        """aicp_hip_register_chain: both clouds through the chain's filters, then the ICP core on
        what they leave. Returns (T 4x4 row-major, stats dict, chain stats dict, rc)."""
        p, keep = make_pair(ref, read)
        outT = np.zeros(16, np.float32)
        st, cs = IcpStats(), ChainStats()
        rc = lib.aicp_hip_register_chain(self.h, C.byref(cfg), C.byref(chain), C.byref(p), _fptr(outT), C.byref(st),
                                         C.byref(cs))
        if raise_on_error:
            self.check(rc)
        return outT.reshape(4, 4).T.copy(), st.as_dict(), cs.as_dict(), rc

    def align_chain_batch(self, pairs, cfg, chain, resolution=0.2, flags=AICP_RUN_ICP, raise_on_error=True):
        """aicp_hip_align_chain_batch: register_chain for every pair of `pairs` (dicts as align_batch
        takes them) in one call; with AICP_RUN_OVERLAP the overlap of the clouds as given sets each
        pair's ratio. Pairs that pass the same `ref` array share it. Returns (T[n,4,4] row-major,
        list of stats dicts, list of chain stats dicts, rc)."""
        arr = (Pair * len(pairs))()
        keep = []
        refs = {}  # the same array object -> one packed copy, so that the pointers are equal too
        for i, pr in enumerate(pairs):
            if id(pr["ref"]) not in refs:
                refs[id(pr["ref"])] = as_points(pr["ref"])
            ref = refs[id(pr["ref"])]
            p, k = make_pair(ref, pr["read"], pr.get("ref_origin", (0, 0, 0)), pr.get("read_origin", (0, 0, 0)),
                             pr.get("init_T"))
            arr[i] = p
            keep.append((k, pr["ref"]))
        outT = np.zeros((len(pairs), 16), np.float32)
        st = (IcpStats * len(pairs))()
        cs = (ChainStats * len(pairs))()
        rc = lib.aicp_hip_align_chain_batch(self.h, C.byref(cfg), C.byref(chain), arr, len(pairs), float(resolution),
                                            int(flags), _fptr(outT), st, cs)
        if raise_on_error:
            self.check(rc)
        T = outT.reshape(-1, 4, 4).transpose(0, 2, 1).copy()
        return T, [s.as_dict() for s in st], [c.as_dict() for c in cs], rc

    def test_chain_batch(self, chain, side, clouds, normals=False, densities=False):
        """aicp_hip_test_chain_batch: one side's list over the clouds at once. Returns one dict per
        cloud, as chain_filter's: n, counts, index and, as asked, normals and densities."""
        clouds = [as_points(c) for c in clouds]
        counts = np.array([len(c) for c in clouds], np.uint32)
        pts = np.ascontiguousarray(np.concatenate([c[:, :3] for c in clouds]), np.float32)
        total, nc = len(pts), len(clouds)
        oc = np.zeros(4 * nc, np.uint64)
        on = np.zeros(nc, np.uint64)
        idx = np.zeros(total, np.int32)
        nrm = np.zeros((total, 3), np.float32) if normals else None
        dens = np.zeros(total, np.float32) if densities else None
        self.check(lib.aicp_hip_test_chain_batch(
            self.h, C.byref(chain), int(side), nc, counts.ctypes.data_as(C.POINTER(C.c_uint32)), _fptr(pts),
            oc.ctypes.data_as(C.POINTER(C.c_uint64)), on.ctypes.data_as(C.POINTER(C.c_uint64)),
            idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(nrm) if normals else None,
            _fptr(dens) if densities else None))
        nf = chain.n_filters[side]
        sn = next((q for q in range(nf) if chain.filters[side][q].kind == AICP_FILTER_SURFACE_NORMAL), None)
        out, k, kd = [], 0, 0
        for c in range(nc):
            n = int(on[c])
            d = {"n": n, "counts": [int(oc[4 * c + q]) for q in range(nf)], "index": idx[k:k + n].copy()}
            if normals:
                d["normals"] = nrm[k:k + n].copy()
            if densities:
                m = d["counts"][sn - 1] if sn else int(counts[c])
                d["densities"] = dens[kd:kd + m].copy()
                kd += m
            k += n
            out.append(d)
        return out

    def overlap(self, ref, read, ref_origin=(0, 0, 0), read_origin=(0, 0, 0), resolution=0.2):
        """aicp_hip_overlap (computeOverlap + getOverlap for one pair): the overlap in percent."""
        p, keep = make_pair(ref, read, ref_origin, read_origin)
        out = np.zeros(1, np.float32)
        self.check(lib.aicp_hip_overlap(self.h, C.byref(p), float(resolution), _fptr(out)))
        return float(out[0])

    def reference_cache_stats(self):
        """aicp_hip_reference_cache_stats: tree hits / builds, overlap-map hits / builds of the
        one-shot calls' resident reference."""
        a = (C.c_uint64 * 4)()
        self.check(lib.aicp_hip_reference_cache_stats(self.h, a))
        return dict(tree_hits=a[0], tree_builds=a[1], ovl_hits=a[2], ovl_builds=a[3])

    def upload(self, pairs):
        return ResidentBatch(self, pairs)

    def sequence_run(self, first, first_origin, readings, origins, cfg=None, params=None, raise_on_error=True,
                     prefilter=None):
        """App's frame-to-reference stream (aicp_hip_sequence_run): the first cloud is the
        reference, readings[i] (prior-pose origin origins[i]) are registered in order with the
        windowed reference update and the max-correction drop. Returns (T[n, 4, 4] row-major
        corrections, list of result dicts, n_done, rc). prefilter (PrefilterParams, or True for
        the defaults): the clouds are RAW and run in App's order (aicp_hip_sequence_run_raw)."""
        cfg = cfg or default_config()
        prm = params or default_sequence_params()
        if prefilter is True:
            prefilter = default_prefilter()
        n = len(readings)
        fc, keep0 = make_cloud(first, first_origin)
        arr = (Cloud * max(n, 1))()
        keep = [keep0]
        for i, r in enumerate(readings):
            c, k = make_cloud(r, origins[i])
            arr[i] = c
            keep.append(k)
        outT = np.zeros((max(n, 1), 16), np.float32)
        res = (SequenceResult * max(n, 1))()
        done = C.c_size_t(0)
        if prefilter is not None:
            rc = lib.aicp_hip_sequence_run_raw(self.h, C.byref(cfg), C.byref(prm), C.byref(prefilter), C.byref(fc), arr,
                                               n, _fptr(outT), res, C.byref(done))
        else:
            rc = lib.aicp_hip_sequence_run(self.h, C.byref(cfg), C.byref(prm), C.byref(fc), arr, n, _fptr(outT), res,
                                           C.byref(done))
        if raise_on_error and rc != AICP_OK:
            self.check(rc)
        T = outT[:n].reshape(-1, 4, 4).transpose(0, 2, 1).copy()
        return T, [res[i].as_dict() for i in range(done.value)], done.value, rc

    def last_sequence_timing(self):
        t = SequenceTiming()
        self.check(lib.aicp_hip_last_sequence_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in SequenceTiming._fields_}

    def last_localization_timing(self):
        """aicp_hip_last_localization_timing: windows, merges, refilters, wall_ms, device_ms of the
        last PriorMap.sequence_run."""
        t = LocalizationTiming()
        self.check(lib.aicp_hip_last_localization_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in LocalizationTiming._fields_ if k != "pad"}

    def last_built_map_timing(self):
        """aicp_hip_last_built_map_timing: windows, appends, wall_ms, device_ms of the last
        BuiltMap.sequence_run."""
        t = BuiltMapTiming()
        self.check(lib.aicp_hip_last_built_map_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in BuiltMapTiming._fields_}

    def last_nn_timing(self):
        n = C.c_int()
        ms = C.c_double()
        by = C.c_double()
        q = C.c_uint64()
        lib.aicp_hip_last_nn_timing(self.h, C.byref(n), C.byref(ms), C.byref(by), C.byref(q))
        return dict(launches=n.value, total_ms=ms.value, bytes=by.value, queries=q.value)

    def last_phase_ms(self):
        a = (C.c_double * 5)()
        lib.aicp_hip_last_phase_ms(self.h, a)
        return dict(overlap=a[0], normals=a[1], matcher_tree=a[2], icp_loop=a[3], total=a[4])

    # -------------------------------------------------------------- kernel-level -----------
    def knn(self, pts, queries, k=1, eps=0.0, max_dist=float("inf")):
        pts = as_points(pts)
        q = as_points(queries)
        ids = np.zeros((q.shape[0], k), np.int32)
        d2 = np.zeros((q.shape[0], k), np.float32)
        touched = np.zeros(2, np.uint64)
        rc = lib.aicp_hip_knn(self.h, _fptr(pts), pts.shape[0], pts.shape[1] * 4, _fptr(q), q.shape[0],
                              q.shape[1] * 4, int(k), float(eps), float(max_dist),
                              ids.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2),
                              touched.ctypes.data_as(C.POINTER(C.c_uint64)))
        self.check(rc)
        return ids, d2, int(touched[0]), int(touched[1])

    def normals(self, pts, knn=20):
        pts = as_points(pts)
        out = np.zeros((pts.shape[0], 3), np.float32)
        deg = C.c_int32()
        rc = lib.aicp_hip_normals(self.h, _fptr(pts), pts.shape[0], pts.shape[1] * 4, int(knn), _fptr(out),
                                  C.byref(deg))
        self.check(rc)
        return out, deg.value

    def dists_quantile(self, d2, quantile):
        d2 = np.ascontiguousarray(d2, np.float32).ravel()
        out = C.c_float()
        rc = lib.aicp_hip_dists_quantile(self.h, _fptr(d2), d2.size, float(quantile), C.byref(out))
        self.check(rc)
        return out.value

    def test_select(self, d2_steps, counts, ratios, variants, active=None):
        """aicp_hip_test_select: one select per step (variants[s]: 0 separate launches, 1 two
        launches with tails, 2 fused, 3 / 4 fused with 2048 / 8192 candidates in LDS, 5 one workgroup
        per pair) on d2_steps[s], the pairs' distances one after another (counts[p] each), on the
        same pair states. Returns limit, status, n_finite, b1 and miss as (n_steps, n_pairs) arrays
        and dirty, the non-zero words the last step left in the select's work space."""
        counts = np.ascontiguousarray(counts, np.uint32).ravel()
        ratios = np.ascontiguousarray(ratios, np.float32).ravel()
        variants = np.ascontiguousarray(variants, np.int32).ravel()
        P, S, total = counts.size, variants.size, int(counts.sum(dtype=np.uint64))
        if ratios.size != P or len(d2_steps) != S:
            raise ValueError("one ratio per pair and one distance array per step")
        d2 = np.empty((S, total), np.float32)
        for s, d in enumerate(d2_steps):
            d = np.ascontiguousarray(d, np.float32).ravel()
            if d.size != total:
                raise ValueError(f"step {s}: {d.size} distances for {total} readings")
            d2[s] = d
        act = None
        if active is not None:
            act = np.ascontiguousarray(active, np.uint8).ravel()
            if act.size != P:
                raise ValueError("one active flag per pair")
        out = dict(limit=np.zeros((S, P), np.float32), status=np.zeros((S, P), np.int32),
                   n_finite=np.zeros((S, P), np.int32), b1=np.zeros((S, P), np.uint32),
                   miss=np.zeros((S, P), np.uint32))
        dirty = C.c_uint64()
        ip, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        rc = lib.aicp_hip_test_select(
            self.h, P, counts.ctypes.data_as(u32p), _fptr(ratios),
            act.ctypes.data_as(C.POINTER(C.c_uint8)) if act is not None else None, S, variants.ctypes.data_as(ip),
            _fptr(d2), _fptr(out["limit"]), out["status"].ctypes.data_as(ip), out["n_finite"].ctypes.data_as(ip),
            out["b1"].ctypes.data_as(u32p), out["miss"].ctypes.data_as(u32p), C.byref(dirty))
        self.check(rc)
        out["dirty"] = int(dirty.value)
        return out

    def test_step(self, n_read, n_ref, ref_off, read_c, ref_pts, ref_nrm, limit, match, d2, touched, init_T=None,
                  active=None, max_iter=20, smooth=4, min_rot=1e-3, min_trans=1e-2):
        """aicp_hip_test_step: the production reduce + update launch, once per step, on given matches.
        n_read, n_ref, ref_off: per pair; read_c (total, 3); ref_pts, ref_nrm (total_ref, 3); limit
        (n_steps, n_pairs); match, d2, touched (n_steps, total). Returns per step and pair: slab (a list
        over steps of (rows, 30) arrays), T (S, P, 16), kept, iters, status, active, converged,
        hist_count, inlier_ratio, touched_pts, touched_nodes, dq, dt as (S, P) arrays, and dirty."""
        if ref_nrm is None:
            raise ValueError("ref_nrm")
        return Context._test_step(self, n_read, n_ref, ref_off, read_c, ref_pts, ref_nrm, limit, match, d2, touched,
                                  init_T, active, max_iter, smooth, min_rot, min_trans)

    def test_step_p2p(self, n_read, n_ref, ref_off, read_c, ref_pts, limit, match, d2, touched, init_T=None,
                      active=None, max_iter=20, smooth=4, min_rot=1e-3, min_trans=1e-2, **unused):
        """aicp_hip_test_step_p2p: test_step with the point-to-point kernels (no normals; a case's other
        keys are ignored). Slab columns: 0..8 sum q_a p_b, 9..11 sum p, 12..14 sum q, 15..26 zero, 27
        kept, 28 / 29 touched points / nodes."""
        return Context._test_step(self, n_read, n_ref, ref_off, read_c, ref_pts, None, limit, match, d2, touched,
                                  init_T, active, max_iter, smooth, min_rot, min_trans)

    def _test_step(self, n_read, n_ref, ref_off, read_c, ref_pts, ref_nrm, limit, match, d2, touched, init_T,
                   active, max_iter, smooth, min_rot, min_trans):
        p2p = ref_nrm is None
        n_read = np.ascontiguousarray(n_read, np.uint32).ravel()
        n_ref = np.ascontiguousarray(n_ref, np.uint32).ravel()
        ref_off = np.ascontiguousarray(ref_off, np.uint32).ravel()
        read_c = np.ascontiguousarray(read_c, np.float32).reshape(-1, 3)
        ref_pts = np.ascontiguousarray(ref_pts, np.float32).reshape(-1, 3)
        ref_nrm = ref_pts if p2p else np.ascontiguousarray(ref_nrm, np.float32).reshape(-1, 3)
        P, total, total_ref = n_read.size, int(n_read.sum(dtype=np.uint64)), ref_pts.shape[0]
        limit = np.ascontiguousarray(limit, np.float32)
        S = limit.shape[0] if limit.ndim == 2 else 0
        match = np.ascontiguousarray(match, np.int32)
        d2 = np.ascontiguousarray(d2, np.float32)
        touched = np.ascontiguousarray(touched, np.uint32)
        if n_ref.size != P or ref_off.size != P or read_c.shape[0] != total or ref_nrm.shape[0] != total_ref:
            raise ValueError("per-pair arrays of one length; read_c of sum(n_read) rows; one normal per reference point")
        if limit.shape != (S, P) or any(a.shape != (S, total) for a in (match, d2, touched)):
            raise ValueError("limit (n_steps, n_pairs); match, d2, touched (n_steps, sum(n_read))")
        T0 = act = None
        if init_T is not None:
            T0 = np.ascontiguousarray(init_T, np.float32).reshape(P, 16)
        if active is not None:
            act = np.ascontiguousarray(active, np.uint8).ravel()
            if act.size != P:
                raise ValueError("one active flag per pair")
        rows = int(((n_read.astype(np.int64) + 1023) // 1024).sum())
        slab = np.zeros((S, rows, 30), np.float64)
        T = np.zeros((S, P, 16), np.float32)
        state = np.zeros((S, P, 6), np.int32)
        inl = np.zeros((S, P), np.float32)
        tch = np.zeros((S, P, 2), np.uint64)
        dqdt = np.zeros((S, P, 2), np.float64)
        dirty = C.c_uint64()
        ip, u32p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        fn = lib.aicp_hip_test_step_p2p if p2p else lib.aicp_hip_test_step
        rc = fn(
            self.h, P, n_read.ctypes.data_as(u32p), n_ref.ctypes.data_as(u32p), ref_off.ctypes.data_as(u32p), total_ref,
            _fptr(read_c), _fptr(ref_pts), *(() if p2p else (_fptr(ref_nrm),)), _fptr(T0) if T0 is not None else None,
            act.ctypes.data_as(u8p) if act is not None else None, int(max_iter), int(smooth), float(min_rot),
            float(min_trans), S, _fptr(limit), match.ctypes.data_as(ip), _fptr(d2), touched.ctypes.data_as(u32p),
            slab.ctypes.data_as(dp), _fptr(T), state.ctypes.data_as(ip), _fptr(inl), tch.ctypes.data_as(u64p),
            dqdt.ctypes.data_as(dp), C.byref(dirty))
        self.check(rc)
        out = dict(slab=slab, T=T, inlier_ratio=inl, touched_pts=tch[..., 0].copy(), touched_nodes=tch[..., 1].copy(),
                   dq=dqdt[..., 0].copy(), dt=dqdt[..., 1].copy(), dirty=int(dirty.value))
        for i, k in enumerate(("kept", "iters", "status", "active", "converged", "hist_count")):
            out[k] = state[..., i].copy()
        return out

    def solve6(self, A, b):
        A = np.ascontiguousarray(A, np.float64).reshape(36)
        b = np.ascontiguousarray(b, np.float64).reshape(6)
        x = np.zeros(6, np.float64)
        path = C.c_int32()
        dp = C.POINTER(C.c_double)
        rc = lib.aicp_hip_solve6(self.h, A.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                 C.byref(path))
        self.check(rc)
        return x, path.value

    def transform(self, T, pts):
        pts = as_points(pts)
        t = np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T.reshape(16))
        out = np.zeros((pts.shape[0], 3), np.float32)
        rc = lib.aicp_hip_transform(self.h, _fptr(t), _fptr(pts), pts.shape[0], pts.shape[1] * 4, _fptr(out))
        self.check(rc)
        return out

    def test_ingest(self, rows, T=None, download=True):
        """aicp_hip_test_ingest: the raw streams' upload and k_stream_ingest alone. rows: (N, 3|4|8|12)
        float32; T: 4x4 row-major (None: no move). Returns (N, 4) float32 rows (x, y, z, 1), or
        None with download=False (the timing tool's)."""
        a = as_points(rows)
        t = None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T.reshape(16))
        out = np.zeros((max(a.shape[0], 1), 4), np.float32) if download else None
        rc = lib.aicp_hip_test_ingest(self.h, _fptr(a), a.shape[0], a.shape[1] * 4, None if t is None else _fptr(t),
                                      _fptr(out) if download else None)
        self.check(rc)
        return out[:a.shape[0]] if download else None

    def test_tree(self, clouds, center=0, bucket=8):
        """aicp_hip_test_tree: the matcher's batched kd-tree build on `clouds` (a list of (n, 3)
        float32 arrays, one batch) and what it wrote. Returns dict(rc, error (the last error text for
        rc != 0), ctl=dict(nseg (50,), n_small, n_mid, n_big, error), trees=[...]); a tree is
        dict(node_off, n_nodes, tree_depth, mean (3,) float32, bpts (n, 3) float32 and ids (n,)
        int32 in bucket order, and per node cd (3: leaf), cut (float32, 0 at a leaf), cut_bits,
        right_or_count (right child, or the leaf's point count), bucket_start (-1 at an inner node),
        parent (-1 at the root), depth). rc is AICP_ERR_UNSUPPORTED / AICP_ERR_HIP for a build
        that reports a depth error / another error bit; the outputs are filled all the same. Any
        other failure raises."""
        clouds = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in clouds]
        counts = np.array([c.shape[0] for c in clouds], np.uint32)
        P, total = counts.size, int(counts.sum(dtype=np.uint64))
        pts = np.ascontiguousarray(np.concatenate(clouds, axis=0)) if P else np.zeros((0, 3), np.float32)
        node_off, n_nodes = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
        depth, mean = np.zeros(P, np.int32), np.zeros((P, 3), np.float32)
        nodes = np.zeros((2 * total + 2, 4), np.uint32)
        bpts = np.zeros((total, 4), np.float32)
        ctl = np.zeros(54, np.uint32)  # AICP_TEST_TREE_CTL_WORDS
        u32p, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        rc = lib.aicp_hip_test_tree(self.h, P, counts.ctypes.data_as(u32p), _fptr(pts), int(center), int(bucket),
                                    node_off.ctypes.data_as(u32p), n_nodes.ctypes.data_as(u32p),
                                    depth.ctypes.data_as(ip), _fptr(mean), nodes.ctypes.data_as(u32p), _fptr(bpts),
                                    ctl.ctypes.data_as(u32p))
        err = int(ctl[53])
        if rc != AICP_OK and not (rc in (AICP_ERR_HIP, AICP_ERR_UNSUPPORTED) and err):
            self.check(rc)
        out = dict(rc=rc, error=self.last_error() if rc else "",
                   ctl=dict(nseg=ctl[:50].copy(), n_small=int(ctl[50]), n_mid=int(ctl[51]), n_big=int(ctl[52]),
                            error=err),
                   trees=[])
        off = 0
        for p in range(P):
            n = int(counts[p])
            no = min(int(node_off[p]), nodes.shape[0])
            rec = nodes[no:min(no + int(n_nodes[p]), nodes.shape[0])]
            leaf = (rec[:, 1] & 3) == 3
            b = bpts[off:off + n]
            out["trees"].append(dict(
                node_off=int(node_off[p]), n_nodes=int(n_nodes[p]), tree_depth=int(depth[p]), mean=mean[p].copy(),
                bpts=b[:, :3].copy(), ids=b[:, 3].copy().view(np.int32),
                cd=(rec[:, 1] & 3).astype(np.int32),
                cut=np.where(leaf, np.uint32(0), rec[:, 0]).astype(np.uint32).view(np.float32),
                cut_bits=rec[:, 0].copy(),
                right_or_count=np.where(leaf, rec[:, 0], rec[:, 1] >> 2).astype(np.int32),
                bucket_start=np.where(leaf, (rec[:, 1] >> 2).astype(np.int64), -1).astype(np.int32),
                parent=rec[:, 2].copy().view(np.int32), depth=rec[:, 3].astype(np.int32)))
            off += n
        return out

    def test_nn(self, refs, bucket, pair_ref, reads, T, active=None, eps=0.0, max_dist=float("inf")):
        """aicp_hip_test_nn: the production NN launch, once per step. refs: a list of (n, 3) float32
        reference clouds (built as one batch, no centring); pair_ref: the reference of each pair;
        reads: one (m, 3) float32 array of readings per pair; T: (n_steps, n_pairs, 16) column-major
        float32; active: (n_steps, n_pairs) flags or None. Returns dict(match, d2, touched: (n_steps,
        total) arrays, match a bucket position within the pair's reference; ids: per reference the
        input id of every bucket position; engine: 0 treelets, 1 node records; dirty; read_off: each
        pair's first column)."""
        refs = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in refs]
        reads = [np.ascontiguousarray(r, np.float32).reshape(-1, 3) for r in reads]
        counts = np.array([c.shape[0] for c in refs], np.uint32)
        n_read = np.array([r.shape[0] for r in reads], np.uint32)
        pair_ref = np.ascontiguousarray(pair_ref, np.uint32).ravel()
        R, P = counts.size, n_read.size
        total_ref, total = int(counts.sum(dtype=np.uint64)), int(n_read.sum(dtype=np.uint64))
        T = np.ascontiguousarray(T, np.float32)
        S = T.shape[0] if T.ndim == 3 else 0
        if pair_ref.size != P or T.shape != (S, P, 16):
            raise ValueError("one reference and one array of readings per pair; T (n_steps, n_pairs, 16)")
        act = None
        if active is not None:
            act = np.ascontiguousarray(active, np.uint8)
            if act.shape != (S, P):
                raise ValueError("active (n_steps, n_pairs)")
        rp = np.ascontiguousarray(np.concatenate(refs, axis=0)) if R else np.zeros((0, 3), np.float32)
        rd = np.ascontiguousarray(np.concatenate(reads, axis=0)) if P else np.zeros((0, 3), np.float32)
        match, d2 = np.zeros((S, total), np.int32), np.zeros((S, total), np.float32)
        touched, ids = np.zeros((S, total), np.uint32), np.zeros(total_ref, np.int32)
        engine, dirty = C.c_int32(-1), C.c_uint64()
        ip, u32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        rc = lib.aicp_hip_test_nn(
            self.h, R, counts.ctypes.data_as(u32p), _fptr(rp), int(bucket), P, pair_ref.ctypes.data_as(u32p),
            n_read.ctypes.data_as(u32p), _fptr(rd), S, _fptr(T), act.ctypes.data_as(u8p) if act is not None else None,
            float(eps), float(max_dist), match.ctypes.data_as(ip), _fptr(d2), touched.ctypes.data_as(u32p),
            ids.ctypes.data_as(ip), C.byref(engine), C.byref(dirty))
        self.check(rc)
        ro = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        return dict(match=match, d2=d2, touched=touched, ids=[ids[ro[r]:ro[r + 1]] for r in range(R)],
                    engine=engine.value, dirty=int(dirty.value),
                    read_off=np.concatenate([[0], np.cumsum(n_read.astype(np.int64))]))

    def test_overlap(self, refs, pair_ref, reads, ref_origins, read_origins, resolution, path=0, filter=-1,
                     wide=-1, caps=None, rigid=0, arena_cap=64 << 20, words_cap=4 << 20, check=True):
        """aicp_hip_test_overlap: the batch's overlap on given clouds, and what it wrote. refs, reads:
        lists of (n, 3) float32 clouds; pair_ref: each pair's reference; ref_origins, read_origins:
        (n_pairs, 3). Clouds are numbered groups first, then readings. Returns dict(path, filter, wide
        (what ran), n_groups, pair_group, cloud_keys, cloud_err, cloud_bbox (n_clouds, 6), pair_counts
        (n_pairs, 3), pair_percent, pair_ratio, pair_err; dense maps: desc_min, desc_dim (n_clouds, 3),
        desc_off, desc_bytes, arena (uint8, the whole arena), arena_bytes; sorted keys: key_counts,
        key_offsets (per point: the groups' references, then the readings), words (sorted), n_words;
        the stream paths 3 and 4: cloud_bound, list_off, list_cap (two lists per group), dirty).
        caps: explicit capacities per cloud (groups, then readings) for paths 3 and 4. check=False
        returns the return code instead of raising."""
        refs = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in refs]
        reads = [np.ascontiguousarray(r, np.float32).reshape(-1, 3) for r in reads]
        counts = np.array([c.shape[0] for c in refs], np.uint32)
        n_read = np.array([r.shape[0] for r in reads], np.uint32)
        pair_ref = np.ascontiguousarray(pair_ref, np.uint32).ravel()
        R, P = counts.size, n_read.size
        ro = np.ascontiguousarray(ref_origins, np.float64).reshape(-1, 3)
        do = np.ascontiguousarray(read_origins, np.float64).reshape(-1, 3)
        if pair_ref.size != P or ro.shape[0] != P or do.shape[0] != P:
            raise ValueError("one reference, one reading and two origins per pair")
        rp = np.ascontiguousarray(np.concatenate(refs, axis=0)) if R else np.zeros((0, 3), np.float32)
        rd = np.ascontiguousarray(np.concatenate(reads, axis=0)) if P else np.zeros((0, 3), np.float32)
        points_cap = int(n_read.sum(dtype=np.uint64)) + sum(int(counts[r]) for r in pair_ref if r < R)
        nc = 2 * max(P, 1)
        a = dict(pair_group=np.zeros(P, np.int32), cloud_keys=np.zeros(nc, np.uint64), cloud_err=np.zeros(nc, np.int32),
                 cloud_bbox=np.zeros((nc, 6), np.int32), pair_counts=np.zeros((P, 3), np.uint64),
                 pair_percent=np.zeros(P, np.float32), pair_ratio=np.zeros(P, np.float32),
                 pair_err=np.zeros(P, np.int32), desc_min=np.zeros((nc, 3), np.int32),
                 desc_dim=np.zeros((nc, 3), np.int32), desc_off=np.zeros(nc, np.uint64),
                 desc_bytes=np.zeros(nc, np.uint64), arena=np.zeros(max(int(arena_cap), 1), np.uint8),
                 key_counts=np.zeros(max(points_cap, 1), np.uint32), key_offsets=np.zeros(max(points_cap, 1), np.uint64),
                 words=np.zeros(max(int(words_cap), 1), np.uint64), cloud_bound=np.zeros(nc, np.uint64),
                 list_off=np.zeros(nc, np.uint64), list_cap=np.zeros(nc, np.uint64))
        cp = None if caps is None else np.ascontiguousarray(caps, np.uint64).ravel()
        if cp is not None and cp.size > nc:
            raise ValueError("one capacity per cloud")
        o = TestOverlapOut()
        for name, ctype in TestOverlapOut._fields_:
            if name in a:
                setattr(o, name, a[name].ctypes.data_as(ctype))
        o.arena_cap, o.points_cap, o.words_cap = int(arena_cap), points_cap, int(words_cap)
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        rc = lib.aicp_hip_test_overlap(
            self.h, R, counts.ctypes.data_as(u32p), _fptr(rp), P, pair_ref.ctypes.data_as(u32p),
            n_read.ctypes.data_as(u32p), _fptr(rd), ro.ctypes.data_as(dp), do.ctypes.data_as(dp), float(resolution),
            int(path), int(filter), int(wide), 0 if cp is None else 1,
            None if cp is None else cp.ctypes.data_as(C.POINTER(C.c_uint64)), int(rigid), C.byref(o))
        if not check and rc:
            return rc
        self.check(rc)
        if o.arena_bytes > o.arena_cap or o.n_words > o.words_cap:
            raise ValueError(f"arena {o.arena_bytes} B / {o.n_words} words exceed the given capacities")
        n = o.n_groups + P
        out = dict(path=o.path, filter=o.filter, wide=o.wide, n_groups=o.n_groups, arena_bytes=int(o.arena_bytes),
                   n_words=int(o.n_words), n_points=int(o.n_points), dirty=int(o.dirty))
        for k in ("pair_group", "pair_counts", "pair_percent", "pair_ratio", "pair_err"):
            out[k] = a[k]
        for k in ("cloud_keys", "cloud_err", "cloud_bbox", "desc_min", "desc_dim", "desc_off", "desc_bytes",
                  "cloud_bound"):
            out[k] = a[k][:n]
        out["list_off"], out["list_cap"] = a["list_off"][:2 * o.n_groups], a["list_cap"][:2 * o.n_groups]
        out["arena"] = a["arena"][:int(o.arena_bytes)]
        out["key_counts"], out["key_offsets"] = a["key_counts"][:int(o.n_points)], a["key_offsets"][:int(o.n_points)]
        out["words"] = a["words"][:int(o.n_words)]
        return out

    def test_normals(self, refs, knn=20, matcher_bucket=8):
        """aicp_hip_test_normals: the SurfaceNormal chain of a batch's references. refs: a list of
        (n, 3) float32 clouds (one batch). Returns dict(ids, ids2: per reference (n, knn) raw bucket
        positions in k-best order, -1 for none; raw_id, matcher_id: per reference the input id of
        every raw / matcher bucket position; nrm, bnrm: per reference (n, 4) float32 in raw / matcher
        bucket order; degenerate: (n_refs,); touched: (bucket points, inner nodes) of the second kNN
        launch; engine: 1 octet, 2 per lane; dirty)."""
        refs = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in refs]
        counts = np.array([c.shape[0] for c in refs], np.uint32)
        R, total = counts.size, int(counts.sum(dtype=np.uint64))
        rp = np.ascontiguousarray(np.concatenate(refs, axis=0)) if R else np.zeros((0, 3), np.float32)
        k = max(int(knn), 0)
        ids, ids2 = np.zeros((total, k), np.int32), np.zeros((total, k), np.int32)
        raw_id, matcher_id = np.zeros(total, np.int32), np.zeros(total, np.int32)
        nrm, bnrm = np.zeros((total, 4), np.float32), np.zeros((total, 4), np.float32)
        deg, touched = np.zeros(R, np.int32), np.zeros(2, np.uint64)
        engine, dirty = C.c_int32(-1), C.c_uint64()
        ip, u32p, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        rc = lib.aicp_hip_test_normals(
            self.h, R, counts.ctypes.data_as(u32p), _fptr(rp), int(knn), int(matcher_bucket), ids.ctypes.data_as(ip),
            ids2.ctypes.data_as(ip), raw_id.ctypes.data_as(ip), _fptr(nrm), deg.ctypes.data_as(ip),
            touched.ctypes.data_as(up), _fptr(bnrm), matcher_id.ctypes.data_as(ip), C.byref(engine), C.byref(dirty))
        self.check(rc)
        ro = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        cut = lambda a: [a[ro[r]:ro[r + 1]] for r in range(R)]
        return dict(ids=cut(ids), ids2=cut(ids2), raw_id=cut(raw_id), matcher_id=cut(matcher_id), nrm=cut(nrm),
                    bnrm=cut(bnrm), degenerate=deg, touched=(int(touched[0]), int(touched[1])), engine=engine.value,
                    dirty=int(dirty.value))

    def crop_box(self, pts, mn, mx, origin):
        """getPointsInOrientedBox (filteringUtils.cpp:619-637) on device: returns (kept xyz in
        input order, box angles rx, ry, rz). origin is a 4x4 row-major pose (Matrix4f values)."""
        pts = as_points(pts)
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(4, 4).T.reshape(16))
        out = np.zeros((pts.shape[0], 3), np.float32)
        m = C.c_size_t(0)
        rpy = np.zeros(3, np.float32)
        rc = lib.aicp_hip_crop_box(self.h, _fptr(pts), pts.shape[0], pts.shape[1] * 4, mn, mx, _fptr(o),
                                   _fptr(out), C.byref(m), _fptr(rpy))
        self.check(rc)
        return out[:m.value].copy(), rpy

    def last_prefilter_stats(self):
        st = PrefilterStats()
        self.check(lib.aicp_hip_last_prefilter_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in PrefilterStats._fields_ if k != "pad"}

    def prefilter(self, pts, params=None, details=False):
        """regionGrowingUniformPlaneSegmentationFilter (filteringUtils.cpp:5-45) on device.
        Returns the kept points (clusters concatenated), or with details=True a dict with
        out, sampled (V, 8) {x, y, z, curvature, nx, ny, nz, 0}, labels (V,) and n_clusters."""
        pts = as_points(pts)
        n = pts.shape[0]
        prm = params or default_prefilter()
        out = np.zeros((max(n, 1), 3), np.float32)
        m, ns, nc = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        sampled = np.zeros((max(n, 1), 8), np.float32) if details else None
        labels = np.zeros(max(n, 1), np.int32) if details else None
        rc = lib.aicp_hip_prefilter(self.h, C.byref(prm), _fptr(pts), n, pts.shape[1] * 4, _fptr(out), C.byref(m),
                                    _fptr(sampled) if details else None,
                                    labels.ctypes.data_as(C.POINTER(C.c_int32)) if details else None,
                                    C.byref(ns), C.byref(nc))
        self.check(rc)
        if not details:
            return out[:m.value].copy()
        V = ns.value
        return dict(out=out[:m.value].copy(), sampled=sampled[:V].copy(), labels=labels[:V].copy(),
                    n_clusters=nc.value)


    # -------------------------------------------------------------- alignment risk ---------
    def fov_overlap(self, cloud_a, cloud_b, pose_a, pose_b, range_m=100.0, angular_view=360.0):
        """overlapFilter (filteringUtils.cpp:111-193): returns (fov_overlap, accepted A, accepted B),
        the accepted clouds (M, 3) float32 in the global frame, input order."""
        ca, ka = make_cloud(cloud_a)
        cb, kb = make_cloud(cloud_b)
        pa, pb = _pose16(pose_a), _pose16(pose_b)
        oa = np.zeros((max(ka.shape[0], 1), 3), np.float32)
        ob = np.zeros((max(kb.shape[0], 1), 3), np.float32)
        na, nb = C.c_size_t(0), C.c_size_t(0)
        ov = C.c_float(0)
        self.check(lib.aicp_hip_fov_overlap(self.h, C.byref(ca), C.byref(cb), _dptr(pa), _dptr(pb), float(range_m),
                                            float(angular_view), C.byref(ov), _fptr(oa), C.byref(na), _fptr(ob),
                                            C.byref(nb)))
        return ov.value, oa[:na.value].copy(), ob[:nb.value].copy()

    def cluster_match(self, sampled_a, labels_a, sampled_b, labels_b, max_angle_deg=20.0, box_scale=(1.0, 1.0, 3.0)):
        """aicp_hip_cluster_match on two pre-filtered clouds (sampled (V, 8), labels (V,)): a dict
        with alignability, n_matches, matching_indeces / _overlap / _distance (per cluster of B),
        eigenvalues, eigenvectors (3, 3; column k for eigenvalue k), centroid, boxes_a / boxes_b
        (dicts of centre (n, 3), rot (n, 3, 3), half (n, 3)), cnt_a_in_box_b (clusters_B,
        clusters_A) and cnt_b_in_box_a (clusters_A, clusters_B)."""
        sa = np.ascontiguousarray(sampled_a, np.float32).reshape(-1, 8)
        sb = np.ascontiguousarray(sampled_b, np.float32).reshape(-1, 8)
        la = np.ascontiguousarray(labels_a, np.int32).ravel()
        lb = np.ascontiguousarray(labels_b, np.int32).ravel()
        if la.size != sa.shape[0] or lb.size != sb.shape[0]:
            raise ValueError("one label per sampled point")
        nca = int(la.max()) + 1 if la.size and la.max() >= 0 else 0
        ncb = int(lb.max()) + 1 if lb.size and lb.max() >= 0 else 0
        i32 = C.POINTER(C.c_int32)
        u32 = C.POINTER(C.c_uint32)
        al, nm = C.c_float(0), C.c_int32(0)
        mi = np.full(max(ncb, 1), -1, np.int32)
        mo = np.full(max(ncb, 1), -1, np.float32)
        md = np.full(max(ncb, 1), -1, np.float32)
        ev, evec, cen = np.zeros(3), np.zeros(9), np.zeros(3)
        ba, bb = (RiskBox * max(nca, 1))(), (RiskBox * max(ncb, 1))()
        cab = np.zeros((max(ncb, 1), max(nca, 1)), np.uint32)
        cba = np.zeros((max(nca, 1), max(ncb, 1)), np.uint32)
        sc = np.asarray(box_scale, np.float32)
        self.check(lib.aicp_hip_cluster_match(
            self.h, _fptr(sa), la.ctypes.data_as(i32), sa.shape[0], _fptr(sb), lb.ctypes.data_as(i32), sb.shape[0],
            float(max_angle_deg), _fptr(sc), C.byref(al), C.byref(nm), mi.ctypes.data_as(i32), _fptr(mo), _fptr(md),
            _dptr(ev), _dptr(evec), _dptr(cen), ba, bb, cab.ctypes.data_as(u32), cba.ctypes.data_as(u32)))

        def boxes(arr, n):
            return dict(centre=np.array([list(arr[i].centre) for i in range(n)], np.float64).reshape(n, 3),
                        rot=np.array([list(arr[i].rot) for i in range(n)], np.float64).reshape(n, 3, 3),
                        half=np.array([list(arr[i].half) for i in range(n)], np.float64).reshape(n, 3))

        return dict(alignability=al.value, n_matches=nm.value, matching_indeces=mi[:ncb].copy(),
                    matching_overlap=mo[:ncb].copy(), matching_distance=md[:ncb].copy(), eigenvalues=ev,
                    eigenvectors=evec.reshape(3, 3), centroid=cen, boxes_a=boxes(ba, nca), boxes_b=boxes(bb, ncb),
                    cnt_a_in_box_b=cab[:ncb, :nca].copy() if nca and ncb else np.zeros((ncb, nca), np.uint32),
                    cnt_b_in_box_a=cba[:nca, :ncb].copy() if nca and ncb else np.zeros((nca, ncb), np.uint32))

    def alignment_features(self, cloud_a, cloud_b, pose_a, pose_b, params=None, planes=False):
        """aicp_hip_alignment_features (App::computeAlignmentRisk up to the classifier): a dict of
        the aicp_risk_result fields; with planes=True also planes_a / planes_b, (M, 8) rows
        {x, y, z, nx, ny, nz, cluster, 0} of the matched planes."""
        prm = params or default_risk_params()
        ca, ka = make_cloud(cloud_a)
        cb, kb = make_cloud(cloud_b)
        pa, pb = _pose16(pose_a), _pose16(pose_b)
        res = RiskResult()
        cap = max(ka.shape[0], kb.shape[0], 1) if planes else 0
        qa = np.zeros((cap, 8), np.float32) if planes else None
        qb = np.zeros((cap, 8), np.float32) if planes else None
        na, nb = C.c_size_t(0), C.c_size_t(0)
        self.check(lib.aicp_hip_alignment_features(
            self.h, C.byref(prm), C.byref(ca), C.byref(cb), _dptr(pa), _dptr(pb), C.byref(res),
            _fptr(qa) if planes else None, C.byref(na), _fptr(qb) if planes else None, C.byref(nb), cap))
        d = {k: getattr(res, k) for k, _ in RiskResult._fields_ if k not in ("pad", "eigenvalues", "eigenvectors",
                                                                              "centroid")}
        d["eigenvalues"] = np.array(list(res.eigenvalues))
        d["eigenvectors"] = np.array(list(res.eigenvectors)).reshape(3, 3)
        d["centroid"] = np.array(list(res.centroid))
        if planes:
            d["planes_a"] = qa[:na.value].copy()
            d["planes_b"] = qb[:nb.value].copy()
        return d

    def last_risk_stats(self):
        st = RiskStats()
        self.check(lib.aicp_hip_last_risk_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in RiskStats._fields_}

    # -------------------------------------------------------------- classifier and gate -----
    def svm_predict(self, model: "SvmModel", samples):
        """aicp_hip_svm_predict: samples (n, 2) = (overlap percent, alignability) in one launch.
        Returns (raw float32[n], risk float64[n])."""
        x = np.ascontiguousarray(np.asarray(samples, np.float32).reshape(-1, 2))
        n = x.shape[0]
        raw, risk = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float64)
        self.check(lib.aicp_hip_svm_predict(self.h, model.h, _fptr(x), n, _fptr(raw), _dptr(risk)))
        return raw[:n], risk[:n]

    def pipeline(self, model: "SvmModel", threshold, ref, read, ref_pose, read_pose, cfg=None, risk_params=None,
                 resolution=0.2, init_T=None):
        """aicp_hip_pipeline (runAicpPipeline with failure_prediction_mode) for one pair of
        pre-filtered clouds: returns (T 4x4 row-major, record dict, stats dict)."""
        cfg = cfg or default_config()
        prm = risk_params or default_risk_params()
        p, keep = make_pair(ref, read, init_T=init_T)
        pa, pb = _pose16(ref_pose), _pose16(read_pose)
        outT = np.zeros(16, np.float32)
        rec, st = PipelineRecord(), IcpStats()
        self.check(lib.aicp_hip_pipeline(self.h, C.byref(cfg), C.byref(prm), model.h, float(threshold), C.byref(p),
                                         _dptr(pa), _dptr(pb), float(resolution), _fptr(outT), C.byref(rec),
                                         C.byref(st)))
        return outT.reshape(4, 4).T.copy(), rec.as_dict(), st.as_dict()

    def sequence_run_risk(self, model: "SvmModel", threshold, first, first_pose, readings, poses, cfg=None,
                          params=None, prefilter=None, risk_params=None, raise_on_error=True):
        """aicp_hip_sequence_run_risk: App's stream from RAW clouds with the risk gate. poses: 4x4
        row-major prior poses. Returns (T[n, 4, 4], list of result dicts, list of record dicts,
        n_done, rc)."""
        cfg = cfg or default_config()
        prm = params or default_sequence_params()
        pf = prefilter or default_prefilter()
        rp = risk_params or default_risk_params()
        n = len(readings)
        fc, keep0 = make_cloud(first, np.asarray(first_pose, np.float64)[:3, 3])
        arr = (Cloud * max(n, 1))()
        keep = [keep0]
        for i, r in enumerate(readings):
            c, k = make_cloud(r, np.asarray(poses[i], np.float64)[:3, 3])
            arr[i] = c
            keep.append(k)
        p0 = _pose16(first_pose)
        pn = np.ascontiguousarray(np.concatenate([_pose16(P) for P in poses]) if n else np.zeros(16))
        outT = np.zeros((max(n, 1), 16), np.float32)
        res = (SequenceResult * max(n, 1))()
        rec = (PipelineRecord * max(n, 1))()
        done = C.c_size_t(0)
        rc = lib.aicp_hip_sequence_run_risk(self.h, C.byref(cfg), C.byref(prm), C.byref(pf), C.byref(rp), model.h,
                                            float(threshold), C.byref(fc), _dptr(p0), arr, _dptr(pn), n, _fptr(outT),
                                            res, rec, C.byref(done))
        if raise_on_error and rc != AICP_OK:
            self.check(rc)
        T = outT[:n].reshape(-1, 4, 4).transpose(0, 2, 1).copy()
        k = done.value
        return T, [res[i].as_dict() for i in range(k)], [rec[i].as_dict() for i in range(k)], k, rc


    # -------------------------------------------------------------- quality monitor ---------
    @staticmethod
    def _monitor_params(cfg, params):
        prm = MonitorParams.from_buffer_copy(params) if params is not None else default_monitor_params()
        if cfg is not None:
            prm.flags |= AICP_MON_PAIRED
        return prm

    @staticmethod
    def _T16(T, n):
        if T is None:
            return None
        t = np.asarray(T, np.float32).reshape(n, 4, 4)
        return np.ascontiguousarray(t.transpose(0, 2, 1).reshape(n, 16))

    def monitor(self, ref, out, T=None, cfg=None, params=None, distances=False):
        """aicp_hip_monitor (icpMonitor.cpp: hausdorffDistance, distancesKNN and, with a chain
        configuration `cfg`, pairedPointsMeanDistance) of the reference and the aligned reading
        `out`; with T (4x4 row-major) out = T * the given cloud, moved on the device. Returns the
        aicp_monitor_result fields as a dict ("bytes": the struct's bytes); with distances=True also
        dist_out / dist_ref, sqrtf(d2) per point of out / of ref."""
        cr, kr = make_cloud(ref)
        co, ko = make_cloud(out)
        prm = self._monitor_params(cfg, params)
        t = self._T16(T, 1)
        res = MonitorResult()
        do = np.zeros(ko.shape[0], np.float32) if distances else None
        dr = np.zeros(kr.shape[0], np.float32) if distances else None
        self.check(lib.aicp_hip_monitor(self.h, C.byref(prm), C.byref(cfg) if cfg is not None else None, C.byref(cr),
                                        C.byref(co), _fptr(t) if t is not None else None, C.byref(res),
                                        _fptr(do) if distances else None, _fptr(dr) if distances else None))
        d = res.as_dict()
        if distances:
            d["dist_out"], d["dist_ref"] = do, dr
        return d

    def monitor_batch(self, pairs, T=None, cfg=None, params=None):
        """aicp_hip_monitor_batch: pairs as align_batch takes them (dict(ref, read); read is the
        aligned reading, or the cloud that T[i] moves), T (n, 4, 4) row-major or None. One launch
        sequence for the whole batch; returns a list of result dicts."""
        n = len(pairs)
        arr = (Pair * max(n, 1))()
        keep = []
        for i, pr in enumerate(pairs):
            p, k = make_pair(pr["ref"], pr["read"])
            arr[i] = p
            keep.append(k)
        prm = self._monitor_params(cfg, params)
        t = self._T16(T, n)
        res = (MonitorResult * max(n, 1))()
        self.check(lib.aicp_hip_monitor_batch(self.h, C.byref(prm), C.byref(cfg) if cfg is not None else None, arr, n,
                                              _fptr(t) if t is not None else None, res))
        return [res[i].as_dict() for i in range(n)]

    def test_monitor_resident(self, ref, read, T, cfg=None, params=None, runs=1):
        """aicp_hip_test_monitor_resident: the monitor's resident core on ref / read (N, 3) and T
        (4x4 row-major) from guarded device buffers, `runs` times on one reference tree. Returns
        (result dict as monitor()'s, changed guard / input words, counters dict)."""
        r = np.ascontiguousarray(as_points(ref)[:, :3], np.float32)
        q = np.ascontiguousarray(as_points(read)[:, :3], np.float32)
        prm = self._monitor_params(cfg, params)
        t = self._T16(T, 1)
        res, dirty, cnt = MonitorResult(), C.c_uint64(0), (C.c_uint64 * 4)()
        self.check(lib.aicp_hip_test_monitor_resident(self.h, C.byref(prm), C.byref(cfg) if cfg is not None else None,
                                                      _fptr(r), r.shape[0], _fptr(q), q.shape[0], _fptr(t), runs,
                                                      C.byref(res), C.byref(dirty), cnt))
        return res.as_dict(), int(dirty.value), dict(zip(MONITOR_COUNTERS, (int(x) for x in cnt)))

    def last_monitor_stats(self):
        st = MonitorStats()
        self.check(lib.aicp_hip_last_monitor_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MonitorStats._fields_}


class ResidentBatch:
    """Pairs uploaded once to HBM (aicp_hip_batch_upload), run many times."""

    def __init__(self, ctx: Context, pairs):
        self.ctx = ctx
        self.n = len(pairs)
        arr = (Pair * self.n)()
        keep = []
        for i, pr in enumerate(pairs):
            p, k = make_pair(pr["ref"], pr["read"], pr.get("ref_origin", (0, 0, 0)),
                             pr.get("read_origin", (0, 0, 0)), pr.get("init_T"))
            arr[i] = p
            keep.append(k)
        h = C.c_void_p()
        rc = lib.aicp_hip_batch_upload(ctx.h, arr, self.n, C.byref(h))
        ctx.check(rc)
        self.h = h
        self.outT = np.zeros((self.n, 16), np.float32)
        self.stats = (IcpStats * self.n)()

    def run(self, cfg=None, resolution=0.2, flags=AICP_RUN_ICP | AICP_RUN_OVERLAP, raise_on_error=True):
        cfg = cfg or default_config()
        rc = lib.aicp_hip_batch_run(self.ctx.h, self.h, C.byref(cfg), float(resolution), int(flags),
                                    _fptr(self.outT), self.stats)
        if raise_on_error and rc != AICP_OK:
            self.ctx.check(rc)
        return rc

    def transforms(self):
        return self.outT.reshape(-1, 4, 4).transpose(0, 2, 1).copy()

    def stats_dicts(self):
        return [s.as_dict() for s in self.stats]

    def free(self):
        if getattr(self, "h", None):
            lib.aicp_hip_batch_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        self.free()


class MultiContext:
    """aicp_hip_multi: one context and host thread per device for independent pairs;
    the C++ host's form of the torch.distributed path in bench.py. `devices` may repeat a device."""

    def __init__(self, devices=None, n_devices: int = 0):
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = lib.aicp_hip_multi_create(arr, len(devices), C.byref(h))
        else:
            rc = lib.aicp_hip_multi_create(None, int(n_devices), C.byref(h))
        if rc != AICP_OK:
            raise AicpError(rc, f"aicp_hip_multi_create(devices={devices}, n={n_devices}) failed")
        self.h = h

    def size(self) -> int:
        return lib.aicp_hip_multi_size(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib.aicp_hip_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def align_batch(self, pairs, cfg=None, resolution=0.2, flags=AICP_RUN_ICP, raise_on_error=True):
        """Context.align_batch over the devices. Returns (T[n,4,4] row-major, stats dicts, the
        device of each pair, rc)."""
        cfg = cfg or default_config()
        arr = (Pair * len(pairs))()
        keep = []
        for i, pr in enumerate(pairs):
            p, k = make_pair(pr["ref"], pr["read"], pr.get("ref_origin", (0, 0, 0)),
                             pr.get("read_origin", (0, 0, 0)), pr.get("init_T"))
            arr[i] = p
            keep.append(k)
        outT = np.zeros((len(pairs), 16), np.float32)
        st = (IcpStats * len(pairs))()
        dev = np.zeros(len(pairs), np.int32)
        rc = lib.aicp_hip_multi_align_batch(self.h, C.byref(cfg), arr, len(pairs), float(resolution), int(flags),
                                            _fptr(outT), st, dev.ctypes.data_as(C.POINTER(C.c_int)))
        if raise_on_error and rc != AICP_OK:
            raise AicpError(rc, lib.aicp_hip_multi_last_error(self.h).decode())
        T = outT.reshape(-1, 4, 4).transpose(0, 2, 1).copy()
        return T, [s.as_dict() for s in st], dev, rc
