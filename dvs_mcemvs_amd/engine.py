"""ctypes binding of include/dsi_engine.h.  Host-side mirror of the reference's
operator interface on the hot path:

    Grid3D       cartesian3dgrid/include/cartesian3dgrid/cartesian3dgrid.h:22-247
    MapperEMVS   mapper_emvs_stereo/include/mapper_emvs_stereo/mapper_emvs_stereo.hpp:94-155
    ShapeDSI     mapper_emvs_stereo.hpp:40-65

Method names, argument meaning and error behaviour follow the reference; where the
reference aborts (glog CHECK) or throws std::out_of_range this binding raises
DsiError carrying the C status code.  numpy arrays cross the boundary as plain
pointers; nothing here computes on the CPU.
"""
import atexit
import collections
import ctypes as C
import os
import sys
import weakref

import numpy as np

PACKET_SIZE = 1024

FUSE_MIN, FUSE_HM, FUSE_GM, FUSE_AM, FUSE_RMS, FUSE_MAX = 1, 2, 3, 4, 5, 6
ACC_SUM, ACC_INV_SUM, ACC_LOG_SUM, ACC_SQ_SUM, ACC_MIN, ACC_MAX, ACC_GM_TREE = 0, 1, 2, 3, 4, 5, 6
REDUCE_SUM, REDUCE_MIN, REDUCE_MAX = 0, 1, 2
VOTE_AUTO, VOTE_GLOBAL_ATOMIC, VOTE_LDS_BANDS, VOTE_FUSED_ARGMAX = 0, 1, 2, 3
FOCUS_LOCAL_VAR, FOCUS_LOCAL_MS, FOCUS_GRAD_MAG, FOCUS_LAPLACIAN, FOCUS_DOG = 0, 1, 2, 3, 4
GRID_OP_SUBTRACT, GRID_OP_RATIO, GRID_OP_QUADRATIC_MEAN, GRID_OP_CUBIC_MEAN = 1, 2, 3, 4
LENS_PLUMB_BOB, LENS_FISHEYE = 0, 1

(OK, ERR_INVALID, ERR_TOO_FEW_EVENTS, ERR_HIP, ERR_SHAPE, ERR_BAD_OP, ERR_NO_DEVICE,
 ERR_CONTEXT, ERR_COMM) = range(9)
COMM_ID_BYTES = 128

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class DsiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("dsi_engine error %d: %s" % (code, message))
        self.code = code


class _MapperConfig(C.Structure):
    _fields_ = [("sensor_width", C.c_int), ("sensor_height", C.c_int), ("K", C.c_float * 4),
                ("dim_x", C.c_int), ("dim_y", C.c_int), ("dim_z", C.c_int),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("fov_deg", C.c_float),
                ("inverse_depth", C.c_int), ("lut", C.POINTER(C.c_float)),
                ("plane_begin", C.c_int), ("plane_count", C.c_int)]


class _Lens(C.Structure):
    _fields_ = [("model", C.c_int), ("n_dist", C.c_int), ("K", C.c_double * 9), ("D", C.c_double * 8),
                ("R", C.c_double * 9), ("P", C.c_double * 12)]


class _DepthMapOptions(C.Structure):
    _fields_ = [("adaptive_threshold_kernel_size", C.c_int), ("adaptive_threshold_c", C.c_double),
                ("median_filter_size", C.c_int), ("max_confidence", C.c_double)]


class _PointCloudOptions(C.Structure):
    _fields_ = [("radius_search", C.c_float), ("min_num_neighbors", C.c_int)]


class _MapInfo(C.Structure):
    _fields_ = [("leaf", C.c_double), ("capacity", C.c_uint64), ("occupied", C.c_uint64), ("calls", C.c_uint64),
                ("accepted", C.c_uint64), ("rejected", C.c_uint64), ("growths", C.c_uint64)]


class _MapView(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("splat", C.c_int32), ("min_points", C.c_uint32),
                ("min_windows", C.c_uint32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("min_depth", C.c_double), ("max_depth", C.c_double), ("T_v_w", C.c_double * 12)]


class _MapRenderInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_cells", C.c_uint64), ("n_clipped", C.c_uint64),
                ("n_outside", C.c_uint64), ("n_drawn", C.c_uint64), ("n_pixels", C.c_uint64)]


class _MapCompareOpts(C.Structure):
    _fields_ = [("min_points_a", C.c_uint32), ("min_windows_a", C.c_uint32), ("min_points_b", C.c_uint32),
                ("min_windows_b", C.c_uint32), ("radius", C.c_double), ("n_bins", C.c_int32)]


class _MapCompareInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_matched", C.c_uint64), ("n_unmatched", C.c_uint64), ("sum_q", C.c_uint64),
                ("reach", C.c_int32)]


class _MapPruneOpts(C.Structure):
    _fields_ = [("min_points", C.c_uint32), ("min_windows", C.c_uint32), ("max_age", C.c_int64), ("use_box", C.c_int32),
                ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3), ("reach", C.c_int32), ("min_neighbors", C.c_uint32),
                ("shrink", C.c_int32)]


class _MapPruneInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_kept", C.c_uint64), ("n_removed", C.c_uint64 * 5), ("capacity", C.c_uint64)]


class _MapComponentsOpts(C.Structure):
    _fields_ = [("min_points", C.c_uint32), ("min_windows", C.c_uint32), ("connectivity", C.c_int32)]


class _MapComponentsInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_unlabelled", C.c_uint64), ("n_components", C.c_uint64), ("n_singletons", C.c_uint64),
                ("largest_label", C.c_uint64), ("largest_cells", C.c_uint64), ("largest_points", C.c_uint64)]


class _MapComponentsSelection(C.Structure):
    _fields_ = [("min_cells", C.c_uint64), ("min_component_points", C.c_uint64), ("keep_largest", C.c_int32), ("shrink", C.c_int32)]


class _MapComponentsSelectInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_kept", C.c_uint64), ("n_removed", C.c_uint64 * 4), ("n_components_kept", C.c_uint64),
                ("capacity", C.c_uint64)]


class _MapKnnOpts(C.Structure):
    _fields_ = [("min_points", C.c_uint32), ("min_windows", C.c_uint32), ("k", C.c_int32), ("min_found", C.c_int32),
                ("radius", C.c_double)]


class _MapKnnInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_unqueried", C.c_uint64), ("n_scored", C.c_uint64), ("n_isolated", C.c_uint64),
                ("sum_q", C.c_uint64), ("sum_q2", C.c_uint64 * 2), ("reach", C.c_int32)]


class _MapKnnSelection(C.Structure):
    _fields_ = [("std_mult", C.c_double), ("shrink", C.c_int32)]


class _MapKnnSelectInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_kept", C.c_uint64), ("n_removed", C.c_uint64 * 3), ("T_q", C.c_uint64),
                ("mu", C.c_double), ("sigma", C.c_double), ("capacity", C.c_uint64)]


class _MapPcaOpts(C.Structure):
    _fields_ = [("min_points", C.c_uint32), ("min_windows", C.c_uint32), ("k", C.c_int32), ("min_found", C.c_int32),
                ("radius", C.c_double), ("orient", C.c_int32), ("keep_moments", C.c_int32), ("viewpoint", C.c_double * 3)]


class _MapPcaInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_unqueried", C.c_uint64), ("n_sparse", C.c_uint64), ("n_label", C.c_uint64 * 3),
                ("n_normal_determined", C.c_uint64), ("n_tangent_determined", C.c_uint64), ("sum_members", C.c_uint64),
                ("reach", C.c_int32)]


class _PcaRow(C.Structure):
    _fields_ = [("normal_d", C.c_double * 3), ("tangent_d", C.c_double * 3), ("lambda_", C.c_double * 3),
                ("normal", C.c_float * 3), ("tangent", C.c_float * 3), ("eval", C.c_float * 3), ("label", C.c_uint8),
                ("flags", C.c_uint8)]


class _MapPcaSelection(C.Structure):
    _fields_ = [("keep_labels", C.c_uint32), ("remove_sparse", C.c_int32), ("shrink", C.c_int32)]


class _MapPcaSelectInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_kept", C.c_uint64), ("n_removed", C.c_uint64 * 3), ("capacity", C.c_uint64)]


class _MapObservation(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("window", C.c_int32), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double), ("abs_tol", C.c_double),
                ("rel_tol", C.c_double), ("T_v_w", C.c_double * 12)]


class _MapObserveInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_clipped", C.c_uint64), ("n_outside", C.c_uint64), ("n_unseen", C.c_uint64),
                ("n_agree", C.c_uint64), ("n_through", C.c_uint64), ("n_behind", C.c_uint64), ("n_valid_pixels", C.c_uint64),
                ("views", C.c_uint64)]


class _MapVisibilitySelection(C.Structure):
    _fields_ = [("min_through", C.c_uint32), ("agree_weight", C.c_uint32), ("shrink", C.c_int32)]


class _MapVisibilitySelectInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_kept", C.c_uint64), ("n_removed", C.c_uint64), ("capacity", C.c_uint64)]


class _MapState(C.Structure):
    _fields_ = [("leaf", C.c_double), ("n_cells", C.c_uint64), ("calls", C.c_uint64), ("accepted", C.c_uint64),
                ("rejected", C.c_uint64)]


class _MapMergeInfo(C.Structure):
    _fields_ = [("n_src_cells", C.c_uint64), ("n_new", C.c_uint64), ("n_common", C.c_uint64), ("capacity", C.c_uint64),
                ("growths", C.c_uint64)]


class _MapAlignOpts(C.Structure):
    _fields_ = [("min_points_a", C.c_uint32), ("min_windows_a", C.c_uint32), ("min_points_b", C.c_uint32),
                ("min_windows_b", C.c_uint32), ("radius", C.c_double), ("max_iterations", C.c_int32), ("reserved", C.c_int32),
                ("min_matched", C.c_uint64), ("eps_rot", C.c_double), ("eps_trans", C.c_double)]


class _MapAlignMoments(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_matched", C.c_uint64), ("n_unmatched", C.c_uint64), ("su", C.c_int64 * 3),
                ("sv", C.c_int64 * 3), ("suv_hi", C.c_int64 * 9), ("suv_lo", C.c_uint64 * 9), ("e2", C.c_uint64),
                ("quantum", C.c_double), ("reach", C.c_int32), ("reserved", C.c_int32)]


class _MapAlignSolveInfo(C.Structure):
    _fields_ = [("n_matched", C.c_uint64), ("rms", C.c_double), ("angle", C.c_double), ("trans", C.c_double),
                ("lambda_", C.c_double * 2)]


class _MapAlignInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("stopped", C.c_int32), ("reach", C.c_int32),
                ("n_cells", C.c_uint64), ("n_matched_first", C.c_uint64), ("n_matched_last", C.c_uint64),
                ("rms_first", C.c_double), ("rms_last", C.c_double), ("angle_last", C.c_double), ("trans_last", C.c_double)]


class _ScatterPlan(C.Structure):
    _fields_ = [("q", C.c_int), ("own_begin", C.c_int), ("own_count", C.c_int), ("tail_begin", C.c_int),
                ("tail_count", C.c_int)]


class _ProveInfo(C.Structure):
    _fields_ = [("rel_gap", C.c_float), ("columns", C.c_longlong), ("columns_proven", C.c_longlong),
                ("columns_unproven", C.c_longlong), ("gap_needed", C.c_double), ("max_votes", C.c_longlong),
                ("elapsed_ms", C.c_float), ("columns_resolved_fully", C.c_longlong)]


class _ResolveInfo(C.Structure):
    _fields_ = [("rel_gap", C.c_float), ("near_tie_pixels", C.c_int), ("candidate_voxels", C.c_int),
                ("candidate_planes", C.c_int), ("votes", C.c_longlong), ("changed_pixels", C.c_int),
                ("max_rel_bound", C.c_double), ("max_order_diff", C.c_double), ("elapsed_ms", C.c_float),
                ("gap_widenings", C.c_int), ("premise_ok", C.c_int), ("columns_bounded", C.c_int)]


class _VoteInfo(C.Structure):
    _fields_ = [("algo", C.c_int), ("bands", C.c_int), ("band_rows", C.c_int),
                ("chunks", C.c_int), ("block_threads", C.c_int), ("lds_bytes", C.c_size_t),
                ("n_packets", C.c_size_t), ("packed", C.c_int), ("group_packets", C.c_int)]


class _ScoreMetrics(C.Structure):
    _fields_ = [("n_est", C.c_uint64), ("n_gt", C.c_uint64), ("n_joint", C.c_uint64), ("n_delta", C.c_uint64 * 3),
                ("n_bad", C.c_uint64), ("n_stored", C.c_uint64), ("overflow", C.c_int32), ("guard_intact", C.c_int32),
                ("sum_di", C.c_double), ("sum_di2", C.c_double), ("sum_are", C.c_double), ("sum_abs", C.c_double),
                ("max_gt", C.c_double), ("delta", C.c_double * 3), ("silog", C.c_double), ("are", C.c_double),
                ("lrmse", C.c_double), ("badp", C.c_double), ("mean_abs", C.c_double), ("median_abs", C.c_double)]


def experiments_requested():
    """DSI_ENGINE_EXPERIMENTS=1 in the environment of THIS process: load the experiments flavour of the library
    (libdsi_engine_experiments.so: environment knobs + dsi_test_* hooks of the timing experiments, some of which make
    the DSIs wrong on purpose).  An explicit opt-in of development tools and of the tests of those hooks; nothing in the
    product sets it."""
    return os.environ.get("DSI_ENGINE_EXPERIMENTS", "0") not in ("", "0")


def library_path():
    return os.path.join(_HERE, "libdsi_engine_experiments.so" if experiments_requested() else "libdsi_engine.so")


def load_library():
    """Load libdsi_engine.so (building it is __graft_entry__.build()'s job).
    Raises when it is absent -- there is no fallback implementation."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: build the HIP engine first (python -m dvs_mcemvs_amd.build%s). "
            "dvs_mcemvs_amd has no CPU fallback." % (path, " --experiments" if experiments_requested() else ""))
    L = C.CDLL(path)
    L.dsi_build_flavour.restype = C.c_int
    if bool(L.dsi_build_flavour()) != experiments_requested():
        raise ImportError("%s is the %s flavour of the engine but the %s one was asked for: rebuild it "
                          "(python -m dvs_mcemvs_amd.build --force)" %
                          (path, "experiments" if L.dsi_build_flavour() else "production",
                           "experiments" if experiments_requested() else "production"))
    vp, f32p, u8p, u16p, u32p, f64p = (C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                       C.POINTER(C.c_uint16), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_double))
    intp, szp, u64p = C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)
    sig = {
        "dsi_last_error": (C.c_char_p, []),
        "dsi_abi_version": (C.c_int, []),
        "dsi_mapper_plane_begin": (C.c_int, [vp]),
        "dsi_mapper_full_depths": (C.c_int, [vp, f32p, intp]),
        "dsi_device_count": (C.c_int, []),
        "dsi_context_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "dsi_context_destroy": (C.c_int, [vp]),
        "dsi_context_synchronize": (C.c_int, [vp]),
        "dsi_context_stream": (vp, [vp]),
        "dsi_context_wait_for": (C.c_int, [vp, vp]),
        "dsi_context_device": (C.c_int, [vp]),
        "dsi_context_timer_start": (C.c_int, [vp]),
        "dsi_context_timer_stop": (C.c_int, [vp, f32p]),
        "dsi_context_timeline_mark": (C.c_int, [vp]),
        "dsi_context_timeline_read": (C.c_int, [vp, f32p, C.c_size_t, szp]),
        "dsi_build_flavour": (C.c_int, []),
        "dsi_mapper_vote_statistics": (C.c_int, [vp, vp, f64p, f64p]),
        "dsi_grid_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "dsi_grid_wrap": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]),
        "dsi_grid_destroy": (C.c_int, [vp]),
        "dsi_grid_dims": (C.c_int, [vp, intp, intp, intp]),
        "dsi_grid_reset": (C.c_int, [vp]),
        "dsi_grid_device_ptr": (vp, [vp]),
        "dsi_grid_upload": (C.c_int, [vp, f32p]),
        "dsi_grid_download": (C.c_int, [vp, f32p]),
        "dsi_grid_fuse2": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_fuse2_into": (C.c_int, [vp, vp, vp, C.c_int]),
        "dsi_grid_fuse_hm_n": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_accumulate": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_finalize": (C.c_int, [vp, C.c_int, C.c_int]),
        "dsi_grid_accumulate_begin": (C.c_int, [vp, C.c_int]),
        "dsi_grid_fuse_n": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_int]),
        "dsi_acc_reduce_op": (C.c_int, [C.c_int]),
        "dsi_grid_collapse_max_z": (C.c_int, [vp, f32p, u8p]),
        "dsi_grid_collapse_max_z_dev": (C.c_int, [vp, vp, vp, vp, vp]),
        "dsi_grid_mean_square": (C.c_int, [vp, f64p]),
        "dsi_grid_collapse_focus": (C.c_int, [vp, C.c_int, C.c_int, f32p, u8p]),
        "dsi_grid_collapse_focus_dev": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "dsi_grid_collapse_min_z": (C.c_int, [vp, f32p, u8p]),
        "dsi_grid_local_focus": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_binary_op": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_min_max": (C.c_int, [vp, f32p, f32p, u64p, u64p]),
        "dsi_grid_get_slice": (C.c_int, [vp, C.c_uint, C.c_uint, f32p]),
        "dsi_grid_get_slice_dev": (C.c_int, [vp, C.c_uint, C.c_uint, vp]),
        "dsi_grid_accumulate_z_slice": (C.c_int, [vp, C.c_uint, f32p, C.c_int, C.c_int]),
        "dsi_grid_value_at": (C.c_int, [vp, C.c_uint64, f32p]),
        "dsi_grid_set_value_at": (C.c_int, [vp, C.c_uint64, C.c_float]),
        "dsi_grid_accumulate_value_at": (C.c_int, [vp, C.c_uint64, C.c_float]),
        "dsi_grid_slices_u8": (C.c_int, [vp, C.c_uint, C.c_int, u8p]),
        "dsi_grid_slices_u8_dev": (C.c_int, [vp, C.c_uint, C.c_int, vp]),
        "dsi_grid_laplacian": (C.c_int, [vp]),
        "dsi_grid_smooth_diffuse": (C.c_int, [vp, C.c_float, intp]),
        "dsi_grid_smooth_iir": (C.c_int, [vp, C.c_float, C.c_float, C.c_float, C.c_int]),
        "dsi_grid_mean_std": (C.c_int, [vp, f64p, f64p]),
        "dsi_grid_moran_index": (C.c_int, [vp, C.c_float, f64p]),
        "dsi_mapper_create": (C.c_int, [vp, C.POINTER(_MapperConfig), C.POINTER(vp)]),
        "dsi_mapper_destroy": (C.c_int, [vp]),
        "dsi_mapper_grid": (vp, [vp]),
        "dsi_mapper_geometry": (C.c_int, [vp, f32p, f32p, intp, intp, intp]),
        "dsi_mapper_set_vote_algo": (C.c_int, [vp, C.c_int]),
        "dsi_mapper_set_band_params": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "dsi_mapper_set_packed_lanes": (C.c_int, [vp, C.c_int]),
        "dsi_mapper_set_inline_cuts": (C.c_int, [vp, C.c_longlong]),
        "dsi_mapper_paired_overflow": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "dsi_mapper_fill_voxel_grid": (C.c_int, [vp, f32p, f32p, C.c_size_t]),
        "dsi_batch_create": (C.c_int, [vp, u16p, u16p, C.c_size_t, u32p, f32p, C.c_size_t,
                                       C.POINTER(vp)]),
        "dsi_batch_destroy": (C.c_int, [vp]),
        "dsi_batch_create_async": (C.c_int, [vp, u16p, u16p, C.c_size_t, u32p, f32p, C.c_size_t,
                                             C.POINTER(vp)]),
        "dsi_batch_uploaded": (C.c_int, [vp]),
        "dsi_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(vp)]),
        "dsi_host_free": (C.c_int, [vp]),
        "dsi_mapper_fetch_depth_map_async": (C.c_int, [vp, f32p, f32p, u8p]),
        "dsi_mapper_fetch_depth_map_in_order": (C.c_int, [vp, f32p, f32p, u8p]),
        "dsi_mapper_fetch_wait": (C.c_int, [vp]),
        "dsi_batch_num_packets": (C.c_size_t, [vp]),
        "dsi_mapper_evaluate_batch": (C.c_int, [vp, vp]),
        "dsi_mapper_evaluate": (C.c_int, [vp, u16p, u16p, f64p, C.c_size_t, f64p, f64p,
                                          C.c_size_t, f64p, szp]),
        "dsi_packetize": (C.c_int, [f64p, C.c_size_t, f64p, f64p, C.c_size_t, f64p, u32p, f32p,
                                    szp]),
        "dsi_packetize_strided": (C.c_int, [vp, C.c_size_t, C.c_size_t, f64p, f64p, C.c_size_t, f64p, u32p, f32p, szp]),
        "dsi_pose_at": (C.c_int, [f64p, f64p, C.c_size_t, C.c_double, f64p]),
        "dsi_mapper_depth_map": (C.c_int, [vp, f32p, f32p, u8p]),
        "dsi_mapper_depth_map_of": (C.c_int, [vp, vp]),
        "dsi_mapper_depth_map_of_focus": (C.c_int, [vp, vp, C.c_int]),
        "dsi_mapper_fetch_depth_map": (C.c_int, [vp, f32p, f32p, u8p]),
        "dsi_mapper_depth_map_of_fusion": (C.c_int, [vp, vp, vp, C.c_int]),
        "dsi_mapper_depth_map_of_fusion_n": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_int]),
        "dsi_mapper_depth_map_of_events": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int]),
        "dsi_mapper_depth_map_of_events_n": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int]),
        "dsi_mapper_depth_map_of_events_alg2": (C.c_int, [vp, vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int]),
        "dsi_alg2_subintervals": (C.c_int, [C.c_size_t, C.c_int, C.c_int, C.c_int, szp]),
        "dsi_alg2_plan": (C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int]),
        "dsi_mapper_get_depth_map_from_dsi": (C.c_int, [vp, vp, C.POINTER(_DepthMapOptions), f32p, f32p,
                                                       u8p, u8p]),
        "dsi_mapper_filter_depth_map": (C.c_int, [vp, C.POINTER(_DepthMapOptions), f32p, f32p, u8p, u8p]),
        "dsi_mapper_get_pointcloud": (C.c_int, [vp, f32p, u8p, C.POINTER(_PointCloudOptions), f32p, C.c_size_t, szp,
                                                szp]),
        "dsi_radius_outlier_removal": (C.c_int, [vp, f32p, C.c_size_t, C.c_size_t, C.c_float, C.c_int, u8p]),
        "dsi_invert_pose": (C.c_int, [f64p, f64p]),
        "dsi_map_create": (C.c_int, [vp, C.c_double, C.c_int, C.POINTER(vp)]),
        "dsi_map_destroy": (C.c_int, [vp]),
        "dsi_map_reset": (C.c_int, [vp]),
        "dsi_map_integrate": (C.c_int, [vp, f32p, C.c_size_t, C.c_size_t, f64p, szp]),
        "dsi_map_integrate_mapper": (C.c_int, [vp, vp, C.POINTER(_PointCloudOptions), f64p, szp, szp]),
        "dsi_map_info": (C.c_int, [vp, C.POINTER(_MapInfo)]),
        "dsi_map_count": (C.c_int, [vp, C.c_uint32, C.c_uint32, szp]),
        "dsi_map_extract": (C.c_int, [vp, C.c_uint32, C.c_uint32, f32p, u32p, u32p, u64p, C.c_size_t, szp]),
        "dsi_map_render": (C.c_int, [vp, C.POINTER(_MapView), C.POINTER(_MapRenderInfo)]),
        "dsi_map_render_fetch": (C.c_int, [vp, f32p, u32p, u32p, u8p]),
        "dsi_score_add_map_render": (C.c_int, [vp, vp, f32p]),
        "dsi_score_add_map_render_gt": (C.c_int, [vp, vp, vp]),
        "dsi_event_image": (C.c_int, [vp, u16p, u16p, u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, u8p, szp]),
        "dsi_event_image_dev": (C.c_int, [vp, u16p, u16p, u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, vp]),
        "dsi_batch_event_image": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_int, u8p, szp]),
        "dsi_batch_event_image_dev": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_int, vp, vp]),
        "dsi_depth_images": (C.c_int, [vp, f32p, f32p, u8p, C.c_int, C.c_int, C.c_float, C.c_float, u8p, u8p, u8p]),
        "dsi_mapper_depth_images": (C.c_int, [vp, C.c_float, C.c_float, u8p, u8p, u8p]),
        "dsi_default_jet_lut": (C.c_int, [u8p]),
        "dsi_score_create": (C.c_int, [vp, C.c_size_t, C.c_double, C.c_double, C.c_double, C.POINTER(vp)]),
        "dsi_score_destroy": (C.c_int, [vp]),
        "dsi_score_reset": (C.c_int, [vp]),
        "dsi_score_add": (C.c_int, [vp, f32p, u8p, f32p, C.c_size_t]),
        "dsi_score_add_dev": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "dsi_score_add_mapper": (C.c_int, [vp, vp, f32p]),
        "dsi_score_metrics": (C.c_int, [vp, C.POINTER(_ScoreMetrics)]),
        "dsi_score_median": (C.c_int, [vp, f64p]),
        "dsi_score_histogram": (C.c_int, [vp, C.c_double, u64p, C.c_size_t, szp, f64p, f64p]),
        "dsi_gt_create": (C.c_int, [vp, C.c_int, C.c_int, f64p, f64p, f64p, C.c_int, C.POINTER(vp)]),
        "dsi_gt_destroy": (C.c_int, [vp]),
        "dsi_gt_project": (C.c_int, [vp, f32p]),
        "dsi_gt_project_u16": (C.c_int, [vp, u16p]),
        "dsi_gt_fetch": (C.c_int, [vp, f32p, u64p, u64p]),
        "dsi_gt_device_ptr": (vp, [vp]),
        "dsi_score_add_gt": (C.c_int, [vp, f32p, u8p, C.c_size_t, vp]),
        "dsi_score_add_mapper_gt": (C.c_int, [vp, vp, vp]),
        "dsi_depth_erode": (C.c_int, [vp, f32p, u8p, C.c_int, C.c_int, C.c_float, f32p, u8p]),
        "dsi_lens_check": (C.c_int, [C.POINTER(_Lens)]),
        "dsi_lens_rr": (C.c_int, [C.POINTER(_Lens), f64p]),
        "dsi_rectify_lut": (C.c_int, [vp, C.POINTER(_Lens), C.c_int, C.c_int, f32p]),
        "dsi_rectify_lut_dev": (C.c_int, [vp, C.POINTER(_Lens), C.c_int, C.c_int, vp]),
        "dsi_mapper_create_with_lens": (C.c_int, [vp, C.POINTER(_MapperConfig), C.POINTER(_Lens), C.POINTER(vp)]),
        "dsi_mapper_last_vote_info": (C.c_int, [vp, C.POINTER(_VoteInfo)]),
        "dsi_mapper_set_kernel_timing": (C.c_int, [vp, C.c_int]),
        "dsi_mapper_vote_kernel_time": (C.c_int, [vp, f32p, intp]),
        "dsi_comm_unique_id": (C.c_int, [u8p]),
        "dsi_comm_create_rank": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.POINTER(vp)]),
        "dsi_comm_create_all": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp)]),
        "dsi_comm_destroy": (C.c_int, [vp]),
        "dsi_comm_rank": (C.c_int, [vp]),
        "dsi_comm_size": (C.c_int, [vp]),
        "dsi_grid_allreduce": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_allreduce_all": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int]),
        "dsi_mapper_depth_map_sharded": (C.c_int, [vp, vp, vp]),
        "dsi_mapper_depth_map_sharded_all": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int]),
        "dsi_mapper_depth_map_reduce_scattered": (C.c_int, [vp, vp, vp, C.c_int, C.c_int]),
        "dsi_mapper_depth_map_reduce_scattered_all": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int,
                                                              C.c_int, C.c_int]),
        "dsi_comm_query": (C.c_int, [vp, intp, intp, intp]),
        "dsi_scatter_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_ScatterPlan)]),
        "dsi_plane_range": (C.c_int, [C.c_int, C.c_int, C.c_int, intp, intp]),
        "dsi_argmax_keys_pack": (C.c_int, [f32p, u8p, C.c_size_t, C.c_int, u64p]),
        "dsi_argmax_keys_unpack": (C.c_int, [u64p, C.c_size_t, f32p, u8p]),
        "dsi_mapper_depth_map_scattered_local": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "dsi_mapper_argmax_keys_download": (C.c_int, [vp, u64p]),
        "dsi_mapper_argmax_keys_upload": (C.c_int, [vp, u64p]),
        "dsi_mapper_depth_map_from_keys": (C.c_int, [vp]),
        "dsi_mapper_resolve_near_ties": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int,
                                                  C.POINTER(_ResolveInfo)]),
        "dsi_mapper_prove_near_ties": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(_ProveInfo)]),
        "dsi_mapper_prove_near_ties_n": (C.c_int, [vp, vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(_ProveInfo)]),
        "dsi_mapper_reference_interval": (C.c_int, [vp, vp, vp, vp, vp]),
        "dsi_grid_widen_interval": (C.c_int, [vp, vp, C.c_int]),
        "dsi_grid_prove_columns": (C.c_int, [vp, vp, vp, vp, C.POINTER(_ProveInfo)]),
        "dsi_mapper_proof_votes": (C.c_int, [vp, C.c_int, u32p, C.c_size_t, u32p]),
        "dsi_mapper_proof_unproven": (C.c_int, [vp, u32p, f32p, C.c_size_t, szp]),
        "dsi_grid_near_tie_voxels": (C.c_int, [vp, vp, C.c_float, u32p, C.c_size_t, szp, szp]),
        "dsi_mapper_exact_voxels": (C.c_int, [vp, vp, u32p, C.c_size_t, f32p, u32p]),
        "dsi_reference_fuse2": (C.c_int, [C.c_int, f32p, f32p, C.c_size_t, f32p]),
        "dsi_reference_accumulate": (C.c_int, [C.c_int, f32p, f32p, C.c_size_t]),
        "dsi_reference_finalize": (C.c_int, [C.c_int, f32p, C.c_size_t, C.c_int]),
        "dsi_mapper_patch_depth_map": (C.c_int, [vp, u32p, u8p, f32p, C.c_size_t]),
        # include/dsi_map_eval.h: the map scored in 3-D
        "dsx_map_integrate_depth": (C.c_int, [vp, f32p, u8p, C.c_int32, C.c_int32] + [C.c_double] * 6 + [f64p, u64p, u64p]),
        "dsx_map_integrate_depth_gt": (C.c_int, [vp, vp] + [C.c_double] * 6 + [f64p, u64p, u64p]),
        "dsx_map_compare": (C.c_int, [vp, vp, C.POINTER(_MapCompareOpts), u64p, C.POINTER(_MapCompareInfo)]),
        "dsx_map_compare_fetch": (C.c_int, [vp, f32p, u64p, C.c_size_t, szp]),
        # include/dsi_map_prune.h: pruning the map
        "dsx_map_prune_classify": (C.c_int, [vp, C.POINTER(_MapPruneOpts), C.POINTER(_MapPruneInfo)]),
        "dsx_map_prune_fetch": (C.c_int, [vp, u8p, u64p, C.c_size_t, szp]),
        "dsx_map_prune": (C.c_int, [vp, C.POINTER(_MapPruneOpts), C.POINTER(_MapPruneInfo)]),
        # include/dsi_map_components.h: the map's connected components
        "dsx_map_components": (C.c_int, [vp, C.POINTER(_MapComponentsOpts), C.POINTER(_MapComponentsInfo)]),
        "dsx_map_components_fetch": (C.c_int, [vp, u64p, u64p, u8p, C.c_size_t, szp]),
        "dsx_map_components_list": (C.c_int, [vp, u64p, u64p, u64p, C.c_size_t, szp]),
        "dsx_map_components_select": (C.c_int, [vp, C.POINTER(_MapComponentsSelection), C.POINTER(_MapComponentsSelectInfo)]),
        "dsx_map_prune_components": (C.c_int, [vp, C.POINTER(_MapComponentsSelection), C.POINTER(_MapComponentsSelectInfo)]),
        # include/dsi_map_knn.h: the map's k nearest cells and its statistical outliers
        "dsx_map_knn_points": (C.c_int, [vp, f32p, C.c_size_t, C.c_size_t, C.POINTER(_MapKnnOpts), u64p, f32p, u8p]),
        "dsx_map_knn": (C.c_int, [vp, C.POINTER(_MapKnnOpts), C.POINTER(_MapKnnInfo)]),
        "dsx_map_knn_threshold": (C.c_int, [C.c_uint64, C.c_uint64, u64p, C.c_double, f64p, f64p, u64p]),
        "dsx_map_knn_select": (C.c_int, [vp, C.POINTER(_MapKnnSelection), C.POINTER(_MapKnnSelectInfo)]),
        "dsx_map_knn_fetch": (C.c_int, [vp, u64p, u8p, f32p, u32p, u8p, C.c_size_t, szp]),
        "dsx_map_prune_knn": (C.c_int, [vp, C.POINTER(_MapKnnSelection), C.POINTER(_MapKnnSelectInfo)]),
        # include/dsi_map_pca.h: the map's local shape
        "dsx_map_pca": (C.c_int, [vp, C.POINTER(_MapPcaOpts), C.POINTER(_MapPcaInfo)]),
        "dsx_map_pca_fetch": (C.c_int, [vp, u64p, f32p, f32p, f32p, u16p, u8p, u8p, C.POINTER(C.c_int64), u8p, C.c_size_t, szp]),
        "dsx_pca_solve": (C.c_int, [C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_double, C.c_int32, f64p, f64p,
                                    C.POINTER(_PcaRow)]),
        "dsx_map_pca_select": (C.c_int, [vp, C.POINTER(_MapPcaSelection), C.POINTER(_MapPcaSelectInfo)]),
        "dsx_map_prune_pca": (C.c_int, [vp, C.POINTER(_MapPcaSelection), C.POINTER(_MapPcaSelectInfo)]),
        # include/dsi_map_visibility.h: the map carved by free space
        "dsx_map_observe": (C.c_int, [vp, f32p, u8p, C.POINTER(_MapObservation), C.POINTER(_MapObserveInfo)]),
        "dsx_map_observe_mapper": (C.c_int, [vp, vp, C.POINTER(_MapObservation), C.POINTER(_MapObserveInfo)]),
        "dsx_map_visibility_clear": (C.c_int, [vp]),
        "dsx_map_visibility_fetch": (C.c_int, [vp, u64p, u32p, u32p, u32p, u8p, C.c_size_t, szp]),
        "dsx_map_visibility_select": (C.c_int, [vp, C.POINTER(_MapVisibilitySelection), C.POINTER(_MapVisibilitySelectInfo)]),
        "dsx_map_prune_visibility": (C.c_int, [vp, C.POINTER(_MapVisibilitySelection), C.POINTER(_MapVisibilitySelectInfo)]),
        # include/dsi_map_merge.h: merging maps, exporting and importing their state
        "dsx_map_export": (C.c_int, [vp, C.POINTER(_MapState), u64p, u32p, u64p, u32p, u32p, C.c_size_t, szp]),
        "dsx_map_import": (C.c_int, [vp, C.POINTER(_MapState), u64p, u32p, u64p, u32p, u32p, C.POINTER(_MapMergeInfo)]),
        "dsx_map_merge": (C.c_int, [vp, vp, C.POINTER(_MapMergeInfo)]),
        # include/dsi_map_align.h: aligning maps
        "dsx_map_align_step": (C.c_int, [vp, vp, C.POINTER(_MapAlignOpts), f64p, C.POINTER(_MapAlignMoments)]),
        "dsx_map_align_fetch": (C.c_int, [vp, u64p, u64p, f32p, C.c_size_t, szp]),
        "dsx_pose_compose": (C.c_int, [f64p, f64p, f64p]),
        "dsx_map_align_solve": (C.c_int, [C.POINTER(_MapAlignMoments), f64p, C.POINTER(_MapAlignSolveInfo)]),
        "dsx_map_align": (C.c_int, [vp, vp, C.POINTER(_MapAlignOpts), f64p, f64p, C.POINTER(_MapAlignInfo)]),
        "dsx_map_integrate_map": (C.c_int, [vp, vp, f64p, C.c_uint32, C.c_uint32, u64p, u64p]),
    }
    if experiments_requested():     # hooks that exist only in the experiments flavour
        sig.update({
            "dsi_test_div_probe": (C.c_int, [vp, f32p, f32p, C.c_size_t, f32p, f32p]),
            "dsi_test_pass_lg": (C.c_int, [vp, C.c_int]),
            "dsi_test_fused_fixed_cost": (C.c_int, [vp, C.c_int]),
            "dsi_test_fused_grid_blocks": (C.c_int, [C.c_int]),
            "dsi_test_fused_solo": (C.c_int, [vp, C.c_int]),
            "dsi_test_fused_last_launch": (C.c_int, [intp, intp, intp, intp]),
            "dsi_test_fused_trace_enable": (C.c_int, [vp, szp]),
            "dsi_test_fused_trace_read": (C.c_int, [vp, vp, C.c_size_t]),
            "dsi_test_run_length_total": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
            "dsi_test_iir_axis": (C.c_int, [vp, C.c_int, C.c_float, C.c_int, C.c_int]),
        })
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the .so does not export the ABI
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


EXPORTED_SYMBOLS = None  # filled by tests from include/dsi_engine.h


# Device objects must be released while the HIP runtime is still alive: close whatever is
# still open at interpreter exit (children before contexts), and never touch the runtime
# from __del__ once the interpreter is finalizing.
_LIVE = weakref.WeakSet()


def _track(obj):
    _LIVE.add(obj)


@atexit.register
def _close_all():
    objs = list(_LIVE)
    for o in objs:
        if not isinstance(o, Context):
            try:
                o.close()
            except Exception:
                pass
    for o in objs:
        if isinstance(o, Context):
            try:
                o.close()
            except Exception:
                pass


def _safe_del(obj):
    if sys is None or sys.is_finalizing():
        return
    try:
        obj.close()
    except Exception:
        pass


def _check(rc):
    if rc != OK:
        msg = load_library().dsi_last_error()
        raise DsiError(rc, msg.decode() if msg else "")


def _ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _info_dict(info, fields=None):
    """A ctypes struct of counts as a dict: an integer field an int, a floating one a float, an array field a list of those.
    fields: the names to take, in the dict's order (None: every field, in the struct's)."""
    out = {}
    for name in fields or [f[0] for f in info._fields_]:
        v = getattr(info, name)
        out[name] = list(v) if isinstance(v, C.Array) else v
    return out


# What WorldMap._fetch_rows is told of a fetch.  _Kind: a column's element, as numpy and as the C entry point take it.
# _Column: its name in the returned dict, its element, the shape of one row and, for an optional column, the WorldMap flag
# that says whether it is there.
_Kind = collections.namedtuple("_Kind", "dtype pointer")
_Column = collections.namedtuple("_Column", "name kind shape flag", defaults=((), None))


def _kind(ctype):
    return _Kind(np.dtype(ctype), C.POINTER(ctype))


_U8, _U16, _U32, _U64 = _kind(C.c_uint8), _kind(C.c_uint16), _kind(C.c_uint32), _kind(C.c_uint64)
_I64, _F32 = _kind(C.c_int64), _kind(C.c_float)


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def acc_reduce_op(mode):
    """REDUCE_SUM / REDUCE_MIN / REDUCE_MAX: how an accumulator of `mode` combines across GPUs."""
    r = load_library().dsi_acc_reduce_op(int(mode))
    if r < 0:
        raise DsiError(ERR_BAD_OP, "bad accumulate mode %r" % (mode,))
    return r


def device_count():
    return load_library().dsi_device_count()


class Context:
    """One GPU + one HIP stream.  All objects created from a context share its stream."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(load_library().dsi_context_create(int(device), C.byref(self._h)))
        _track(self)

    def close(self):
        if self._h:
            # objects created from this context hold a pointer to it on the C side: release whatever is
            # still open (e.g. left behind by an exception) BEFORE the context goes
            for o in list(_LIVE):
                if o is not self and getattr(o, "ctx", None) is self:
                    try:
                        o.close()
                    except Exception:
                        pass
            # (the C side refuses while children are alive: that would be a permanent leak of the stream, the pool and
            #  the scratch -- raise, and keep the handle so that a later close() can succeed)
            _check(load_library().dsi_context_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)

    def synchronize(self):
        _check(load_library().dsi_context_synchronize(self._h))

    @property
    def stream(self):
        return load_library().dsi_context_stream(self._h)

    def wait_for(self, other):
        """Device-side: work queued on this context from now on starts after everything already
        queued on `other` (no host wait)."""
        _check(load_library().dsi_context_wait_for(self._h, other._h))

    @property
    def device(self):
        return load_library().dsi_context_device(self._h)

    def timer_start(self):
        _check(load_library().dsi_context_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        _check(load_library().dsi_context_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def timeline_mark(self):
        """Record a HIP event on the stream (asynchronous); see timeline_read()."""
        _check(load_library().dsi_context_timeline_mark(self._h))

    def timeline_read(self, capacity=1 << 16):
        """Milliseconds between consecutive marks (waits for the last one; clears the timeline)."""
        out = np.zeros(capacity, np.float32)
        n = C.c_size_t()
        _check(load_library().dsi_context_timeline_read(self._h, _ptr(out, C.c_float), capacity, C.byref(n)))
        return out[:min(n.value, capacity)].copy()


class Comm:
    """One rank of an RCCL communicator created by the engine itself (include/dsi_engine.h,
    "multi-GPU"): nothing here needs torch.  One process per GPU: rank 0 makes
    `uid = Comm.unique_id()`, ships the 128 bytes to the other ranks, every rank builds
    `Comm(ctx, uid, nranks, rank)`.  One process, several GPUs: `Comm.create_all(contexts)`."""

    def __init__(self, ctx, uid, nranks, rank, _handle=None):
        self.ctx = ctx
        if _handle is not None:
            self._h = _handle
        else:
            buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
            self._h = C.c_void_p()
            _check(load_library().dsi_comm_create_rank(ctx._h, buf, int(nranks), int(rank), C.byref(self._h)))
        _track(self)

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        _check(load_library().dsi_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def create_all(cls, contexts):
        n = len(contexts)
        hs = (C.c_void_p * n)(*[c._h for c in contexts])
        out = (C.c_void_p * n)()
        _check(load_library().dsi_comm_create_all(hs, n, out))
        return [cls(contexts[i], None, n, i, _handle=C.c_void_p(out[i])) for i in range(n)]

    @property
    def rank(self):
        return load_library().dsi_comm_rank(self._h)

    @property
    def size(self):
        return load_library().dsi_comm_size(self._h)

    def query(self):
        """(nranks, rank, device) as RCCL itself reports them (ncclCommCount / ncclCommUserRank / ncclCommCuDevice)."""
        n, r, dev = C.c_int(), C.c_int(), C.c_int()
        _check(load_library().dsi_comm_query(self._h, C.byref(n), C.byref(r), C.byref(dev)))
        return n.value, r.value, dev.value

    def close(self):
        if self._h:
            load_library().dsi_comm_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)


def scatter_plan(dim_z, nranks, rank):
    """dsi_scatter_plan: which planes rank `rank` of `nranks` owns when the temporal fusion's collective is a
    reduce-scatter: dict(q, own_begin, own_count, tail_begin, tail_count) -- the arithmetic the RCCL path uses."""
    sp = _ScatterPlan()
    _check(load_library().dsi_scatter_plan(int(dim_z), int(nranks), int(rank), C.byref(sp)))
    return {k: getattr(sp, k) for k, _ in _ScatterPlan._fields_}


def plane_range(dim_z, nranks, rank):
    """dsi_plane_range: (begin, count) of rank's planes under plane sharding."""
    b, c = C.c_int(), C.c_int()
    _check(load_library().dsi_plane_range(int(dim_z), int(nranks), int(rank), C.byref(b), C.byref(c)))
    return b.value, c.value


def argmax_keys_pack(conf, idx_local, plane_begin):
    conf = _arr(conf, np.float32)
    idx_local = _arr(idx_local, np.uint8)
    keys = np.empty(conf.shape, np.uint64)
    _check(load_library().dsi_argmax_keys_pack(_ptr(conf, C.c_float), _ptr(idx_local, C.c_uint8), conf.size,
                                               int(plane_begin), _ptr(keys, C.c_uint64)))
    return keys


def argmax_keys_unpack(keys):
    keys = _arr(keys, np.uint64)
    conf = np.empty(keys.shape, np.float32)
    idx = np.empty(keys.shape, np.uint8)
    _check(load_library().dsi_argmax_keys_unpack(_ptr(keys, C.c_uint64), keys.size, _ptr(conf, C.c_float),
                                                 _ptr(idx, C.c_uint8)))
    return conf, idx


def widen_interval(lo, hi, roundings):
    """dsi_grid_widen_interval: lo <- lo (1 - k u) rounded down, hi <- hi (1 + k u) rounded up, u = 2^-24 -- after a grid op
    that performs k fp32 roundings per voxel was applied to both grids of an interval."""
    _check(load_library().dsi_grid_widen_interval(lo._h, hi._h, int(roundings)))


def reference_fuse2(op, a, g):
    """The reference's 2-ary camera-fusion op on host arrays (dsi_reference_fuse2: cartesian3dgrid.h:111-190 applied to
    a grid initialised by resetGrid(); addTwoGrids(a)), bit for bit what the device computes."""
    a, g = _arr(a, np.float32), _arr(g, np.float32)
    out = np.empty(a.shape, np.float32)
    _check(load_library().dsi_reference_fuse2(int(op), _ptr(a, C.c_float), _ptr(g, C.c_float), a.size, _ptr(out, C.c_float)))
    return out


def reference_accumulate(mode, acc, g):
    """acc + g (ACC_SUM) / acc + 1/(0.01 + g) (ACC_INV_SUM) on host arrays (cartesian3dgrid.h:64-78); returns a new array."""
    acc, g = np.array(acc, np.float32, order="C"), _arr(g, np.float32)
    _check(load_library().dsi_reference_accumulate(int(mode), _ptr(acc, C.c_float), _ptr(g, C.c_float), acc.size))
    return acc


def reference_finalize(mode, acc, n_maps):
    """acc / n (ACC_SUM) / n / acc (ACC_INV_SUM) on a host array (cartesian3dgrid.h:80-93); returns a new array."""
    acc = np.array(acc, np.float32, order="C")
    _check(load_library().dsi_reference_finalize(int(mode), _ptr(acc, C.c_float), acc.size, int(n_maps)))
    return acc


def allreduce_all(comms, grids, op):
    """All ranks of one process at once (comms from Comm.create_all; grids[i] on comms[i]'s GPU)."""
    n = len(comms)
    cs = (C.c_void_p * n)(*[c._h for c in comms])
    gs = (C.c_void_p * n)(*[g._h for g in grids])
    _check(load_library().dsi_grid_allreduce_all(cs, gs, n, int(op)))


def depth_map_reduce_scattered_all(mappers, accs, comms, mode, n_maps):
    """One process, several GPUs: MapperEMVS.computeDepthMapReduceScattered on every rank in one group call."""
    n = len(comms)
    hm = (C.c_void_p * n)(*[m._h for m in mappers])
    hg = (C.c_void_p * n)(*[g._h for g in accs])
    hc = (C.c_void_p * n)(*[c._h for c in comms])
    _check(load_library().dsi_mapper_depth_map_reduce_scattered_all(hm, hg, hc, n, int(mode), int(n_maps)))


def depth_map_sharded_all(mappers, grids, comms):
    n = len(comms)
    ms = (C.c_void_p * n)(*[m._h for m in mappers])
    gs = (C.c_void_p * n)(*[g._h for g in grids])
    cs = (C.c_void_p * n)(*[c._h for c in comms])
    _check(load_library().dsi_mapper_depth_map_sharded_all(ms, gs, cs, n))


class Grid3D:
    """Device-resident counterpart of the reference's Grid3D (cartesian3dgrid.h:22-247).

    Layout volume[x + dimX*(y + dimY*z)]; host views are numpy [dimZ][dimY][dimX].
    Fusion methods keep the reference's names and in-place semantics.
    """

    def __init__(self, ctx, dimX, dimY, dimZ, _handle=None, _owner=None, device_ptr=None):
        self.ctx = ctx
        self._owner = _owner
        self._keep = None
        L = load_library()
        if _handle is not None:
            self._h = _handle
            self._owned = False
        elif device_ptr is not None:
            self._h = C.c_void_p()
            _check(L.dsi_grid_wrap(ctx._h, dimX, dimY, dimZ, C.c_void_p(device_ptr),
                                   C.byref(self._h)))
            self._owned = True
        else:
            self._h = C.c_void_p()
            _check(L.dsi_grid_create(ctx._h, dimX, dimY, dimZ, C.byref(self._h)))
            self._owned = True
        if self._owned:
            _track(self)

    def close(self):
        if getattr(self, "_owned", False) and self._h:
            load_library().dsi_grid_destroy(self._h)
        self._h = C.c_void_p()
        self._owned = False

    def __del__(self):
        _safe_del(self)

    def getDimensions(self):
        nx, ny, nz = C.c_int(), C.c_int(), C.c_int()
        _check(load_library().dsi_grid_dims(self._h, C.byref(nx), C.byref(ny), C.byref(nz)))
        return nx.value, ny.value, nz.value

    @property
    def shape(self):
        nx, ny, nz = self.getDimensions()
        return nz, ny, nx

    @property
    def device_ptr(self):
        return load_library().dsi_grid_device_ptr(self._h)

    def resetGrid(self):
        _check(load_library().dsi_grid_reset(self._h))

    def upload(self, host):
        host = _arr(host, np.float32)
        if host.shape != self.shape:
            raise DsiError(ERR_SHAPE, "host array shape %s != grid shape %s" % (host.shape, self.shape))
        _check(load_library().dsi_grid_upload(self._h, _ptr(host, C.c_float)))

    def download(self):
        out = np.empty(self.shape, np.float32)
        _check(load_library().dsi_grid_download(self._h, _ptr(out, C.c_float)))
        return out

    # -- voxel-wise fusion, cartesian3dgrid.h:64-192 --------------------------------
    def _fuse(self, other, op):
        _check(load_library().dsi_grid_fuse2(self._h, other._h, op))

    def minTwoGrids(self, grid2):
        self._fuse(grid2, FUSE_MIN)

    def harmonicMeanTwoGrids(self, grid2, n=None):
        if n is None:
            self._fuse(grid2, FUSE_HM)
        else:
            _check(load_library().dsi_grid_fuse_hm_n(self._h, grid2._h, int(n)))

    def geometricMeanTwoGrids(self, grid2):
        self._fuse(grid2, FUSE_GM)

    def arithmeticMeanTwoGrids(self, grid2):
        self._fuse(grid2, FUSE_AM)

    def rmsTwoGrids(self, grid2):
        self._fuse(grid2, FUSE_RMS)

    def maxTwoGrids(self, grid2):
        self._fuse(grid2, FUSE_MAX)

    def fuseTwoGrids(self, grid2, fusion_method):
        """The switch(fusion_method) of process1.cpp:136-158."""
        self._fuse(grid2, int(fusion_method))

    def setToFusionOf(self, grid_a, grid_b, fusion_method):
        """self = op(grid_a, grid_b): the result of the reference's
        `resetGrid(); addTwoGrids(a); <op>TwoGrids(b)` (process1.cpp:126-158) in one pass."""
        _check(load_library().dsi_grid_fuse2_into(self._h, grid_a._h, grid_b._h, int(fusion_method)))

    def addTwoGrids(self, grid2):
        _check(load_library().dsi_grid_accumulate(self._h, grid2._h, ACC_SUM))

    def addInverseOfTwoGrids(self, grid2):
        _check(load_library().dsi_grid_accumulate(self._h, grid2._h, ACC_INV_SUM))

    def computeAMfromSum(self, n):
        _check(load_library().dsi_grid_finalize(self._h, ACC_SUM, int(n)))

    def computeHMfromSumOfInv(self, n):
        _check(load_library().dsi_grid_finalize(self._h, ACC_INV_SUM, int(n)))

    # -- n-ary accumulate / finalize (dsi_acc_mode_t): the reference's temporal accumulators
    #    (modes 0, 1) and the n-ary forms of its 2-ary camera-fusion ops (modes 2..5), which it
    #    does not have (process1.cpp:169-191 drops camera 3 for GM / AM / RMS)
    def accumulateBegin(self, mode):
        _check(load_library().dsi_grid_accumulate_begin(self._h, int(mode)))

    def accumulate(self, grid2, mode):
        _check(load_library().dsi_grid_accumulate(self._h, grid2._h, int(mode)))

    def finalize(self, mode, n):
        _check(load_library().dsi_grid_finalize(self._h, int(mode), int(n)))

    def allReduce(self, comm, op):
        """In-place RCCL all-reduce over `comm` on this grid's stream (op: REDUCE_SUM/MIN/MAX, or
        acc_reduce_op(mode) for an accumulator)."""
        _check(load_library().dsi_grid_allreduce(comm._h, self._h, int(op)))

    def setToFusionOfN(self, grids, mode):
        """self = n-ary mean of `grids`: ACC_SUM arithmetic, ACC_LOG_SUM geometric (0 where any
        grid is 0), ACC_SQ_SUM root mean square, ACC_MIN / ACC_MAX."""
        if len(grids) <= 8 and all(g is not self for g in grids):
            hs = (C.c_void_p * len(grids))(*[g._h for g in grids])   # one pass over the volumes, same bits
            _check(load_library().dsi_grid_fuse_n(self._h, hs, len(grids), int(mode)))
            return
        self.accumulateBegin(mode)
        for g in grids:
            self.accumulate(g, mode)
        self.finalize(mode, len(grids))

    # -- cartesian3dgrid.cpp:115-137, :164-174 --------------------------------------
    def collapseMaxZSlice(self):
        """Returns (max_val float32 [dimY][dimX], max_pos uint8 [dimY][dimX])."""
        nz, ny, nx = self.shape
        conf = np.empty((ny, nx), np.float32)
        idx = np.empty((ny, nx), np.uint8)
        _check(load_library().dsi_grid_collapse_max_z(self._h, _ptr(conf, C.c_float),
                                                      _ptr(idx, C.c_uint8)))
        return conf, idx

    # -- focus-based collapses, cartesian3dgrid.cpp:139-483 (arithmetic: DESIGN.md "Focus-based collapses") --------
    def _collapse_focus(self, method, half_patchsize=1):
        nz, ny, nx = self.shape
        conf = np.empty((ny, nx), np.float32)
        idx = np.empty((ny, nx), np.uint8)
        _check(load_library().dsi_grid_collapse_focus(self._h, int(method), int(half_patchsize), _ptr(conf, C.c_float),
                                                      _ptr(idx, C.c_uint8)))
        return conf, idx

    def collapseZSliceByLocalVar(self):
        """Returns (confidence float32 [dimY][dimX], depth_cell_indices uint8 [dimY][dimX])."""
        return self._collapse_focus(FOCUS_LOCAL_VAR)

    def collapseZSliceByLocalMeanSquare(self):
        return self._collapse_focus(FOCUS_LOCAL_MS)

    def collapseZSliceByGradMag(self, half_patchsize=1):
        return self._collapse_focus(FOCUS_GRAD_MAG, half_patchsize)

    def collapseZSliceByLaplacianMag(self):
        return self._collapse_focus(FOCUS_LAPLACIAN)

    def collapseZSliceByDoG(self):
        return self._collapse_focus(FOCUS_DOG)

    def collapseMinZSlice(self):
        """Returns (min_val float32 [dimY][dimX], min_pos uint8 [dimY][dimX]): the first minimum wins."""
        nz, ny, nx = self.shape
        val = np.empty((ny, nx), np.float32)
        idx = np.empty((ny, nx), np.uint8)
        _check(load_library().dsi_grid_collapse_min_z(self._h, _ptr(val, C.c_float), _ptr(idx, C.c_uint8)))
        return val, idx

    def computeLocalFocusInPlace(self, focus_method):
        """focus_method 1: Gaussian local mean square; any other value: local standard deviation."""
        _check(load_library().dsi_grid_local_focus(self._h, self._h, int(focus_method)))

    def setToLocalFocusOf(self, grid, focus_method):
        """self = grid with computeLocalFocusInPlace(focus_method) applied, in one pass (grid is unchanged)."""
        _check(load_library().dsi_grid_local_focus(self._h, grid._h, int(focus_method)))

    def computeMeanSquare(self):
        out = C.c_double()
        _check(load_library().dsi_grid_mean_square(self._h, C.byref(out)))
        return out.value

    # -- volume filters, cartesian3dgrid_filter.cpp and gaussianiir3d.cpp -------------------------------
    def laplacian(self):
        """laplacianInPlace: the 7-point Laplacian with index-clamped neighbours, in place."""
        _check(load_library().dsi_grid_laplacian(self._h))

    def smooth_diffuse(self, sigma=1.0):
        """smoothInPlace: explicit heat-equation steps, in place.  Returns the number of steps taken."""
        steps = C.c_int()
        _check(load_library().dsi_grid_smooth_diffuse(self._h, float(np.float32(sigma)), C.byref(steps)))
        return steps.value

    def smooth_iir(self, sigma_x=1.0, sigma_y=1.0, sigma_z=1.0, numsteps=3):
        """smoothInPlaceIIR3D (numsteps = 3): the recursive Gaussian of gaussianiir3d, in place.  A sigma <= 0 or
        numsteps <= 0 leaves the grid unchanged."""
        _check(load_library().dsi_grid_smooth_iir(self._h, float(np.float32(sigma_x)), float(np.float32(sigma_y)),
                                                  float(np.float32(sigma_z)), int(numsteps)))

    def mean_std(self):
        """computeMeanStd: (mean, population standard deviation), accumulated in double; the same bits on every call."""
        mean, std = C.c_double(), C.c_double()
        _check(load_library().dsi_grid_mean_std(self._h, C.byref(mean), C.byref(std)))
        return mean.value, std.value

    def moran_index(self, sigma):
        """computeMoranIndexGaussianWeights: Moran's index under Gaussian weights; the grid is not modified."""
        out = C.c_double()
        _check(load_library().dsi_grid_moran_index(self._h, float(np.float32(sigma)), C.byref(out)))
        return out.value

    laplacianInPlace = laplacian
    smoothInPlace = smooth_diffuse
    computeMeanStd = mean_std
    computeMoranIndexGaussianWeights = moran_index

    def smoothInPlaceIIR3D(self, sigma_x=1.0, sigma_y=1.0, sigma_z=1.0):
        self.smooth_iir(sigma_x, sigma_y, sigma_z, 3)

    # -- the members that are no camera fusion, cartesian3dgrid.h:95-109,166-184 ----------------
    def _binary(self, other, op):
        _check(load_library().dsi_grid_binary_op(self._h, other._h, int(op)))

    def subtractTwoGrids(self, grid2):
        self._binary(grid2, GRID_OP_SUBTRACT)

    def ratioTwoGrids(self, grid2, eps=None):
        """self /= |grid2| + 0.1f.  Only the reference's default eps is offered."""
        if eps is not None and np.float32(eps) != np.float32(1e-1):
            raise DsiError(ERR_INVALID, "ratioTwoGrids: only the default eps = 1e-1f is supported")
        self._binary(grid2, GRID_OP_RATIO)

    def quadraticMeanTwoGrids(self, grid2):
        self._binary(grid2, GRID_OP_QUADRATIC_MEAN)

    def cubicMeanTwoGrids(self, grid2):
        self._binary(grid2, GRID_OP_CUBIC_MEAN)

    # -- cartesian3dgrid.cpp:72-113, :177-188, cartesian3dgrid.h:40-58,195-204 ------------------------------------
    def getMinMax(self):
        """(min, max, min_pos, max_pos): the first smallest and the last largest element of the flat array."""
        lo, hi = C.c_float(), C.c_float()
        lo_pos, hi_pos = C.c_uint64(), C.c_uint64()
        _check(load_library().dsi_grid_min_max(self._h, C.byref(lo), C.byref(hi), C.byref(lo_pos), C.byref(hi_pos)))
        return np.float32(lo.value), np.float32(hi.value), int(lo_pos.value), int(hi_pos.value)

    def _slice_shape(self, dimIdx):
        nx, ny, nz = self.getDimensions()
        if dimIdx not in (0, 1, 2):
            raise DsiError(ERR_INVALID, "dimIdx should be 0, 1 or 2 (got %r)" % (dimIdx,))
        return ((nx, ny, nz)[dimIdx],) + ((ny, nz), (nx, nz), (ny, nx))[dimIdx]

    def getSlice(self, sliceIdx, dimIdx):
        """float32 [rows][cols]: dimIdx 0 -> (dimY, dimZ) at x, 1 -> (dimX, dimZ) at y, 2 -> (dimY, dimX) at z."""
        if sliceIdx < 0:
            raise DsiError(ERR_INVALID, "negative slice index")
        out = np.empty(self._slice_shape(dimIdx)[1:], np.float32)
        _check(load_library().dsi_grid_get_slice(self._h, int(sliceIdx), int(dimIdx), _ptr(out, C.c_float)))
        return out

    def accumulateZSliceAt(self, iz, img):
        """vol(ix, iy, iz) += img[iy, ix]; the image may be smaller than the plane."""
        img = _arr(img, np.float32)
        if img.ndim != 2 or iz < 0:
            raise DsiError(ERR_INVALID, "accumulateZSliceAt takes a 2-D image and a slice index >= 0")
        _check(load_library().dsi_grid_accumulate_z_slice(self._h, int(iz), _ptr(img, C.c_float), img.shape[0], img.shape[1]))

    def _flat(self, p, iy=None, iz=None):
        if iy is None:
            if p < 0:
                raise DsiError(ERR_INVALID, "negative voxel index")
            return int(p)
        nx, ny, nz = self.getDimensions()
        if not (0 <= p < nx and 0 <= iy < ny and 0 <= iz < nz):
            raise DsiError(ERR_INVALID, "voxel (%d,%d,%d) is outside the grid (%d,%d,%d)" % (p, iy, iz, nx, ny, nz))
        return int(p) + nx * (int(iy) + ny * int(iz))

    def getGridValueAt(self, p, iy=None, iz=None):
        """getGridValueAt(p) or getGridValueAt(ix, iy, iz)."""
        out = C.c_float()
        _check(load_library().dsi_grid_value_at(self._h, self._flat(p, iy, iz), C.byref(out)))
        return np.float32(out.value)

    def setGridValueAt(self, p, fval):
        _check(load_library().dsi_grid_set_value_at(self._h, self._flat(p), float(np.float32(fval))))

    def accumulateGridValueAt(self, p, fval):
        _check(load_library().dsi_grid_accumulate_value_at(self._h, self._flat(p), float(np.float32(fval))))

    # -- cartesian3dgrid_IO.cpp:39-76 ------------------------------------------------------------------------------
    def slicesU8(self, dimIdx, normalize_by_minmax=True):
        """Every slice of one orientation as an 8-bit image: uint8 [size[dimIdx]][rows][cols], getSlice's shapes."""
        out = np.empty(self._slice_shape(dimIdx), np.uint8)
        _check(load_library().dsi_grid_slices_u8(self._h, int(dimIdx), int(bool(normalize_by_minmax)), _ptr(out, C.c_uint8)))
        return out

    def imwriteSlices(self, prefix, dimIdx, normalize_by_minmax=True):
        """prefix + three-digit zero-padded slice index + ".png", 8-bit grayscale; returns the file names."""
        from . import io as _io
        names = []
        for i, img in enumerate(self.slicesU8(dimIdx, normalize_by_minmax)):
            names.append("%s%03d.png" % (prefix, i))
            _io.write_png_gray8(names[-1], img)
        return names


class ShapeDSI:
    """mapper_emvs_stereo.hpp:40-65"""

    def __init__(self, dimX=0, dimY=0, dimZ=100, min_depth=0.3, max_depth=5.0, fov=0.0):
        self.dimX_, self.dimY_, self.dimZ_ = int(dimX), int(dimY), int(dimZ)
        self.min_depth_, self.max_depth_, self.fov_ = float(min_depth), float(max_depth), float(fov)


class OptionsDepthMap:
    """mapper_emvs_stereo.hpp:68-82 (the fields getDepthMapFromDSI reads; defaults of main.cpp:73-75,97)."""

    def __init__(self, adaptive_threshold_kernel_size=5, adaptive_threshold_c=5.0, median_filter_size=5,
                 max_confidence=0.0):
        self.adaptive_threshold_kernel_size_ = int(adaptive_threshold_kernel_size)
        self.adaptive_threshold_c_ = float(adaptive_threshold_c)
        self.median_filter_size_ = int(median_filter_size)
        self.max_confidence = float(max_confidence)


class OptionsPointCloud:
    """mapper_emvs_stereo.hpp:84-89 (defaults of main.cpp:80-81: --radius_search, --min_num_neighbors)."""

    def __init__(self, radius_search_=0.05, min_num_neighbors_=3):
        self.radius_search_ = float(radius_search_)
        self.min_num_neighbors_ = int(min_num_neighbors_)


def radius_outlier_removal(ctx, xyz, radius, min_neighbors):
    """pcl::RadiusOutlierRemoval on the device (dsi_radius_outlier_removal): xyz (N, 3) or (N, 4) float32 -- x, y, z
    first -- to a bool keep mask.  Point i is kept iff at least min_neighbors + 1 points j (j = i and duplicates
    included) satisfy (double) d2_f32(i, j) <= (double) radius**2, d2_f32 = ((dx*dx) + dy*dy) + dz*dz in fp32 without
    FMA (FLANN's L2_Simple<float>); radius is taken as float32 like OptionsPointCloud::radius_search_."""
    xyz = _arr(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
        raise ValueError("xyz must be (N, 3) or (N, 4)")
    n = xyz.shape[0]
    keep = np.zeros(n, np.uint8)
    _check(load_library().dsi_radius_outlier_removal(ctx._h, _ptr(xyz, C.c_float), xyz.shape[1], n, C.c_float(radius),
                                                     int(min_neighbors), _ptr(keep, C.c_uint8)))
    return keep.astype(bool)


def pose_matrix(pose):
    """A pose as the 12 doubles, row-major [R | t], that the world map takes: a 7-vector (tx, ty, tz, qw, qx, qy, qz) --
    the form process.py's reference views have -- or anything of 12 numbers (3 x 4, or 4 x 4 without its last row)."""
    p = np.asarray(pose, np.float64)
    if p.shape == (4, 4):
        p = p[:3]
    if p.size == 12:
        return np.ascontiguousarray(p.reshape(12))
    if p.shape != (7,):
        raise ValueError("a pose is 7 numbers (t, q) or a 3 x 4 matrix")
    w, x, y, z = p[3:]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.ascontiguousarray(np.concatenate([R, p[:3, None]], axis=1).reshape(12))


def invert_pose(T):
    """The inverse of a rigid pose (dsi_invert_pose, the routine dsi::invert_pose calls too): T as pose_matrix takes it,
    the result 12 doubles, row-major [R | t], with R' = R^T and t'_i = -((r0i t0 + r1i t1) + r2i t2) in double without
    FMA.  Turns a window's T_rv_w into the T_w_rv that WorldMap.integrate takes."""
    T = pose_matrix(T)
    out = np.empty(12, np.float64)
    _check(load_library().dsi_invert_pose(_ptr(T, C.c_double), _ptr(out, C.c_double)))
    return out


class WorldMap:
    """A persistent world-frame map on the device (dsi_map_*): every integrate call moves one window's cloud
    from its reference view to the world frame with T_w_rv and merges it into cubic cells of edge `leaf` -- a centroid
    per cell as PCL's VoxelGrid gives, the number of points and the number of calls (windows) that reached the cell.
    The cell sums are 64-bit fixed point: the map's bits depend neither on the order of the points nor on how they are
    split into calls nor on the table's size (tests/world_map_reference.py restates the arithmetic).  capacity_log2: the
    initial table of 2**capacity_log2 slots (8..27); it doubles by itself.  render() gives the depth image the map presents
    to a camera, for DepthScore.addMapRender and renderImage."""

    def __init__(self, ctx, leaf, capacity_log2=16):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(load_library().dsi_map_create(ctx._h, float(leaf), int(capacity_log2), C.byref(self._h)))
        # what the library keeps of the last passes and does not tell: the render's size; whether a selection left reasons
        # beside the labelling, the self query, the local-shape pass and the visibility tally; whether that pass kept its moments
        self._render_shape = (0, 0)
        self._components_selected = self._knn_selected = self._pca_selected = self._pca_moments = self._visibility_selected = False
        _track(self)

    @staticmethod
    def _by_key(rows):
        order = np.argsort(rows["keys"], kind="stable")
        return {k: v[order] for k, v in rows.items()}

    def _fetch_rows(self, fn, columns, sort, lead=()):
        """The two calls of a fetch, fn(self._h, *lead, one pointer per column, capacity, &n).  The first, with no column and
        no room, asks for the number of rows: it is refused for want of room as soon as there are rows, so its refusal counts
        only when it leaves n at 0.  The second fills fresh arrays, also when there is no row.  columns: one _Column per
        pointer, in the order of fn's arguments (the table stands above each fetch); an optional column whose flag is down
        is passed as None and left out.  Returns the dict of the arrays, keys first (dsx_map_compare_fetch and
        dsx_map_prune_fetch take their values before the keys), in the table's order or, with sort, by ascending key."""
        n = C.c_size_t()
        no_columns = [None] * len(columns)
        rc = fn(self._h, *lead, *no_columns, 0, C.byref(n))
        if rc != OK and n.value == 0:
            _check(rc)
        m = n.value
        out = {c.name: np.empty((m,) + c.shape, c.kind.dtype) for c in columns if c.flag is None or getattr(self, c.flag)}
        pointers = [out[c.name].ctypes.data_as(c.kind.pointer) if c.name in out else None for c in columns]
        _check(fn(self._h, *lead, *pointers, m, C.byref(n)))
        if "keys" in out:
            out = {"keys": out.pop("keys"), **out}
        return self._by_key(out) if sort else out

    def _select(self, fn, selection, info, flag):
        """A selection or the prune by it: the flag that fetches read falls before the call and rises after it went through"""
        setattr(self, flag, False)
        _check(fn(self._h, C.byref(selection), C.byref(info)))
        setattr(self, flag, True)
        return _info_dict(info)

    def integrate(self, xyz, T_w_rv):
        """One call (window) of host points: xyz (N, 3) or (N, 4) float32, x y z first (a getPointcloud result as it is);
        T_w_rv as pose_matrix takes it.  N = 0 still counts as a call.  Returns the number of points rejected (not
        finite in the world frame, or beyond +-(2**20 - 2) cells)."""
        xyz = _arr(xyz, np.float32)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
            raise ValueError("xyz must be (N, 3) or (N, 4)")
        T = pose_matrix(T_w_rv)
        rej = C.c_size_t()
        _check(load_library().dsi_map_integrate(self._h, _ptr(xyz, C.c_float), xyz.shape[1], xyz.shape[0], _ptr(T, C.c_double),
                                                C.byref(rej)))
        return rej.value

    def integrate_mapper(self, mapper, T_w_rv, options_pc=None):
        """One call of the cloud mapper.getPointcloud(options_pc=options_pc) would return -- the filtered maps the last
        getDepthMapFromDSI(..., options_depth_map) / filterDepthMap left on the device -- without bringing it to the
        host.  The mapper must live on the map's context.  Returns (points in the cloud, points rejected)."""
        o = options_pc or OptionsPointCloud()
        opts = _PointCloudOptions(o.radius_search_, o.min_num_neighbors_)
        T = pose_matrix(T_w_rv)
        n, rej = C.c_size_t(), C.c_size_t()
        _check(load_library().dsi_map_integrate_mapper(self._h, mapper._h, C.byref(opts), _ptr(T, C.c_double), C.byref(n),
                                                       C.byref(rej)))
        return n.value, rej.value

    def count(self, min_points=1, min_windows=1):
        n = C.c_size_t()
        _check(load_library().dsi_map_count(self._h, int(min_points), int(min_windows), C.byref(n)))
        return n.value

    def extract(self, min_points=1, min_windows=1, sort=True):
        """The cells with at least min_points points, seen in at least min_windows calls: dict of xyz (M, 3) float32
        centroids, n and windows (uint32) and keys (uint64, the packed cell coordinates).  sort=True orders them by
        ascending key on the host (reproducible files); otherwise the order is the table's.  For a PCD file:
        io.save_pcd_ascii(path, np.column_stack([xyz, windows])) writes the window count as the intensity."""
        L = load_library()
        n = C.c_size_t()
        _check(L.dsi_map_count(self._h, int(min_points), int(min_windows), C.byref(n)))
        m = n.value
        out = {"xyz": np.empty((m, 3), np.float32), "n": np.empty(m, np.uint32), "windows": np.empty(m, np.uint32),
               "keys": np.empty(m, np.uint64)}
        _check(L.dsi_map_extract(self._h, int(min_points), int(min_windows), _ptr(out["xyz"], C.c_float), _ptr(out["n"], C.c_uint32),
                                 _ptr(out["windows"], C.c_uint32), _ptr(out["keys"], C.c_uint64), m, C.byref(n)))
        return self._by_key(out) if sort else out

    def info(self):
        """dict of leaf, capacity (slots), occupied (cells), calls, accepted, rejected (points) and growths (doublings)."""
        i = _MapInfo()
        _check(load_library().dsi_map_info(self._h, C.byref(i)))
        return _info_dict(i, ("capacity", "occupied", "calls", "accepted", "rejected", "growths", "leaf"))

    def render(self, T_v_w, width, height, fx, fy, cx, cy, min_depth, max_depth, splat=0, min_points=1, min_windows=1,
               fetch=True):
        """The depth image the map presents to a pinhole camera (dsi_map_render; DESIGN.md 7j "Rendering"): every cell
        that passes extract()'s filter is projected through T_v_w (world -> view, as pose_matrix takes it; invert_pose
        makes it from the camera's pose in the world) and the nearest one per pixel is kept; a cell is drawn on the
        (2 splat + 1)^2 pixels around its own.  Integer pixel coordinates are pixel centres.  Returns the counts n_cells
        (passed the filter) = n_clipped + n_outside + n_drawn, n_pixels (covered), width and height, and with fetch=True
        the images (height, width): depth float32 (0 where empty), windows uint32 (the winner's window count), hits uint32
        (cells drawn on the pixel) and mask uint8.  The images stay on the device for renderImage and
        DepthScore.addMapRender until the map changes."""
        v = _MapView()
        v.width, v.height, v.splat = int(width), int(height), int(splat)
        v.min_points, v.min_windows = int(min_points), int(min_windows)
        v.fx, v.fy, v.cx, v.cy = float(fx), float(fy), float(cx), float(cy)
        v.min_depth, v.max_depth = float(min_depth), float(max_depth)
        v.T_v_w[:] = pose_matrix(T_v_w).tolist()
        i = _MapRenderInfo()
        _check(load_library().dsi_map_render(self._h, C.byref(v), C.byref(i)))
        self._render_shape = (int(i.height), int(i.width))
        out = _info_dict(i)
        if fetch:
            out.update(self.fetchRender())
        return out

    def fetchRender(self):
        """dict of depth, windows, hits and mask of the last render (dsi_map_render_fetch); raises DsiError when the map
        changed since, or was never rendered."""
        shape = self._render_shape
        out = {"depth": np.empty(shape, np.float32), "windows": np.empty(shape, np.uint32), "hits": np.empty(shape, np.uint32),
               "mask": np.empty(shape, np.uint8)}
        _check(load_library().dsi_map_render_fetch(self._h, _ptr(out["depth"], C.c_float), _ptr(out["windows"], C.c_uint32),
                                                   _ptr(out["hits"], C.c_uint32), _ptr(out["mask"], C.c_uint8)))
        return out

    def renderImage(self, min_depth, max_depth, lut=None):
        """The inverse-depth colour image (height, width, 3) uint8, B G R, of the last render: its depth and mask through
        depth_images' encoder (dsi_depth_images without a confidence map)."""
        r = self.fetchRender()
        rows, cols = r["depth"].shape
        lut = _lut_bytes(lut)
        bgr = np.empty((rows, cols, 3), np.uint8)
        _check(load_library().dsi_depth_images(self.ctx._h, _ptr(r["depth"], C.c_float), None, _ptr(r["mask"], C.c_uint8), rows, cols,
                                               C.c_float(min_depth), C.c_float(max_depth),
                                               None if lut is None else _ptr(lut, C.c_uint8), None, _ptr(bgr, C.c_uint8)))
        return bgr

    def integrateDepth(self, depth, mask, K, min_depth, max_depth, T_w_c):
        """One call of a depth image (dsx_map_integrate_depth; DESIGN.md 7j "Scoring the map in 3-D"): depth (height, width)
        float32, mask (the same shape, > 0 keeps a pixel) or None, K = (fx, fy, cx, cy) or a 3 x 3 matrix, T_w_c the camera's
        pose in the world as pose_matrix takes it.  A pixel is integrated iff it is unmasked and its depth is finite and in
        [min_depth, max_depth]; integer pixel coordinates are pixel centres.  Bit for bit integrate() of the back-projected
        float32 points.  Returns (pixels integrated, of those rejected)."""
        depth = _arr(depth, np.float32)
        if depth.ndim != 2:
            raise ValueError("depth must be (height, width)")
        if mask is not None:
            mask = _arr(mask, np.uint8)
            if mask.shape != depth.shape:
                raise ValueError("mask must have the depth image's shape")
        fx, fy, cx, cy = _pinhole(K)
        T = pose_matrix(T_w_c)
        n, rej = C.c_uint64(), C.c_uint64()
        _check(load_library().dsx_map_integrate_depth(self._h, _ptr(depth, C.c_float), None if mask is None else _ptr(mask, C.c_uint8),
                                                      depth.shape[1], depth.shape[0], fx, fy, cx, cy, float(min_depth), float(max_depth),
                                                      _ptr(T, C.c_double), C.byref(n), C.byref(rej)))
        return n.value, rej.value

    def integrateGroundTruth(self, projector, K, min_depth, max_depth, T_w_c):
        """integrateDepth of the depth map a GroundTruthProjector last made, where it lies on the device, at the projector's
        size and without a mask (dsx_map_integrate_depth_gt): only the counts travel."""
        fx, fy, cx, cy = _pinhole(K)
        T = pose_matrix(T_w_c)
        n, rej = C.c_uint64(), C.c_uint64()
        _check(load_library().dsx_map_integrate_depth_gt(self._h, projector._h, fx, fy, cx, cy, float(min_depth), float(max_depth),
                                                         _ptr(T, C.c_double), C.byref(n), C.byref(rej)))
        return n.value, rej.value

    def compare(self, other, radius, n_bins=16, min_points=1, min_windows=1, min_points_other=1, min_windows_other=1,
                distances=False):
        """For every cell of this map (that passes min_points / min_windows) the distance to the nearest centroid of `other`
        (cells passing min_points_other / min_windows_other) within `radius`, looked up in other's table over
        ceil(radius / other's leaf) <= 3 cells per axis (dsx_map_compare; the arithmetic is stated in dsi_map_eval.h).
        Returns hist (uint64 [n_bins], bins of width radius / n_bins), n_cells = n_matched + n_unmatched, sum_q, reach and
        mean (of the matched distances; nan without one); with distances=True also keys and dist (float32, inf where
        unmatched), sorted by key."""
        o = _MapCompareOpts(int(min_points), int(min_windows), int(min_points_other), int(min_windows_other), float(radius), int(n_bins))
        i = _MapCompareInfo()
        hist = np.zeros(max(int(n_bins), 0), np.uint64)
        L = load_library()
        _check(L.dsx_map_compare(self._h, other._h, C.byref(o), _ptr(hist, C.c_uint64) if hist.size else None, C.byref(i)))
        out = _info_dict(i)
        out["hist"] = hist
        out["mean"] = out["sum_q"] * float(radius) / 4294967296.0 / out["n_matched"] if out["n_matched"] else float("nan")
        if distances:
            out.update(self.fetchDistances())
        return out

    _DISTANCE_COLUMNS = (_Column("dist", _F32), _Column("keys", _U64))  # (dsx_map_compare_fetch takes the values first)

    def fetchDistances(self, sort=True):
        """keys (uint64) and dist (float32) of the last compare() of this map (dsx_map_compare_fetch); raises DsiError when
        the map changed since, or was never compared."""
        return self._fetch_rows(load_library().dsx_map_compare_fetch, self._DISTANCE_COLUMNS, sort)

    def prune(self, min_points=1, min_windows=1, max_age=None, box=None, reach=0, min_neighbors=0, shrink=False):
        """Removes cells and rebuilds the table around the rest (dsx_map_prune; the rule is stated in dsi_map_prune.h and
        DESIGN.md 7j "Pruning").  A cell leaves by the first criterion that fails: fewer than min_points points; seen in
        fewer than min_windows calls; max_age (None: off) -- more than max_age integrate calls since the last one that
        reached it, empty calls included; box = (lo, hi), three numbers each (None: off) -- its extracted centroid outside
        the closed box; reach 1 or 2 (0: off) -- fewer than min_neighbors other cells that survive the first four within
        reach cells per axis.  The defaults remove nothing.  shrink=True: the table becomes the smallest that holds the
        kept cells at 3/4 load (at least 2**8 slots).  Returns dict of n_cells = n_kept + sum(n_removed), n_kept,
        n_removed (five counts, by criterion) and capacity (slots afterwards).  Render, compare and classification of the
        map are invalid afterwards."""
        return self._prune(load_library().dsx_map_prune, min_points, min_windows, max_age, box, reach, min_neighbors, shrink)

    def classifyPrune(self, min_points=1, min_windows=1, max_age=None, box=None, reach=0, min_neighbors=0, shrink=False):
        """prune()'s dry run (dsx_map_prune_classify): the same counts, the map unchanged and its render and compare still
        valid; the per-cell verdicts stay on the device for fetchPruneReasons until the map changes."""
        return self._prune(load_library().dsx_map_prune_classify, min_points, min_windows, max_age, box, reach, min_neighbors, shrink)

    def _prune(self, fn, min_points, min_windows, max_age, box, reach, min_neighbors, shrink):
        if max_age is not None and int(max_age) < 0:
            raise ValueError("max_age is None or >= 0")
        o = _MapPruneOpts()
        o.min_points, o.min_windows = int(min_points), int(min_windows)
        o.max_age = -1 if max_age is None else int(max_age)
        o.use_box = 0 if box is None else 1
        if box is not None:
            lo, hi = (np.asarray(b, np.float64).reshape(3) for b in box)
            o.box_lo[:], o.box_hi[:] = lo.tolist(), hi.tolist()
        o.reach, o.min_neighbors, o.shrink = int(reach), int(min_neighbors), 1 if shrink else 0
        i = _MapPruneInfo()
        _check(fn(self._h, C.byref(o), C.byref(i)))
        return _info_dict(i)

    _PRUNE_COLUMNS = (_Column("reason", _U8), _Column("keys", _U64))  # (dsx_map_prune_fetch takes the values first)

    def fetchPruneReasons(self, sort=True):
        """keys (uint64) and reason (uint8: 0 kept, 1..5 the first criterion that failed) of every cell, from the last
        classifyPrune() of this map (dsx_map_prune_fetch); raises DsiError when the map changed since, or was never
        classified.  sort=True orders them by ascending key; otherwise the order is extract(sort=False)'s."""
        return self._fetch_rows(load_library().dsx_map_prune_fetch, self._PRUNE_COLUMNS, sort)

    def components(self, min_points=1, min_windows=1, connectivity=26):
        """Labels the map's connected components (dsx_map_components; the rule is stated in dsi_map_components.h and
        DESIGN.md 7j "Components").  The nodes are the cells extract(min_points, min_windows) returns; two are adjacent
        when their cell indices differ by an offset of the connectivity: 6 (faces), 18 (and edges), 26 (and corners) or
        124 (the 5 x 5 x 5 box).  A component's label is the smallest key among its cells.  Returns dict of n_cells
        (nodes), n_unlabelled, n_components, n_singletons, largest_label, largest_cells, largest_points (the largest by
        cells, then by the smaller label).  The labelling stays on the device for fetchComponents, listComponents,
        selectComponents and pruneComponents until the map changes; nothing else of the map changes."""
        o = _MapComponentsOpts(int(min_points), int(min_windows), int(connectivity))
        i = _MapComponentsInfo()
        _check(load_library().dsx_map_components(self._h, C.byref(o), C.byref(i)))
        self._components_selected = False
        return _info_dict(i)

    _COMPONENT_COLUMNS = (_Column("keys", _U64), _Column("labels", _U64), _Column("reason", _U8, flag="_components_selected"))

    def fetchComponents(self, sort=True):
        """keys and labels (uint64) of every node of the last components() of this map and, after a selectComponents() on
        it, reason (uint8: 0 kept, 1..4 the first reason of the selection that holds) (dsx_map_components_fetch); raises
        DsiError when the map changed since.  sort=True orders them by ascending key; otherwise the order is
        extract(sort=False)'s under the labelling's filter."""
        return self._fetch_rows(load_library().dsx_map_components_fetch, self._COMPONENT_COLUMNS, sort)

    _COMPONENT_LIST_COLUMNS = (_Column("labels", _U64), _Column("cells", _U64), _Column("points", _U64))

    def listComponents(self):
        """labels, cells and points (uint64) of every component of the last components() of this map
        (dsx_map_components_list), by cells descending, then label ascending; raises DsiError when the map changed since."""
        out = self._fetch_rows(load_library().dsx_map_components_list, self._COMPONENT_LIST_COLUMNS, sort=False)
        order = np.lexsort((out["labels"], -out["cells"].astype(np.int64)))
        return {k: v[order] for k, v in out.items()}

    def selectComponents(self, min_cells=1, min_component_points=1, keep_largest=0, shrink=False):
        """pruneComponents()'s dry run (dsx_map_components_select): the same counts, the map unchanged; the per-cell reasons
        stay on the device for fetchComponents until the map changes."""
        return self._select(load_library().dsx_map_components_select,
                            _MapComponentsSelection(int(min_cells), int(min_component_points), int(keep_largest), 1 if shrink else 0),
                            _MapComponentsSelectInfo(), "_components_selected")

    def pruneComponents(self, min_cells=1, min_component_points=1, keep_largest=0, shrink=False):
        """Removes cells by the last components() of this map and rebuilds the table around the rest
        (dsx_map_prune_components).  A cell leaves by the first reason that holds: it is unlabelled; its component has fewer
        than min_cells cells; fewer than min_component_points points; keep_largest (1..16; 0: off) -- its component is not
        among the keep_largest first of those left, by cells descending, then label ascending.  shrink as prune()'s.
        Returns dict of n_cells = n_kept + sum(n_removed), n_kept, n_removed (four counts, by reason), n_components_kept
        and capacity (slots afterwards).  Render, compare, alignment, classification and labelling are invalid afterwards."""
        return self._select(load_library().dsx_map_prune_components,
                            _MapComponentsSelection(int(min_cells), int(min_component_points), int(keep_largest), 1 if shrink else 0),
                            _MapComponentsSelectInfo(), "_components_selected")

    def query(self, points, k, radius, min_points=1, min_windows=1):
        """The k nearest cells of every point (dsx_map_knn_points; the rule is stated in dsi_map_knn.h and DESIGN.md 7j
        "Neighbours and statistical outliers"): points (N, 3) or (N, 4) float32, x y z first; the candidates are the cells
        extract(min_points, min_windows) returns, within radius (at most three leaves) of the point, ordered by distance,
        then by key.  Returns dict of keys (N, k) uint64 padded with 0, dist (N, k) float32 padded with +inf and found
        (N,) uint8.  A non-finite point has found 0.  Reads the map only."""
        pts = _arr(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] not in (3, 4):
            raise ValueError("points must be (N, 3) or (N, 4)")
        o = _MapKnnOpts(int(min_points), int(min_windows), int(k), 1, float(radius))
        n, kk = pts.shape[0], max(int(k), 0)
        out = {"keys": np.zeros((n, kk), np.uint64), "dist": np.full((n, kk), np.inf, np.float32), "found": np.zeros(n, np.uint8)}
        _check(load_library().dsx_map_knn_points(self._h, _ptr(pts, C.c_float), pts.shape[1], n, C.byref(o), _ptr(out["keys"], C.c_uint64),
                                                 _ptr(out["dist"], C.c_float), _ptr(out["found"], C.c_uint8)))
        return out

    def knn(self, k, radius, min_found=1, min_points=1, min_windows=1):
        """The self query (dsx_map_knn): every cell extract(min_points, min_windows) returns asks for its k nearest other
        cells within radius, from its own centroid; per cell found, the mean distance m and q = floor(m / radius * 2**30)
        stay on the device for fetchKnn, selectOutliers and pruneOutliers until the map changes.  A cell is scored when
        found >= min_found.  Returns dict of n_cells, n_unqueried, n_scored, n_isolated, sum_q, sum_q2 (a Python int, the
        exact sum of q * q over the scored cells) and reach.  Nothing else of the map changes."""
        o = _MapKnnOpts(int(min_points), int(min_windows), int(k), int(min_found), float(radius))
        i = _MapKnnInfo()
        _check(load_library().dsx_map_knn(self._h, C.byref(o), C.byref(i)))
        self._knn_selected = False
        out = _info_dict(i, ("n_cells", "n_unqueried", "n_scored", "n_isolated", "sum_q", "reach"))
        out["sum_q2"] = int(i.sum_q2[0]) | (int(i.sum_q2[1]) << 64)
        return out

    _KNN_COLUMNS = (_Column("keys", _U64), _Column("found", _U8), _Column("mean", _F32), _Column("q", _U32),
                    _Column("reason", _U8, flag="_knn_selected"))

    def fetchKnn(self, sort=True):
        """keys (uint64), found (uint8), mean (float32, +inf where found is 0) and q (uint32) of every query of the last
        knn() of this map and, after a selectOutliers() on it, reason (uint8: 0 kept, 1..3 the first reason that holds)
        (dsx_map_knn_fetch); raises DsiError when the map changed since.  sort=True orders them by ascending key; otherwise
        the order is extract(sort=False)'s under the query's filter."""
        return self._fetch_rows(load_library().dsx_map_knn_fetch, self._KNN_COLUMNS, sort)

    def selectOutliers(self, std_mult=1.0, shrink=False):
        """pruneOutliers()'s dry run (dsx_map_knn_select): the same counts, the map unchanged; the per-cell reasons stay on
        the device for fetchKnn until the map changes."""
        return self._select(load_library().dsx_map_knn_select, _MapKnnSelection(float(std_mult), 1 if shrink else 0), _MapKnnSelectInfo(),
                            "_knn_selected")

    def pruneOutliers(self, std_mult=1.0, shrink=False):
        """PCL's StatisticalOutlierRemoval on the last knn() of this map (dsx_map_prune_knn): a cell leaves by the first
        reason that holds -- it fails the query's filter; it is isolated (found < min_found); std_mult >= 0 and its q lies
        above T_q = floor(mu + std_mult * sigma), mu and sigma the mean and the sample deviation of q over the scored cells
        (knn_threshold) -- and the table is rebuilt around the rest, shrink as prune()'s.  Returns dict of n_cells = n_kept +
        sum(n_removed), n_kept, n_removed (three counts, by reason), T_q, mu, sigma and capacity (slots afterwards).
        Render, compare, alignment, classification, labelling and self query are invalid afterwards."""
        return self._select(load_library().dsx_map_prune_knn, _MapKnnSelection(float(std_mult), 1 if shrink else 0), _MapKnnSelectInfo(),
                            "_knn_selected")

    def pca(self, k, radius, min_found=2, orient=False, viewpoint=None, keep_moments=False, min_points=1, min_windows=1):
        """The local shape of every cell extract(min_points, min_windows) returns (dsx_map_pca; the rule is stated in
        dsi_map_pca.h and DESIGN.md 7j "Local shape"): the principal components of the cell and its neighbours within
        radius (at most three leaves) -- all of them for k = 0, the k nearest for k in 1..16 --, from exact integer moments.
        Per cell a normal, a tangent, three eigenvalues, the number of members, a label (0 sparse: fewer than min_found
        neighbours; 1 linear, 2 planar, 3 scattered) and flags (bit 0: the normal is determined, bit 1: the tangent) stay on
        the device for fetchPca, selectShapes and pruneShapes until the map changes.  orient=True turns every normal towards
        viewpoint (three finite numbers); keep_moments=True keeps the nine integers per cell for fetchPca.  Returns dict of
        n_cells, n_unqueried, n_sparse, n_label (linear, planar, scattered), n_normal_determined, n_tangent_determined,
        sum_members and reach.  Nothing else of the map changes."""
        vp = (0.0, 0.0, 0.0) if viewpoint is None else tuple(float(v) for v in viewpoint)
        if len(vp) != 3:
            raise ValueError("viewpoint must be three numbers")
        if orient and viewpoint is None:
            raise ValueError("orient needs a viewpoint")
        o = _MapPcaOpts(int(min_points), int(min_windows), int(k), int(min_found), float(radius), 1 if orient else 0,
                        1 if keep_moments else 0, (C.c_double * 3)(*vp))
        i = _MapPcaInfo()
        self._pca_selected = False
        self._pca_moments = False
        _check(load_library().dsx_map_pca(self._h, C.byref(o), C.byref(i)))
        self._pca_moments = bool(keep_moments)
        return _info_dict(i, ("n_cells", "n_unqueried", "n_sparse", "n_normal_determined", "n_tangent_determined", "sum_members", "reach",
                              "n_label"))

    _PCA_COLUMNS = (_Column("keys", _U64), _Column("normal", _F32, (3,)), _Column("tangent", _F32, (3,)), _Column("eval", _F32, (3,)),
                    _Column("members", _U16), _Column("label", _U8), _Column("flags", _U8), _Column("moments", _I64, (9,), flag="_pca_moments"),
                    _Column("reason", _U8, flag="_pca_selected"))

    def fetchPca(self, sort=False):
        """keys (uint64), normal, tangent and eval ((M, 3) float32), members (uint16), label and flags (uint8) of every query
        of the last pca() of this map, moments ((M, 9) int64: s[3], ss[6]) when it kept them and, after a selectShapes() on
        it, reason (uint8: 0 kept, 1..3 the first reason that holds) (dsx_map_pca_fetch); raises DsiError when the map
        changed since.  The order is extract(sort=False)'s under the pass's filter; sort=True orders by ascending key."""
        return self._fetch_rows(load_library().dsx_map_pca_fetch, self._PCA_COLUMNS, sort)

    def selectShapes(self, keep=("linear", "planar"), remove_sparse=True, shrink=False):
        """pruneShapes()'s dry run (dsx_map_pca_select): the same counts, the map unchanged; the per-cell reasons stay on the
        device for fetchPca until the map changes."""
        return self._select(load_library().dsx_map_pca_select,
                            _MapPcaSelection(shape_mask(keep), 1 if remove_sparse else 0, 1 if shrink else 0), _MapPcaSelectInfo(),
                            "_pca_selected")

    def pruneShapes(self, keep=("linear", "planar"), remove_sparse=True, shrink=False):
        """Keeps the cells of the last pca() of this map whose label is in keep -- names out of "linear", "planar" and
        "scattered", or the mask itself (1, 2, 4) -- (dsx_map_prune_pca): a cell leaves by the first reason that holds -- it
        fails the pass's filter; it is sparse and remove_sparse; its label is not kept -- and the table is rebuilt around the
        rest, shrink as prune()'s.  Returns dict of n_cells = n_kept + sum(n_removed), n_kept, n_removed (three counts, by
        reason) and capacity (slots afterwards).  Everything derived from the map is invalid afterwards."""
        return self._select(load_library().dsx_map_prune_pca,
                            _MapPcaSelection(shape_mask(keep), 1 if remove_sparse else 0, 1 if shrink else 0), _MapPcaSelectInfo(),
                            "_pca_selected")

    @staticmethod
    def _observation(width, height, K, min_depth, max_depth, T_v_w, window, abs_tol, rel_tol):
        o = _MapObservation()
        o.width, o.height, o.window = int(width), int(height), int(window)
        o.fx, o.fy, o.cx, o.cy = _pinhole(K)
        o.min_depth, o.max_depth = float(min_depth), float(max_depth)
        o.abs_tol, o.rel_tol = float(abs_tol), float(rel_tol)
        o.T_v_w[:] = pose_matrix(T_v_w).tolist()
        return o

    def observe(self, depth, mask, K, min_depth, max_depth, T_v_w, window=1, abs_tol=0.0, rel_tol=0.0):
        """What one depth image says about every cell (dsx_map_observe; the rule is stated in dsi_map_visibility.h and
        DESIGN.md 7j "Visibility"): depth (height, width) float32, mask (the same shape, > 0 keeps a pixel) or None,
        K = (fx, fy, cx, cy) or a 3 x 3 matrix, T_v_w world -> view as render() takes it.  A cell is projected as render()
        projects it and judged by the valid pixels -- unmasked, finite, in [min_depth, max_depth] -- among the
        (2 window + 1)^2 around its own, against its depth Z with tol = rel_tol * Z + abs_tol: the view AGREES when any of
        them lies within Z +- tol, looks THROUGH the cell when every one lies beyond Z + tol, and otherwise sees a surface
        in front (BEHIND).  The verdicts accumulate per cell over the observations until the map changes or
        clearVisibility(), for fetchVisibility, selectCarved and pruneCarved.  Returns this view's counts: n_cells =
        n_clipped + n_outside + n_unseen + n_agree + n_through + n_behind, n_valid_pixels and views (observations in the
        tally).  Nothing else of the map changes."""
        depth = _arr(depth, np.float32)
        if depth.ndim != 2:
            raise ValueError("depth must be (height, width)")
        if mask is not None:
            mask = _arr(mask, np.uint8)
            if mask.shape != depth.shape:
                raise ValueError("mask must have the depth image's shape")
        o = self._observation(depth.shape[1], depth.shape[0], K, min_depth, max_depth, T_v_w, window, abs_tol, rel_tol)
        i = _MapObserveInfo()
        self._visibility_selected = False
        _check(load_library().dsx_map_observe(self._h, _ptr(depth, C.c_float), None if mask is None else _ptr(mask, C.c_uint8), C.byref(o),
                                              C.byref(i)))
        return _info_dict(i)

    def observeMapper(self, mapper, K, min_depth, max_depth, T_v_w, window=1, abs_tol=0.0, rel_tol=0.0):
        """observe() of the filtered depth map and mask the mapper's last getDepthMapFromDSI(..., options_depth_map) /
        filterDepthMap left on the device, read where they lie (dsx_map_observe_mapper): only the counts travel.  The
        mapper must live on the map's context."""
        o = self._observation(mapper.dimX, mapper.dimY, K, min_depth, max_depth, T_v_w, window, abs_tol, rel_tol)
        i = _MapObserveInfo()
        self._visibility_selected = False
        _check(load_library().dsx_map_observe_mapper(self._h, mapper._h, C.byref(o), C.byref(i)))
        return _info_dict(i)

    def clearVisibility(self):
        """Zeroes the tally (dsx_map_visibility_clear): the next observe() is the first."""
        self._visibility_selected = False
        _check(load_library().dsx_map_visibility_clear(self._h))

    _VISIBILITY_COLUMNS = (_Column("keys", _U64), _Column("seen", _U32), _Column("agree", _U32), _Column("through", _U32),
                           _Column("reason", _U8, flag="_visibility_selected"))

    def fetchVisibility(self, sort=True):
        """keys (uint64), seen, agree and through (uint32: the views with a verdict on the cell, and those that agreed and
        looked through; behind = seen - agree - through) of every cell and, after a selectCarved() on this tally, reason
        (uint8: 1 carved, 0 kept) (dsx_map_visibility_fetch); raises DsiError without an observe() since the map last
        changed.  sort=True orders by ascending key; otherwise the order is extract(sort=False)'s."""
        return self._fetch_rows(load_library().dsx_map_visibility_fetch, self._VISIBILITY_COLUMNS, sort)

    def selectCarved(self, min_through=2, agree_weight=1, shrink=False):
        """pruneCarved()'s dry run (dsx_map_visibility_select): the same counts, the map unchanged; the per-cell reasons stay
        on the device for fetchVisibility until the next observe()."""
        return self._select(load_library().dsx_map_visibility_select,
                            _MapVisibilitySelection(int(min_through), int(agree_weight), 1 if shrink else 0), _MapVisibilitySelectInfo(),
                            "_visibility_selected")

    def pruneCarved(self, min_through=2, agree_weight=1, shrink=False):
        """Removes the cells that the observed views carve away (dsx_map_prune_visibility): those with through >= min_through
        and through > agree_weight * agree; the table is rebuilt around the rest, shrink as prune()'s.  Returns dict of
        n_cells = n_kept + n_removed, n_kept, n_removed and capacity (slots afterwards).  Everything derived from the map
        is invalid afterwards, the tally included."""
        return self._select(load_library().dsx_map_prune_visibility,
                            _MapVisibilitySelection(int(min_through), int(agree_weight), 1 if shrink else 0), _MapVisibilitySelectInfo(),
                            "_visibility_selected")

    _STATE_COLUMNS = (_Column("keys", _U64), _Column("n", _U32), _Column("S", _U64, (3,)), _Column("windows", _U32), _Column("stamp", _U32))

    def exportState(self, sort=True):
        """The map's exact state (dsx_map_export; the rule is stated in dsi_map_merge.h and DESIGN.md 7j "Merging"): dict
        of leaf, calls, accepted, rejected and, per cell, keys (uint64), n (uint32), S (uint64, (M, 3): the sums of the
        32-bit cell fractions), windows and stamp (uint32).  sort=True orders the cells by ascending key; otherwise the
        order is extract(sort=False)'s.  importState() of it into an empty map restores the map bit for bit, ages
        included; io.save_world_map writes it to a file.  Changes nothing: render, compare and classification stay."""
        st = _MapState()
        cells = self._fetch_rows(load_library().dsx_map_export, self._STATE_COLUMNS, sort, lead=(C.byref(st),))
        return dict(_info_dict(st, ("leaf", "calls", "accepted", "rejected")), **cells)

    def importState(self, state):
        """Appends an exported state to this map (dsx_map_import), exactly as merge() appends the map it came from: into
        an empty map with no calls it restores that map.  state: exportState()'s dict (any cell order); the arrays are
        validated on the device and a state that no map could have produced is refused, this map unchanged.  Returns
        dict of n_src_cells = n_new + n_common, capacity (slots afterwards) and growths (doublings made by this call)."""
        keys = np.ascontiguousarray(state["keys"], np.uint64).reshape(-1)
        m = keys.shape[0]
        n, w, s = (np.ascontiguousarray(state[k], np.uint32).reshape(-1) for k in ("n", "windows", "stamp"))
        S = np.ascontiguousarray(state["S"], np.uint64).reshape(-1)
        if not (n.shape[0] == w.shape[0] == s.shape[0] == m and S.shape[0] == 3 * m):
            raise ValueError("keys, n, windows and stamp need one entry per cell and S three")
        st = _MapState(float(state["leaf"]), m, int(state["calls"]), int(state["accepted"]), int(state["rejected"]))
        i = _MapMergeInfo()
        _check(load_library().dsx_map_import(self._h, C.byref(st), _ptr(keys, C.c_uint64), _ptr(n, C.c_uint32), _ptr(S, C.c_uint64),
                                             _ptr(w, C.c_uint32), _ptr(s, C.c_uint32), C.byref(i)))
        return _info_dict(i)

    def merge(self, other):
        """Appends `other` (a WorldMap on the same context and of the same leaf) to this map on the device
        (dsx_map_merge): afterwards this map is, bit for bit, the map that had made its own integrate calls and then
        other's -- n, S and windows add up, other's stamps move behind this map's calls.  other is unchanged; this map's
        render, compare and classification are invalid afterwards.  Maps of different contexts:
        process.merge_world_maps.  Returns importState()'s dict."""
        i = _MapMergeInfo()
        _check(load_library().dsx_map_merge(self._h, other._h, C.byref(i)))
        return _info_dict(i)

    @staticmethod
    def _align_opts(radius, min_points, min_windows, min_points_other, min_windows_other, max_iterations=1, min_matched=0,
                    eps_rot=0.0, eps_trans=0.0):
        return _MapAlignOpts(int(min_points), int(min_windows), int(min_points_other), int(min_windows_other), float(radius),
                             int(max_iterations), 0, int(min_matched), float(eps_rot), float(eps_trans))

    def alignStep(self, other, radius, T=None, min_points=1, min_windows=1, min_points_other=1, min_windows_other=1,
                  correspondences=False):
        """One correspondence pass of ICP (dsx_map_align_step; the arithmetic is stated in dsi_map_align.h and DESIGN.md 7j
        "Aligning"): every filtered cell of this map, moved by T (this map's frame in other's, as pose_matrix takes it; None:
        the identity), is paired with the nearest filtered centroid of `other` within `radius`, ties to the smaller key.
        Returns the exact integer moments of the matched pairs as Python ints -- n_cells = n_matched + n_unmatched, su, sv
        (3), suv_hi, suv_lo (9, row-major: sum U[r] V[c] = suv_hi * 2**32 + suv_lo), e2 -- with quantum and reach: what
        solve_alignment takes.  correspondences=True adds fetchAlignment()'s arrays."""
        o = self._align_opts(radius, min_points, min_windows, min_points_other, min_windows_other)
        T = pose_matrix(np.eye(4)[:3] if T is None else T)
        m = _MapAlignMoments()
        _check(load_library().dsx_map_align_step(self._h, other._h, C.byref(o), _ptr(T, C.c_double), C.byref(m)))
        out = _moments_dict(m)
        if correspondences:
            out.update(self.fetchAlignment())
        return out

    _ALIGNMENT_COLUMNS = (_Column("keys", _U64), _Column("keys_other", _U64), _Column("dist", _F32))

    def fetchAlignment(self, sort=True):
        """keys (uint64, this map's), keys_other (uint64, the correspondence's key in the other map; 0 where unmatched) and
        dist (float32, inf where unmatched) of the last alignStep() or align() of this map (dsx_map_align_fetch); raises
        DsiError when the map changed since, or was never aligned.  sort=True orders them by ascending key."""
        return self._fetch_rows(load_library().dsx_map_align_fetch, self._ALIGNMENT_COLUMNS, sort)

    def align(self, other, radius, T_init=None, max_iterations=20, min_matched=3, eps_rot=1e-6, eps_trans=None, min_points=1,
              min_windows=1, min_points_other=1, min_windows_other=1):
        """ICP of this map onto `other` (dsx_map_align): up to max_iterations rounds of alignStep, solve_alignment and
        T <- compose_pose(T_delta, T), from T_init (None: the identity), until a round's T_delta turns by at most eps_rot
        radians and moves by at most eps_trans (None: 1e-4 of other's leaf).  Returns (T, info): T the 12 doubles of this
        map's frame in other's, info a dict of iterations, converged, stopped, reach, n_cells, n_matched_first / _last,
        rms_first / _last, angle_last and trans_last.  A round that matches fewer than min_matched cells, or whose pairs do
        not determine a rotation, raises DsiError; the exception's `T` and `info` hold the last good pose."""
        if eps_trans is None:
            eps_trans = 1e-4 * other.info()["leaf"]
        o = self._align_opts(radius, min_points, min_windows, min_points_other, min_windows_other, max_iterations, min_matched,
                             eps_rot, eps_trans)
        T0 = pose_matrix(np.eye(4)[:3] if T_init is None else T_init)
        T = np.empty(12, np.float64)
        i = _MapAlignInfo()
        rc = load_library().dsx_map_align(self._h, other._h, C.byref(o), _ptr(T0, C.c_double), _ptr(T, C.c_double), C.byref(i))
        info = _info_dict(i)
        if rc != OK:
            try:
                _check(rc)
            except DsiError as e:
                if i.stopped:
                    e.T, e.info = T, info
                raise
        return T, info

    def integrateMap(self, other, T=None, min_points=1, min_windows=1):
        """One integrate call of `other`'s cells that pass min_points / min_windows, each as its float32 centroid, under
        the pose T (other's frame in this map's; None: the identity), on the device (dsx_map_integrate_map): bit for bit
        integrate(other.extract(min_points, min_windows)["xyz"], T).  The leaves may differ; other must be another map on
        the same context.  Returns (cells integrated, of those rejected)."""
        T = pose_matrix(np.eye(4)[:3] if T is None else T)
        n, rej = C.c_uint64(), C.c_uint64()
        _check(load_library().dsx_map_integrate_map(self._h, other._h, _ptr(T, C.c_double), int(min_points), int(min_windows),
                                                    C.byref(n), C.byref(rej)))
        return n.value, rej.value

    def reset(self):
        _check(load_library().dsi_map_reset(self._h))

    def close(self):
        if self._h:
            load_library().dsi_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)


def _pinhole(K):
    """(fx, fy, cx, cy) as floats from those four numbers or from a 3 x 3 camera matrix"""
    K = np.asarray(K, np.float64)
    if K.shape == (3, 3):
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if K.size != 4:
        raise ValueError("K is (fx, fy, cx, cy) or a 3 x 3 matrix")
    return tuple(float(v) for v in K.reshape(4))


MOMENT_COUNTS = ("n_cells", "n_matched", "n_unmatched", "e2", "reach")
MOMENT_SUMS = ("su", "sv", "suv_hi", "suv_lo")


def _moments_dict(m):
    out = {k: int(getattr(m, k)) for k in MOMENT_COUNTS}
    out.update({k: [int(v) for v in getattr(m, k)] for k in MOMENT_SUMS})
    out["quantum"] = float(m.quantum)
    return out


def _moments_struct(moments):
    m = _MapAlignMoments()
    for k in ("n_cells", "n_matched", "n_unmatched", "e2"):
        setattr(m, k, int(moments[k]))
    for k in MOMENT_SUMS:
        getattr(m, k)[:] = [int(v) for v in moments[k]]
    m.quantum = float(moments["quantum"])
    m.reach = int(moments.get("reach", 0))
    return m


def compose_pose(A, B):
    """A o B of two rigid poses as pose_matrix takes them (dsx_pose_compose, the routine dsi::compose_pose calls too):
    R = A_R B_R, t = A_R B_t + A_t, 12 doubles, every dot product ((a0 b0 + a1 b1) + a2 b2) in double without FMA."""
    A, B = pose_matrix(A), pose_matrix(B)
    out = np.empty(12, np.float64)
    _check(load_library().dsx_pose_compose(_ptr(A, C.c_double), _ptr(B, C.c_double), _ptr(out, C.c_double)))
    return out


def solve_alignment(moments):
    """The rigid motion that carries the matched cells onto their correspondences in the least-squares sense, from
    WorldMap.alignStep's moments alone (dsx_map_align_solve: Horn's quaternion form, a 4 x 4 Jacobi eigen-solve; stated
    in dsi_map_align.h; no device is touched).  Returns (T_delta, info): 12 doubles and a dict of n_matched, rms (of the
    pairs as matched), angle (radians) and trans of T_delta and the two largest eigenvalues `lambda`.  Raises DsiError
    for fewer than 3 pairs and for pairs that do not determine a rotation (collinear or coincident)."""
    m = _moments_struct(moments)
    T = np.empty(12, np.float64)
    i = _MapAlignSolveInfo()
    _check(load_library().dsx_map_align_solve(C.byref(m), _ptr(T, C.c_double), C.byref(i)))
    return T, {"n_matched": int(i.n_matched), "rms": float(i.rms), "angle": float(i.angle), "trans": float(i.trans),
               "lambda": [float(v) for v in i.lambda_]}


def knn_threshold(n_scored, sum_q, sum_q2, std_mult):
    """The outlier threshold from WorldMap.knn's moments alone (dsx_map_knn_threshold, the routine dsi::knn_threshold and
    the selection call too; stated in dsi_map_knn.h; no device is touched): V = N sum_q2 - sum_q**2 exactly, mu = sum_q / N,
    sigma = sqrt(V / (N (N - 1))), T_q = floor(mu + std_mult * sigma) clamped to [0, 2**30]; N = 0 gives 2**30.  sum_q2 is
    a Python int below 2**128.  Returns dict of mu, sigma and T_q."""
    s2 = int(sum_q2)
    if not 0 <= s2 < 1 << 128:
        raise ValueError("sum_q2 must be in 0..2**128 - 1")
    words = (C.c_uint64 * 2)(s2 & 0xffffffffffffffff, s2 >> 64)
    mu, sigma, tq = C.c_double(), C.c_double(), C.c_uint64()
    _check(load_library().dsx_map_knn_threshold(int(n_scored), int(sum_q), words, float(std_mult), C.byref(mu), C.byref(sigma),
                                                C.byref(tq)))
    return {"mu": mu.value, "sigma": sigma.value, "T_q": int(tq.value)}


SHAPE_LABELS = {"linear": 1, "planar": 2, "scattered": 4}


def shape_mask(keep):
    """keep_labels of dsi_map_pca.h from names ("linear", "planar", "scattered") or from the mask itself"""
    if isinstance(keep, str):
        keep = (keep,)
    if isinstance(keep, (int, np.integer)):
        return int(keep) & 0xffffffff
    mask = 0
    for name in keep:
        if name not in SHAPE_LABELS:
            raise ValueError("unknown shape %r: linear, planar or scattered" % (name,))
        mask |= SHAPE_LABELS[name]
    return mask


def pca_solve(m, s, ss, quantum, orient=False, viewpoint=None, p=None):
    """One cell's local shape from its integer moments alone (dsx_pca_solve, the routine the pass runs per cell; stated in
    dsi_map_pca.h; no device is touched): m members, s the three sums and ss the six sums of products of the quantised
    offsets, quantum = leaf / 1024; orient=True needs viewpoint and the cell's centroid p.  Returns dict of normal, tangent
    and eval (float32 [3], the row's bits), label, flags, and the doubles normal_d, tangent_d and lambda (ascending)."""
    sv = (C.c_int64 * 3)(*[int(v) for v in s])
    ssv = (C.c_int64 * 6)(*[int(v) for v in ss])
    vp = None if viewpoint is None else (C.c_double * 3)(*[float(v) for v in viewpoint])
    pp = None if p is None else (C.c_double * 3)(*[float(v) for v in p])
    r = _PcaRow()
    _check(load_library().dsx_pca_solve(int(m), sv, ssv, float(quantum), 1 if orient else 0, vp, pp, C.byref(r)))
    return {"normal": np.array(r.normal[:], np.float32), "tangent": np.array(r.tangent[:], np.float32),
            "eval": np.array(r.eval[:], np.float32), "label": int(r.label), "flags": int(r.flags),
            "normal_d": np.array(r.normal_d[:]), "tangent_d": np.array(r.tangent_d[:]), "lambda": np.array(r.lambda_[:])}


def map_f_score(est, gt, radius, n_bins=16, min_points=1, min_windows=1, min_points_gt=1, min_windows_gt=1):
    """3-D accuracy, completeness and F-score of the map `est` against the map `gt` (two WorldMap.compare runs, one per
    direction; the curves of the reference's scripts/precision_completeness.py:44,60,76 taken in space): thresholds
    (i + 1) * radius / n_bins, precision = 100 cumsum(hist_est) / n_cells_est, recall = 100 cumsum(hist_gt) / n_cells_gt,
    f1 = 2 P R / (P + R) (0 where P + R == 0) -- float64 from the integer counts -- plus the two compare dicts."""
    fwd = est.compare(gt, radius, n_bins, min_points, min_windows, min_points_gt, min_windows_gt)
    bwd = gt.compare(est, radius, n_bins, min_points_gt, min_windows_gt, min_points, min_windows)
    n_bins = int(n_bins)
    thresholds = (np.arange(n_bins, dtype=np.float64) + 1.0) * (np.float64(radius) / np.float64(n_bins))
    zero = np.zeros(n_bins, np.float64)
    P = 100.0 * np.cumsum(fwd["hist"]).astype(np.float64) / np.float64(fwd["n_cells"]) if fwd["n_cells"] else zero
    R = 100.0 * np.cumsum(bwd["hist"]).astype(np.float64) / np.float64(bwd["n_cells"]) if bwd["n_cells"] else zero
    some = P + R > 0
    f1 = np.where(some, 2.0 * P * R / np.where(some, P + R, 1.0), 0.0)
    return {"thresholds": thresholds, "precision": P, "recall": R, "f1": f1, "est": fwd, "gt": bwd}


def _polarity_bytes(polarity, n, use_polarity):
    if polarity is None:
        if use_polarity:
            raise ValueError("use_polarity needs the events' polarities")
        return None
    polarity = np.ascontiguousarray(np.asarray(polarity) != 0, np.uint8)
    if polarity.shape != (n,):
        raise ValueError("one polarity per event")
    return polarity


def accumulate_events(ctx, x, y, polarity, width, height, use_polarity=True, return_dropped=False):
    """accumulateEvents(events, use_polarity, img) (utils.cpp:184-216) on the device (dsi_event_image): the uint8
    [height][width] event image of the events x, y (uint16) with polarity (non-zero / True = positive; None is legal
    with use_polarity=False).  width x height is the sensor's size.  use_polarity: 128 = no events, the largest
    |#positive - #negative| maps to 0 / 255; otherwise the count modulo 256, min-max normalised.  Events outside the
    sensor are dropped; return_dropped=True returns (image, number dropped)."""
    x, y = _arr(x, np.uint16), _arr(y, np.uint16)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D arrays of one length")
    pol = _polarity_bytes(polarity, x.shape[0], use_polarity)
    out = np.empty((max(int(height), 0), max(int(width), 0)), np.uint8)
    dropped = C.c_size_t()
    _check(load_library().dsi_event_image(ctx._h, _ptr(x, C.c_uint16), _ptr(y, C.c_uint16),
                                          None if pol is None else _ptr(pol, C.c_uint8), x.shape[0], int(width), int(height),
                                          int(bool(use_polarity)), _ptr(out, C.c_uint8), C.byref(dropped)))
    return (out, dropped.value) if return_dropped else out


def default_jet_lut():
    """The engine's default colour table of depth_images: uint8 [256][3], B G R -- a piecewise-linear jet, not OpenCV's
    COLORMAP_JET table (pass cv2.applyColorMap of a 0..255 ramp as `lut` for that)."""
    lut = np.empty((256, 3), np.uint8)
    _check(load_library().dsi_default_jet_lut(_ptr(lut, C.c_uint8)))
    return lut


def _lut_bytes(lut):
    if lut is None:
        return None
    lut = _arr(lut, np.uint8)
    if lut.shape != (256, 3):
        raise ValueError("lut must be a (256, 3) uint8 table, B G R")
    return lut


def depth_images(ctx, depth, conf, mask, min_depth, max_depth, lut=None):
    """The two images saveDepthMaps writes (utils.cpp:55-58, 82-93) of host maps (dsi_depth_images): (confidence_negated
    uint8 [rows][cols], inv_depth_colored_dilated uint8 [rows][cols][3], B G R).  conf is the confidence map as
    getDepthMapFromDSI returns it; lut a (256, 3) B G R table, None = default_jet_lut()."""
    depth, conf, mask = _arr(depth, np.float32), _arr(conf, np.float32), _arr(mask, np.uint8)
    if depth.ndim != 2 or conf.shape != depth.shape or mask.shape != depth.shape:
        raise ValueError("depth, conf and mask must be 2-D maps of one shape")
    rows, cols = depth.shape
    lut = _lut_bytes(lut)
    neg = np.empty((rows, cols), np.uint8)
    bgr = np.empty((rows, cols, 3), np.uint8)
    _check(load_library().dsi_depth_images(ctx._h, _ptr(depth, C.c_float), _ptr(conf, C.c_float), _ptr(mask, C.c_uint8), rows, cols,
                                           C.c_float(min_depth), C.c_float(max_depth),
                                           None if lut is None else _ptr(lut, C.c_uint8), _ptr(neg, C.c_uint8), _ptr(bgr, C.c_uint8)))
    return neg, bgr


class DepthScore:
    """Depth maps scored against ground-truth depth on the device (dsi_score_*): what the reference's
    scripts/depth_metrics.py and precision_completeness.py compute over the consolidated (windows x H x W) stack, from maps
    added one window at a time.  capacity_points: how many joint pixels' errors the object can hold for the median and the
    curves (8 bytes each); baseline, focal: the b and f of the bad-pixel measure; gt_min: ground truth below it (or not
    finite) is no measurement (the script's 0.05)."""

    def __init__(self, ctx, capacity_points, baseline, focal, gt_min=0.05):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(load_library().dsi_score_create(ctx._h, int(capacity_points), float(baseline), float(focal), float(gt_min),
                                               C.byref(self._h)))
        _track(self)

    def add(self, depth, mask, gt):
        """One window: estimated depth (float32), its mask (non-zero = estimated) and the ground-truth depth, arrays of one
        shape.  Queued on the context's stream."""
        depth, mask, gt = _arr(depth, np.float32), _arr(np.asarray(mask) != 0, np.uint8), _arr(gt, np.float32)
        if depth.shape != mask.shape or depth.shape != gt.shape:
            raise ValueError("depth, mask and gt must have one shape")
        _check(load_library().dsi_score_add(self._h, _ptr(depth, C.c_float), _ptr(mask, C.c_uint8), _ptr(gt, C.c_float),
                                            depth.size))

    def addMapper(self, mapper, gt):
        """One window from the filtered depth map and mask that mapper.getDepthMapFromDSI(..., options_depth_map) /
        filterDepthMap left on the device: only gt is uploaded."""
        gt = _arr(gt, np.float32)
        if gt.shape != (mapper.dimY, mapper.dimX):
            raise ValueError("gt must have the mapper's (dimY, dimX) shape")
        _check(load_library().dsi_score_add_mapper(self._h, mapper._h, _ptr(gt, C.c_float)))

    def metrics(self):
        """dict of the counts (n_est, n_gt, n_joint, n_delta, n_bad, n_stored), overflow, the raw sums (sum_di, sum_di2,
        sum_are, sum_abs), max_gt and the derived delta (3), silog, are, lrmse, badp, mean_abs, median_abs.  After an overflow
        median_abs is NaN; without a joint pixel every real-valued entry is."""
        m = _ScoreMetrics()
        _check(load_library().dsi_score_metrics(self._h, C.byref(m)))
        out = {k: int(getattr(m, k)) for k in ("n_est", "n_gt", "n_joint", "n_bad", "n_stored")}
        out["n_delta"] = [int(v) for v in m.n_delta]
        out["overflow"] = bool(m.overflow)
        out["guard_intact"] = bool(m.guard_intact)
        for k in ("sum_di", "sum_di2", "sum_are", "sum_abs", "max_gt", "silog", "are", "lrmse", "badp", "mean_abs", "median_abs"):
            out[k] = float(getattr(m, k))
        out["delta"] = [float(v) for v in m.delta]
        return out

    def median(self):
        """np.ma.median of the absolute error; raises DsiError after an overflow."""
        v = C.c_double()
        _check(load_library().dsi_score_median(self._h, C.byref(v)))
        return v.value

    def histogram(self, binwidth=0.01):
        """(counts int64 [n_bins], first_edge, last_edge) of np.histogram(err, bins=int(max(err) / binwidth)); n_bins may be 0."""
        L = load_library()
        n, lo, hi = C.c_size_t(), C.c_double(), C.c_double()
        _check(L.dsi_score_histogram(self._h, float(binwidth), None, 0, C.byref(n), C.byref(lo), C.byref(hi)))
        counts = np.zeros(n.value, np.uint64)
        if n.value:
            _check(L.dsi_score_histogram(self._h, float(binwidth), _ptr(counts, C.c_uint64), counts.size, C.byref(n), C.byref(lo),
                                         C.byref(hi)))
        return counts.astype(np.int64), lo.value, hi.value

    def curves(self, binwidth=0.01):
        """precision_completeness.py:43-92: dict of base (the bins' left edges), precision, recall, f1 and outliers (per
        cent, cumulative over the error bins), host arithmetic on the exact counts as the script writes it."""
        m = self.metrics()
        counts, lo, hi = self.histogram(binwidth)
        if counts.size == 0:
            empty = np.zeros(0)
            return {"base": empty, "precision": empty, "recall": empty, "f1": empty, "outliers": empty}
        base = np.linspace(lo, hi, counts.size + 1)[:-1]
        cum = np.cumsum(counts)
        with np.errstate(divide="ignore", invalid="ignore"):
            precision = cum / m["n_est"] * 100
            recall = cum / m["n_gt"] * 100
            f1 = 2 * precision * recall / (precision + recall)
            outliers = (m["n_joint"] - cum) / m["n_joint"] * 100
        return {"base": base, "precision": precision, "recall": recall, "f1": f1, "outliers": outliers}

    def addGroundTruth(self, depth, mask, projector):
        """add() against the depth map that projector (a GroundTruthProjector of this context and of the maps' size) last
        made: the ground truth is read where it lies on the device."""
        depth, mask = _arr(depth, np.float32), _arr(np.asarray(mask) != 0, np.uint8)
        if depth.shape != mask.shape:
            raise ValueError("depth and mask must have one shape")
        _check(load_library().dsi_score_add_gt(self._h, _ptr(depth, C.c_float), _ptr(mask, C.c_uint8), depth.size, projector._h))

    def addMapperGroundTruth(self, mapper, projector):
        """addMapper() against the projector's depth map: both sides are on the device, nothing is uploaded."""
        _check(load_library().dsi_score_add_mapper_gt(self._h, mapper._h, projector._h))

    def addMapRender(self, world_map, gt):
        """One frame from the depth image and mask that world_map.render(...) left on the device (a WorldMap of this
        context), against gt: a host depth map of the render's (height, width) -- only it is uploaded -- or a
        GroundTruthProjector of that size, whose last projection is read where it lies."""
        if isinstance(gt, GroundTruthProjector):
            _check(load_library().dsi_score_add_map_render_gt(self._h, world_map._h, gt._h))
            return
        gt = _arr(gt, np.float32)
        if gt.shape != getattr(world_map, "_render_shape", None):
            raise ValueError("gt must have the render's (height, width) shape")
        _check(load_library().dsi_score_add_map_render(self._h, world_map._h, _ptr(gt, C.c_float)))

    def reset(self):
        _check(load_library().dsi_score_reset(self._h))

    def close(self):
        if self._h:
            load_library().dsi_score_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)


GT_AS_SCRIPT, GT_DROP_OUTSIDE = 0, 1


def disparity_from_png16(raw):
    """The script's `plt.imread(png).astype(np.float32) * 256` from the PNG's uint16 samples (io.read_png_gray16):
    matplotlib's 16-bit rule, float32(raw) / 65535, then * 256 -- two float32 operations, the bits that
    GroundTruthProjector.project_png16 computes on the device."""
    raw = np.asarray(raw)
    if raw.dtype != np.uint16:
        raise ValueError("disparity_from_png16 takes the uint16 samples of the PNG")
    return np.divide(raw.astype(np.float32), np.float32(65535.0), dtype=np.float32) * np.float32(256.0)


class GroundTruthProjector:
    """Ground-truth depth from DSEC disparity images on the device (dsi_gt_*): what
    scripts/evaluate_mcemvs_dsec.py:108-122 computes per frame.  Q (4 x 4), T (4 x 4: the matrix that is applied, the
    script's np.linalg.inv(T_rect0_0)) and K (3 x 4, the script's K_0) are float64.  mode: GT_AS_SCRIPT (a frame with one
    point outside the image gives zeros, like the script's except branch) or GT_DROP_OUTSIDE (such points, and those with a
    negative index, are dropped one by one)."""

    def __init__(self, ctx, width, height, Q, T, K, mode=GT_AS_SCRIPT):
        self.ctx = ctx
        self.width, self.height, self.mode = int(width), int(height), int(mode)
        self._h = C.c_void_p()
        Q, T, K = _arr(Q, np.float64), _arr(T, np.float64), _arr(K, np.float64)
        if Q.shape != (4, 4) or T.shape != (4, 4) or K.shape != (3, 4):
            raise ValueError("Q and T are 4 x 4, K is 3 x 4")
        _check(load_library().dsi_gt_create(ctx._h, self.width, self.height, _ptr(Q, C.c_double), _ptr(T, C.c_double),
                                            _ptr(K, C.c_double), self.mode, C.byref(self._h)))
        _track(self)

    def _frame(self, a, dtype):
        if np.asarray(a).dtype != dtype:
            raise ValueError("expected a %s image" % np.dtype(dtype).name)
        a = _arr(a, dtype)
        if a.shape != (self.height, self.width):
            raise ValueError("the image must have the projector's (height, width) = (%d, %d)" % (self.height, self.width))
        return a

    def project(self, disp):
        """disp: float32 [height][width], the script's d.  Queued on the context's stream; the map stays on the device."""
        disp = self._frame(disp, np.float32)
        _check(load_library().dsi_gt_project(self._h, _ptr(disp, C.c_float)))

    def project_png16(self, raw):
        """raw: the uint16 samples of the disparity PNG (io.read_png_gray16); converted on the device."""
        raw = self._frame(raw, np.uint16)
        _check(load_library().dsi_gt_project_u16(self._h, _ptr(raw, C.c_uint16)))

    def fetch(self):
        """(depth float32 [height][width], n_points, n_outside) of the last projection.  Synchronises."""
        depth = np.zeros((self.height, self.width), np.float32)
        n, o = C.c_uint64(), C.c_uint64()
        _check(load_library().dsi_gt_fetch(self._h, _ptr(depth, C.c_float), C.byref(n), C.byref(o)))
        return depth, int(n.value), int(o.value)

    def device_ptr(self):
        return load_library().dsi_gt_device_ptr(self._h)

    def close(self):
        if self._h:
            load_library().dsi_gt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)


def thicken_edges(ctx, depth, mask, no_estimate=255.0):
    """scripts/evaluate_mcemvs_dsec.py:75-79 with thicken_edges = True: (depth, mask) eroded by the 3 x 3 cross on the
    device, pixels without an estimate standing at no_estimate (the script's 255) -- every estimate grows into its four
    neighbours, the smaller depth winning."""
    depth, mask = _arr(depth, np.float32), _arr(np.asarray(mask) != 0, np.uint8)
    if depth.ndim != 2 or depth.shape != mask.shape:
        raise ValueError("depth and mask must be 2-D and of one shape")
    out_d, out_m = np.zeros_like(depth), np.zeros_like(mask)
    _check(load_library().dsi_depth_erode(ctx._h, _ptr(depth, C.c_float), _ptr(mask, C.c_uint8), depth.shape[0], depth.shape[1],
                                          float(no_estimate), _ptr(out_d, C.c_float), _ptr(out_m, C.c_uint8)))
    return out_d, out_m


class Lens:
    """A camera's calibration numbers as sensor_msgs::CameraInfo holds them (dsi_lens_t): model "plumb_bob" /
    "fisheye" (or LENS_PLUMB_BOB / LENS_FISHEYE), K 3 x 3, D the distortion coefficients (plumb_bob: 0, 4, 5 or 8 of
    k1 k2 p1 p2 k3 k4 k5 k6; fisheye: k1..k4), R 3 x 3 (default: the identity), P 3 x 4 (default: [K | 0]; its fourth column
    is not read).  The constructor only stores them; check() is dsi_lens_check, which every entry point applies itself."""

    MODELS = {"plumb_bob": LENS_PLUMB_BOB, "fisheye": LENS_FISHEYE}

    def __init__(self, model, K, D, R=None, P=None):
        if isinstance(model, str):
            if model not in self.MODELS:
                raise ValueError("Distortion model not set properly: %r (expected plumb_bob or fisheye)" % (model,))
            model = self.MODELS[model]
        self.model = int(model)
        self.K = np.array(K, np.float64).reshape(3, 3)
        self.D = np.array(D, np.float64).reshape(-1)
        if self.D.size > 8:
            raise ValueError("at most 8 distortion coefficients (got %d)" % self.D.size)
        self.R = np.eye(3) if R is None else np.array(R, np.float64).reshape(3, 3)
        self.P = np.hstack([self.K, np.zeros((3, 1))]) if P is None else np.array(P, np.float64).reshape(3, 4)

    def _c(self):
        c = _Lens()
        c.model, c.n_dist = self.model, int(self.D.size)
        c.K = (C.c_double * 9)(*self.K.ravel())
        c.D = (C.c_double * 8)(*self.D, *([0.0] * (8 - self.D.size)))
        c.R = (C.c_double * 9)(*self.R.ravel())
        c.P = (C.c_double * 12)(*self.P.ravel())
        return c

    def check(self):
        """Raises DsiError(ERR_INVALID) for what dsi_lens_check refuses.  Host only."""
        _check(load_library().dsi_lens_check(C.byref(self._c())))

    def rr(self):
        """P[:, :3] R as the engine multiplies it (dsi_lens_rr): the matrix applied to the undistorted point.  Host only."""
        out = np.zeros((3, 3), np.float64)
        _check(load_library().dsi_lens_rr(C.byref(self._c()), _ptr(out, C.c_double)))
        return out


def rectify_lut(ctx, lens, width, height):
    """The table of precomputeRectifiedPoints (mapper_emvs_stereo.cpp:256-299) for `lens`, made on the device: float32
    [height * width, 2], entry y * width + x = the rectified position of the raw pixel (x, y).  Synchronises."""
    n = max(int(width), 0) * max(int(height), 0)
    lut = np.empty((n, 2), np.float32)
    _check(load_library().dsi_rectify_lut(ctx._h, C.byref(lens._c()), int(width), int(height), _ptr(lut, C.c_float)))
    return lut


def rectify_lut_dev(ctx, lens, width, height, device_ptr):
    """The same into device memory (2 * width * height floats, e.g. Grid3D.device_ptr), queued without a synchronise."""
    _check(load_library().dsi_rectify_lut_dev(ctx._h, C.byref(lens._c()), int(width), int(height), C.c_void_p(device_ptr)))


class PinnedArray:
    """numpy array in page-locked host memory (dsi_host_alloc): the source / destination of
    asynchronous uploads and depth-map fetches.  `a` is the array; close() frees the memory."""

    def __init__(self, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        self._p = C.c_void_p()
        _check(load_library().dsi_host_alloc(max(1, n * dtype.itemsize), C.byref(self._p)))
        buf = (C.c_uint8 * (n * dtype.itemsize)).from_address(self._p.value)
        self.a = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
        _track(self)

    def close(self):
        if self._p:
            self.a = None
            load_library().dsi_host_free(self._p)
        self._p = C.c_void_p()

    def __del__(self):
        _safe_del(self)


class EventBatch:
    """Device-resident events of one evaluateDSI call + their packetisation
    (mapper_emvs_stereo.cpp:88-105).  asynchronous=True: x, y, Rt, packet_first are views of
    PinnedArray memory that the caller leaves alone until uploaded() (or a later synchronisation of
    the context that evaluated the batch); the constructor then returns without waiting."""

    def __init__(self, ctx, x, y, Rt, packet_first=None, asynchronous=False):
        x = _arr(x, np.uint16)
        y = _arr(y, np.uint16)
        Rt = _arr(Rt, np.float32).reshape(-1, 12)
        pf = None
        if packet_first is not None:
            packet_first = _arr(packet_first, np.uint32)
            pf = _ptr(packet_first, C.c_uint32)
        self.ctx = ctx
        self.n_packets = Rt.shape[0]
        self.n_events = x.shape[0]
        self._h = C.c_void_p()
        L = load_library()
        fn = L.dsi_batch_create_async if asynchronous else L.dsi_batch_create
        if asynchronous:
            self._keep = (x, y, Rt, packet_first)   # the views (not the pinned memory itself)
        _check(fn(ctx._h, _ptr(x, C.c_uint16), _ptr(y, C.c_uint16), x.shape[0], pf, _ptr(Rt, C.c_float),
                  Rt.shape[0], C.byref(self._h)))
        _track(self)

    def uploaded(self):
        return bool(load_library().dsi_batch_uploaded(self._h))

    def event_image(self, polarity, width, height, use_polarity=True, return_dropped=False):
        """accumulate_events of the events this batch holds on the device (dsi_batch_event_image): only the polarity
        bytes are uploaded."""
        pol = _polarity_bytes(polarity, self.n_events, use_polarity)
        out = np.empty((max(int(height), 0), max(int(width), 0)), np.uint8)
        dropped = C.c_size_t()
        _check(load_library().dsi_batch_event_image(self._h, None if pol is None else _ptr(pol, C.c_uint8), int(width),
                                                    int(height), int(bool(use_polarity)), _ptr(out, C.c_uint8),
                                                    C.byref(dropped)))
        return (out, dropped.value) if return_dropped else out

    def close(self):
        if self._h:
            load_library().dsi_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)


class MapperEMVS:
    """Device-resident counterpart of EMVS::MapperEMVS (mapper_emvs_stereo.hpp:94-155).

    cam = (width, height, fx, fy, cx, cy): full resolution and the projection-matrix
    intrinsics the reference reads from image_geometry::PinholeCameraModel
    (mapper_emvs_stereo.cpp:34-48).  lut = undistortion table of
    precomputeRectifiedPoints (mapper_emvs_stereo.cpp:256-299), shape [H*W][2] or None; lens = a Lens
    instead: the engine makes that table on the device, in the mapper's own buffer (dsi_mapper_create_with_lens).
    """

    def __init__(self, ctx, cam, dsi_shape, lut=None, inverse_depth=False, plane_range=None, lens=None):
        """plane_range = (begin, count): own only those planes of dsi_shape's dimZ planes (plane
        sharding across GPUs; the DSI then has `count` planes and equals that slice of the full one)."""
        if lut is not None and lens is not None:
            raise ValueError("lut and lens exclude each other")
        w, h, fx, fy, cx, cy = cam
        cfg = _MapperConfig()
        if plane_range is not None:
            cfg.plane_begin, cfg.plane_count = int(plane_range[0]), int(plane_range[1])
        cfg.sensor_width, cfg.sensor_height = int(w), int(h)
        cfg.K = (C.c_float * 4)(fx, fy, cx, cy)
        cfg.dim_x, cfg.dim_y, cfg.dim_z = dsi_shape.dimX_, dsi_shape.dimY_, dsi_shape.dimZ_
        cfg.min_depth, cfg.max_depth, cfg.fov_deg = (dsi_shape.min_depth_, dsi_shape.max_depth_,
                                                     dsi_shape.fov_)
        cfg.inverse_depth = 1 if inverse_depth else 0
        self._lut = None
        if lut is not None:
            self._lut = _arr(lut, np.float32).reshape(int(w) * int(h), 2)
            cfg.lut = _ptr(self._lut, C.c_float)
        self.ctx = ctx
        self._h = C.c_void_p()
        L = load_library()
        if lens is not None:
            _check(L.dsi_mapper_create_with_lens(ctx._h, C.byref(cfg), C.byref(lens._c()), C.byref(self._h)))
        else:
            _check(L.dsi_mapper_create(ctx._h, C.byref(cfg), C.byref(self._h)))
        _track(self)
        nx, ny, nz = C.c_int(), C.c_int(), C.c_int()
        kv = (C.c_float * 4)()
        _check(L.dsi_mapper_geometry(self._h, kv, None, C.byref(nx), C.byref(ny), C.byref(nz)))
        self.dimX, self.dimY, self.dimZ = nx.value, ny.value, nz.value
        planes = np.empty(self.dimZ, np.float32)
        _check(L.dsi_mapper_geometry(self._h, None, _ptr(planes, C.c_float), None, None, None))
        self.raw_depths_vec_ = planes
        self.plane_begin = int(L.dsi_mapper_plane_begin(self._h))
        nfull = C.c_int()
        _check(L.dsi_mapper_full_depths(self._h, None, C.byref(nfull)))
        self.full_depths_ = np.empty(nfull.value, np.float32)   # whole depth vector (plane shards index into it)
        _check(L.dsi_mapper_full_depths(self._h, _ptr(self.full_depths_, C.c_float), None))
        self.virtual_cam_ = tuple(float(v) for v in kv)  # fx, fy, cx, cy
        # public member dsi_ (mapper_emvs_stereo.hpp:116)
        self.dsi_ = Grid3D(ctx, 0, 0, 0, _handle=C.c_void_p(L.dsi_mapper_grid(self._h)), _owner=self)
        self.name = ""

    def close(self):
        if self._h:
            load_library().dsi_mapper_destroy(self._h)
            self._h = C.c_void_p()
            self.dsi_._h = C.c_void_p()

    def __del__(self):
        _safe_del(self)

    def set_vote_algo(self, algo):
        _check(load_library().dsi_mapper_set_vote_algo(self._h, int(algo)))

    def set_band_params(self, band_rows=0, chunks=0, block_threads=0):
        _check(load_library().dsi_mapper_set_band_params(self._h, int(band_rows), int(chunks),
                                                         int(block_threads)))

    def set_packed_lanes(self, mode=-1):
        _check(load_library().dsi_mapper_set_packed_lanes(self._h, int(mode)))

    def paired_overflow(self):
        """Lane mapping 8 (paired 32-bit cells): did a cell of the last vote reach half its capacity?  (Then vote again
        with an exact mapping.)"""
        flag = C.c_int(0)
        _check(load_library().dsi_mapper_paired_overflow(self._h, C.byref(flag)))
        return bool(flag.value)

    def set_inline_cuts(self, min_packets=-1):
        """Lane mappings 5 / 6: from how many packets per call on the voting kernel derives the packets' runs itself
        instead of reading a cut table (-1 = default 8192, 0 = always)."""
        _check(load_library().dsi_mapper_set_inline_cuts(self._h, int(min_packets)))

    def last_vote_info(self):
        info = _VoteInfo()
        _check(load_library().dsi_mapper_last_vote_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in _VoteInfo._fields_}

    def vote_statistics(self, batch):
        """(accepted event-planes, accepted records) of voting `batch`: the DSI's sum, and the same count after the
        packet sort merged same-pixel events of a packet (= LDS atomics issued / 4).  Votes twice; the DSI is left as
        evaluateDSI_batch leaves it."""
        a, r = C.c_double(), C.c_double()
        _check(load_library().dsi_mapper_vote_statistics(self._h, batch._h, C.byref(a), C.byref(r)))
        return a.value, r.value

    def set_kernel_timing(self, enable=True):
        _check(load_library().dsi_mapper_set_kernel_timing(self._h, 1 if enable else 0))

    def vote_kernel_time(self):
        """(total ms, launches) of the voting kernel since the last call (HIP events)."""
        ms, n = C.c_float(), C.c_int()
        _check(load_library().dsi_mapper_vote_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def evaluateDSI(self, events, trajectory, T_rv_w):
        """mapper_emvs_stereo.cpp:67-148.  events = (x uint16[n], y uint16[n], ts float64[n]);
        trajectory = (times float64[m], poses float64[m][7] as tx,ty,tz,qw,qx,qy,qz);
        T_rv_w = 7 doubles.  Returns False where the reference returns false."""
        x, y, ts = events
        x, y, ts = _arr(x, np.uint16), _arr(y, np.uint16), _arr(ts, np.float64)
        times, poses = trajectory
        times, poses = _arr(times, np.float64), _arr(poses, np.float64).reshape(-1, 7)
        T = _arr(T_rv_w, np.float64)
        voted = C.c_size_t()
        rc = load_library().dsi_mapper_evaluate(
            self._h, _ptr(x, C.c_uint16), _ptr(y, C.c_uint16), _ptr(ts, C.c_double), x.shape[0],
            _ptr(times, C.c_double), _ptr(poses, C.c_double), times.shape[0], _ptr(T, C.c_double),
            C.byref(voted))
        if rc == ERR_TOO_FEW_EVENTS:
            return False
        _check(rc)
        self.n_voted = voted.value
        return True

    def evaluateDSI_batch(self, batch):
        """evaluateDSI past the pose lookup, on a device-resident EventBatch (asynchronous)."""
        _check(load_library().dsi_mapper_evaluate_batch(self._h, batch._h))

    def fillVoxelGrid(self, event_locations_z0, camera_centers):
        """mapper_emvs_stereo.cpp:151-205 (private in the reference; the parity test point).
        Accumulates into dsi_ without resetting it."""
        xy = _arr(event_locations_z0, np.float32).reshape(-1, 2)
        cc = _arr(camera_centers, np.float32).reshape(-1, 3)
        if xy.shape[0] != cc.shape[0] * PACKET_SIZE:
            raise DsiError(ERR_INVALID, "need 1024 event locations per camera centre")
        _check(load_library().dsi_mapper_fill_voxel_grid(self._h, _ptr(xy, C.c_float),
                                                         _ptr(cc, C.c_float), cc.shape[0]))

    def getDepthMapFromDSI(self, grid=None, options_depth_map=None, method=-1):
        """mapper_emvs_stereo.cpp:339-437.  With options_depth_map (OptionsDepthMap): the full
        extraction -- arg-max, confidence normalisation, Gaussian adaptive threshold, masked
        median, border removal -- returning (depth_map, confidence_map, mask) like the
        reference's signature (dense inpainted map excluded).  Without: the raw arg-max
        (:368) + convertDepthIndicesToValues (:302-313), returning (depth, confidence, indices).
        method 0..4 (FOCUS_*) replaces the arg-max by that focus-based collapse (:348-364; GradMag with
        half_patchsize 1); any other value is the arg-max."""
        L = load_library()
        if 0 <= method <= 4:
            _check(L.dsi_mapper_depth_map_of_focus(self._h, (grid or self.dsi_)._h, int(method)))
            if options_depth_map is None:
                return self.fetchDepthMap()
            return self.filterDepthMap(options_depth_map)
        if options_depth_map is not None:
            o = options_depth_map
            opts = _DepthMapOptions(o.adaptive_threshold_kernel_size_, o.adaptive_threshold_c_,
                                    o.median_filter_size_, o.max_confidence)
            depth = np.empty((self.dimY, self.dimX), np.float32)
            conf = np.empty((self.dimY, self.dimX), np.float32)
            mask = np.empty((self.dimY, self.dimX), np.uint8)
            self.depth_cell_indices_filtered = np.empty((self.dimY, self.dimX), np.uint8)
            _check(L.dsi_mapper_get_depth_map_from_dsi(
                self._h, (grid or self.dsi_)._h, C.byref(opts), _ptr(depth, C.c_float), _ptr(conf, C.c_float),
                _ptr(mask, C.c_uint8), _ptr(self.depth_cell_indices_filtered, C.c_uint8)))
            return depth, conf, mask
        _check(L.dsi_mapper_depth_map_of(self._h, (grid or self.dsi_)._h))
        return self.fetchDepthMap()

    def filterDepthMap(self, options_depth_map):
        """mapper_emvs_stereo.cpp:390-437 -- everything getDepthMapFromDSI does after
        collapseMaxZSlice -- on the raw depth map this mapper holds from the last computeDepthMap /
        computeDepthMapOfFusion / computeDepthMapOfEvents call: (depth_map, confidence_map, mask).
        The way to the reference's filtered per-window outputs when no DSI is materialised."""
        o = options_depth_map
        opts = _DepthMapOptions(o.adaptive_threshold_kernel_size_, o.adaptive_threshold_c_,
                                o.median_filter_size_, o.max_confidence)
        depth = np.empty((self.dimY, self.dimX), np.float32)
        conf = np.empty((self.dimY, self.dimX), np.float32)
        mask = np.empty((self.dimY, self.dimX), np.uint8)
        self.depth_cell_indices_filtered = np.empty((self.dimY, self.dimX), np.uint8)
        _check(load_library().dsi_mapper_filter_depth_map(
            self._h, C.byref(opts), _ptr(depth, C.c_float), _ptr(conf, C.c_float), _ptr(mask, C.c_uint8),
            _ptr(self.depth_cell_indices_filtered, C.c_uint8)))
        return depth, conf, mask

    def getPointcloud(self, depth_map=None, mask=None, options_pc=None):
        """MapperEMVS::getPointcloud (mapper_emvs_stereo.cpp:440-480) on the device: the pixels with mask > 0
        back-projected through the virtual camera (double, row-major order), then PCL's RadiusOutlierRemoval
        (radius_outlier_removal's count rule).  Returns an (N, 4) float32 array of x, y, z, intensity = 1 / z;
        self.n_unfiltered_ is the count before the filter.  With depth_map and mask both None: the filtered maps the
        last getDepthMapFromDSI(..., options_depth_map) / filterDepthMap left on the device (no upload)."""
        if (depth_map is None) != (mask is None):
            raise ValueError("pass both depth_map and mask, or neither")
        o = options_pc or OptionsPointCloud()
        opts = _PointCloudOptions(o.radius_search_, o.min_num_neighbors_)
        npix = self.dimX * self.dimY
        out = np.empty((npix, 4), np.float32)
        n, n0 = C.c_size_t(), C.c_size_t()
        dp = mp = None
        if depth_map is not None:
            depth_map = _arr(depth_map, np.float32)
            mask = _arr(mask, np.uint8)
            if depth_map.shape != (self.dimY, self.dimX) or mask.shape != (self.dimY, self.dimX):
                raise ValueError("depth_map and mask must be (dimY, dimX)")
            dp, mp = _ptr(depth_map, C.c_float), _ptr(mask, C.c_uint8)
        _check(load_library().dsi_mapper_get_pointcloud(self._h, dp, mp, C.byref(opts), _ptr(out, C.c_float), npix,
                                                        C.byref(n), C.byref(n0)))
        self.n_unfiltered_ = n0.value
        return out[:n.value].copy()

    def depthImages(self, min_depth, max_depth, lut=None):
        """depth_images of the filtered maps the last getDepthMapFromDSI(..., options_depth_map) / filterDepthMap left on
        the device (dsi_mapper_depth_images; no upload): (confidence_negated, inv_depth_colored_dilated)."""
        lut = _lut_bytes(lut)
        neg = np.empty((self.dimY, self.dimX), np.uint8)
        bgr = np.empty((self.dimY, self.dimX, 3), np.uint8)
        _check(load_library().dsi_mapper_depth_images(self._h, C.c_float(min_depth), C.c_float(max_depth),
                                                      None if lut is None else _ptr(lut, C.c_uint8), _ptr(neg, C.c_uint8),
                                                      _ptr(bgr, C.c_uint8)))
        return neg, bgr

    def computeDepthMap(self, grid=None):
        """Asynchronous half of getDepthMapFromDSI; pair with fetchDepthMap()."""
        _check(load_library().dsi_mapper_depth_map_of(self._h, (grid or self.dsi_)._h))

    def computeDepthMapOfFusion(self, grid_a, grid_b, fusion_method):
        """computeDepthMap of op(grid_a, grid_b) without materialising the fused DSI (bit-identical to
        setToFusionOf + computeDepthMap; one pass over the two volumes)."""
        _check(load_library().dsi_mapper_depth_map_of_fusion(self._h, grid_a._h, grid_b._h, int(fusion_method)))

    def computeDepthMapOfFusionN(self, grids, mode):
        """computeDepthMap of the n-ary fusion of up to 8 grids (mode = ACC_*) without materialising
        the fused DSI: bit-identical to Grid3D.setToFusionOfN + computeDepthMap."""
        hs = (C.c_void_p * len(grids))(*[g._h for g in grids])
        _check(load_library().dsi_mapper_depth_map_of_fusion_n(self._h, hs, len(grids), int(mode)))

    def computeDepthMapOfEvents(self, mappers, batches, fusion_method=FUSE_HM):
        """Depth map of 1, 2 or 3 cameras' events without building their DSIs: one kernel votes each
        (band, plane) of every camera into LDS, fuses the cameras per voxel and keeps the running
        arg-max in registers (dsi_mapper_depth_map_of_events).  Bit-identical to evaluateDSI_batch on
        every mapper + computeDepthMapOfFusion (or computeDepthMap for one camera; for three, the
        trinocular sequence of process1.cpp:126-191: the 2-ary op, then min / harmonicMeanTwoGrids(g, 3) /
        max with camera 2 -- ops 3, 4, 5 ignore it like the reference); the mappers' DSIs
        are not touched.  Results land in THIS mapper's depth-map buffers (fetchDepthMap)."""
        hm = (C.c_void_p * len(mappers))(*[m._h for m in mappers])
        hb = (C.c_void_p * len(batches))(*[b._h for b in batches])
        _check(load_library().dsi_mapper_depth_map_of_events(self._h, hm, hb, len(mappers), int(fusion_method)))

    def computeDepthMapOfEventsN(self, mappers, batches, mode=None):
        """Depth map of four (or two) cameras' events fused by the geometric-mean tree (ACC_GM_TREE) without building their
        DSIs (dsi_mapper_depth_map_of_events_n): bit-identical to evaluateDSI_batch on every mapper +
        computeDepthMapOfFusionN([m.dsi_ ...], ACC_GM_TREE).  Results in THIS mapper's depth-map buffers."""
        hm = (C.c_void_p * len(mappers))(*[m._h for m in mappers])
        hb = (C.c_void_p * len(batches))(*[b._h for b in batches])
        _check(load_library().dsi_mapper_depth_map_of_events_n(self._h, hm, hb, len(mappers),
                                                               int(ACC_GM_TREE if mode is None else mode)))

    def computeDepthMapOfEventsAlg2(self, mapper_camera_time, mappers, batches, num_subintervals, stereo_fusion,
                                    temporal_fusion):
        """Alg. 2 of one window (process_2 / process_5) without a DSI (dsi_mapper_depth_map_of_events_alg2): THIS mapper
        receives the depth map of the reference's mapper_fused ("time_camera"), mapper_camera_time (None: not computed)
        that of mapper_fused_camera_time -- bit-identical to process.process_2 + computeDepthMap of those two DSIs.
        mappers: the two cameras' mappers (calibrations; their DSIs are not touched); batches: 2 * num_subintervals
        EventBatch, k-major (camera 0, camera 1 of sub-interval k), packetised against reference_view_process2."""
        n = int(num_subintervals)
        if len(mappers) != 2 or len(batches) != 2 * n:
            raise DsiError(ERR_INVALID, "two camera mappers and 2 * num_subintervals batches")
        hm = (C.c_void_p * 2)(*[m._h for m in mappers])
        hb = (C.c_void_p * len(batches))(*[b._h for b in batches])
        _check(load_library().dsi_mapper_depth_map_of_events_alg2(
            self._h, mapper_camera_time._h if mapper_camera_time is not None else None, hm, hb, n, int(stereo_fusion),
            int(temporal_fusion)))

    def resolveNearTies(self, mappers, batches, fusion_method=FUSE_HM, rel_gap=0.0):
        """Exact tie resolver (dsi_mapper_resolve_near_ties): after the mappers' DSIs were built from `batches`
        (evaluateDSI_batch) and this mapper holds the depth map of their fusion, re-sum the contending voxels of the
        near-tie columns in the REFERENCE's summation order (fp32, event order) and re-pick the first maximum, so that
        the plane index map equals the CPU reference's on every pixel.  Returns the call's statistics (dict)."""
        n = len(mappers)
        hm = (C.c_void_p * n)(*[m._h for m in mappers])
        hb = (C.c_void_p * n)(*[b._h for b in batches])
        info = _ResolveInfo()
        info.rel_gap = float(rel_gap)
        _check(load_library().dsi_mapper_resolve_near_ties(self._h, hm, hb, n, int(fusion_method), C.byref(info)))
        return {k: getattr(info, k) for k, _ in _ResolveInfo._fields_}

    def proveNearTies(self, mappers, batches, fusion_method=FUSE_HM, rel_gap=0.0):
        """The resolver's premise as a per-column proof (dsi_mapper_prove_near_ties; a verification pass): counts the votes of
        every voxel of the mappers' DSIs (built from `batches`) and checks, with rigorous bounds of the reference's fp32
        event-order sums, that in every column no plane outside `rel_gap` of the maximum can be the reference's first
        maximum.  Returns {columns, columns_proven, columns_unproven, gap_needed, max_votes, elapsed_ms, rel_gap}."""
        n = len(mappers)
        hm = (C.c_void_p * n)(*[m._h for m in mappers])
        hb = (C.c_void_p * n)(*[b._h for b in batches])
        info = _ProveInfo()
        info.rel_gap = float(rel_gap)
        _check(load_library().dsi_mapper_prove_near_ties(self._h, hm, hb, n, int(fusion_method), C.byref(info)))
        return {k: getattr(info, k) for k, _ in _ProveInfo._fields_}

    def proveNearTiesN(self, mappers, batches, mode, fused_grid=None, rel_gap=0.0):
        """dsi_mapper_prove_near_ties_n: the per-column proof for n <= 8 cameras fused by an n-ary mode (ACC_GM_TREE with
        2 / 4 / 8 cameras, ACC_MIN, ACC_MAX, ACC_SUM); fused_grid: the grid that holds the fusion (default: this mapper's
        dsi_), whose values decided the near-tie columns."""
        n = len(mappers)
        hm = (C.c_void_p * n)(*[m._h for m in mappers])
        hb = (C.c_void_p * n)(*[b._h for b in batches])
        info = _ProveInfo()
        info.rel_gap = float(rel_gap)
        g = fused_grid if fused_grid is not None else self.dsi_
        _check(load_library().dsi_mapper_prove_near_ties_n(self._h, g._h, hm, hb, n, int(mode), C.byref(info)))
        return {k: getattr(info, k) for k, _ in _ProveInfo._fields_}

    def referenceInterval(self, mapper, batch, lo, hi):
        """dsi_mapper_reference_interval: lo, hi (Grid3D) <- voxel-wise bounds of the value the reference holds in the DSI
        `mapper` built from `batch` (its votes counted; this mapper lends the scratch)."""
        _check(load_library().dsi_mapper_reference_interval(self._h, mapper._h, batch._h, lo._h, hi._h))

    def proveColumns(self, fused, lo, hi, rel_gap=0.0):
        """dsi_grid_prove_columns: every column of `fused` (the engine's values) against the interval grids lo / hi."""
        info = _ProveInfo()
        info.rel_gap = float(rel_gap)
        _check(load_library().dsi_grid_prove_columns(self._h, fused._h, lo._h, hi._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in _ProveInfo._fields_}

    def proofUnproven(self):
        """dsi_mapper_proof_unproven: (pixels uint32[n], gaps float32[n]) -- the columns the last proveNearTies could not
        prove and the rel_gap each of them alone would need."""
        n = C.c_size_t(0)
        lib = load_library()
        _check(lib.dsi_mapper_proof_unproven(self._h, None, None, 0, C.byref(n)))
        pixels, gaps = np.empty(n.value, np.uint32), np.empty(n.value, np.float32)
        if n.value:
            _check(lib.dsi_mapper_proof_unproven(self._h, _ptr(pixels, C.c_uint32), _ptr(gaps, C.c_float), n.value, C.byref(n)))
        return pixels, gaps

    def proofVotes(self, camera, voxels):
        """dsi_mapper_proof_votes: the votes of the listed voxels of camera 0 / 1 as the last proveNearTies counted them."""
        voxels = _arr(voxels, np.uint32)
        votes = np.empty(voxels.shape, np.uint32)
        _check(load_library().dsi_mapper_proof_votes(self._h, int(camera), _ptr(voxels, C.c_uint32), voxels.size,
                                                     _ptr(votes, C.c_uint32)))
        return votes

    def nearTieVoxels(self, grid=None, rel_gap=0.0):
        """dsi_grid_near_tie_voxels of `grid` (default: this mapper's DSI): the voxels (linear indices z*Ny*Nx + y*Nx + x)
        within rel_gap of their column's maximum, for columns with >= 2 of them; a column's run contiguous, planes
        ascending.  Returns (voxels uint32[n], n_columns)."""
        g = self.dsi_ if grid is None else grid
        cap = 1 << 16
        while True:
            vox = np.empty(cap, np.uint32)
            n, cols = C.c_size_t(), C.c_size_t()
            _check(load_library().dsi_grid_near_tie_voxels(self._h, g._h, float(rel_gap), _ptr(vox, C.c_uint32), cap,
                                                           C.byref(n), C.byref(cols)))
            if n.value <= cap:
                return vox[:n.value].copy(), cols.value
            cap = n.value

    def exactVoxels(self, batch, voxels):
        """dsi_mapper_exact_voxels: (values float32[n], votes uint32[n]) of the listed voxels of the DSI this mapper
        builds from `batch`, summed the way the reference sums (fp32, event order)."""
        voxels = _arr(voxels, np.uint32)
        values = np.empty(voxels.shape, np.float32)
        votes = np.empty(voxels.shape, np.uint32)
        _check(load_library().dsi_mapper_exact_voxels(self._h, batch._h, _ptr(voxels, C.c_uint32), voxels.size,
                                                      _ptr(values, C.c_float), _ptr(votes, C.c_uint32)))
        return values, votes

    def patchDepthMap(self, pixels, idx, conf):
        """dsi_mapper_patch_depth_map: overwrite pixels (y*Nx + x) of the raw depth map held on the device."""
        pixels, idx, conf = _arr(pixels, np.uint32), _arr(idx, np.uint8), _arr(conf, np.float32)
        _check(load_library().dsi_mapper_patch_depth_map(self._h, _ptr(pixels, C.c_uint32), _ptr(idx, C.c_uint8),
                                                         _ptr(conf, C.c_float), pixels.size))

    def computeDepthMapSharded(self, grid, comm):
        """Plane-sharded arg-max: local collapse of this rank's plane range, ONE all-reduce(MAX) of
        packed (confidence, index) keys, index -> depth over the full depth vector; fetchDepthMap()
        then returns the unsharded result on every rank."""
        _check(load_library().dsi_mapper_depth_map_sharded(self._h, (grid or self.dsi_)._h, comm._h))

    def computeDepthMapReduceScattered(self, acc, comm, mode, n_maps):
        """Temporal fusion's last step across GPUs with a reduce-scatter instead of an all-reduce: `acc` (this
        rank's accumulated slices, mode = ACC_*) is reduced by plane ranges, every rank finalises and arg-maxes
        its planes, one all-reduce(MAX) of packed keys -> the fused depth map on every rank (fetchDepthMap).
        `acc` is consumed."""
        _check(load_library().dsi_mapper_depth_map_reduce_scattered(self._h, acc._h, comm._h, int(mode), int(n_maps)))

    def computeDepthMapScatteredLocal(self, acc, nranks, rank, mode, n_maps):
        """The local step of computeDepthMapReduceScattered for a caller-provided transport: finalize + arg-max of
        the planes scatter_plan(dimZ, nranks, rank) gives this rank -> packed keys on the device (argmaxKeys)."""
        _check(load_library().dsi_mapper_depth_map_scattered_local(self._h, acc._h, int(nranks), int(rank), int(mode),
                                                                   int(n_maps)))

    def argmaxKeys(self):
        ny, nx = self.dsi_.shape[1:]
        keys = np.empty((ny, nx), np.uint64)
        _check(load_library().dsi_mapper_argmax_keys_download(self._h, _ptr(keys, C.c_uint64)))
        return keys

    def setArgmaxKeys(self, keys):
        keys = _arr(keys, np.uint64)
        ny, nx = self.dsi_.shape[1:]
        assert keys.shape == (ny, nx)
        _check(load_library().dsi_mapper_argmax_keys_upload(self._h, _ptr(keys, C.c_uint64)))

    def computeDepthMapFromKeys(self):
        """keys (after the caller's MAX over the ranks) -> confidence / index / depth (fetchDepthMap)."""
        _check(load_library().dsi_mapper_depth_map_from_keys(self._h))

    def fetchDepthMapAsync(self, depth, conf, idx):
        """Queue the device -> host copies into PinnedArray-backed arrays (any may be None) on the copy
        stream; they are valid after fetchWait()."""
        _check(load_library().dsi_mapper_fetch_depth_map_async(
            self._h, None if depth is None else _ptr(depth, C.c_float),
            None if conf is None else _ptr(conf, C.c_float), None if idx is None else _ptr(idx, C.c_uint8)))

    def fetchWait(self):
        _check(load_library().dsi_mapper_fetch_wait(self._h))

    def fetchDepthMapInOrder(self, depth, conf, idx):
        """Like fetchDepthMapAsync, but on the context's COMPUTE stream behind whatever it holds (no second stream per
        context: for pipelines with one context per window in flight); valid after fetchWait()."""
        _check(load_library().dsi_mapper_fetch_depth_map_in_order(
            self._h, None if depth is None else _ptr(depth, C.c_float),
            None if conf is None else _ptr(conf, C.c_float), None if idx is None else _ptr(idx, C.c_uint8)))

    def fetchDepthMap(self, in_order=False):
        """(depth, confidence, indices) on the host (synchronises).  in_order: the copies go on the compute stream (see
        fetchDepthMapInOrder) instead of the context's copy stream."""
        depth = np.empty((self.dimY, self.dimX), np.float32)
        conf = np.empty((self.dimY, self.dimX), np.float32)
        idx = np.empty((self.dimY, self.dimX), np.uint8)
        if in_order:
            self.fetchDepthMapInOrder(depth, conf, idx)
            self.fetchWait()                       # (pageable destinations: the runtime has copied by then)
            _check(load_library().dsi_context_synchronize(self.ctx._h))
            return depth, conf, idx
        _check(load_library().dsi_mapper_fetch_depth_map(self._h, _ptr(depth, C.c_float),
                                                         _ptr(conf, C.c_float), _ptr(idx, C.c_uint8)))
        return depth, conf, idx


def packetize(ts, trajectory, T_rv_w):
    """Host packetisation + pose pipeline of evaluateDSI (mapper_emvs_stereo.cpp:67-105).
    Returns (packet_first uint32[np], Rt float32[np][12]) or None when the reference
    would return false."""
    ts = _arr(ts, np.float64)
    times, poses = trajectory
    times, poses = _arr(times, np.float64), _arr(poses, np.float64).reshape(-1, 7)
    T = _arr(T_rv_w, np.float64)
    cap = ts.shape[0] // PACKET_SIZE + 1
    first = np.empty(cap, np.uint32)
    Rt = np.empty((cap, 12), np.float32)
    n = C.c_size_t()
    rc = load_library().dsi_packetize(_ptr(ts, C.c_double), ts.shape[0], _ptr(times, C.c_double),
                                      _ptr(poses, C.c_double), times.shape[0], _ptr(T, C.c_double),
                                      _ptr(first, C.c_uint32), _ptr(Rt, C.c_float), C.byref(n))
    if rc == ERR_TOO_FEW_EVENTS:
        return None
    _check(rc)
    return first[:n.value].copy(), Rt[:n.value].copy()


def alg2_subintervals(n_events, num_subintervals, process_method=2, camera=0):
    """The event ranges of Alg. 2's sub-intervals for one camera (dsi_alg2_subintervals): a list of num_subintervals
    (begin0, end0, begin1, end1); sub-interval k is events [begin0, end0) followed by [begin1, end1) -- the second range
    is empty unless camera 1 of process_method 5 wraps around the end of its events (process5.cpp:135-150)."""
    n = int(num_subintervals)
    if n < 1:
        raise DsiError(ERR_INVALID, "num_subintervals must be >= 1")
    out = np.empty(4 * n, np.uint64)
    _check(load_library().dsi_alg2_subintervals(int(n_events), n, int(process_method), int(camera),
                                                out.ctypes.data_as(C.POINTER(C.c_size_t))))
    return [tuple(int(v) for v in out[4 * k:4 * k + 4]) for k in range(n)]


def alg2_plan(num_subintervals, n_events, nx, camera_time=True):
    """The engine's Alg. 2 planner (dsi_alg2_plan): 'fused' when a window of n_events events (both cameras),
    num_subintervals sub-intervals and nx DSI columns goes through the DSI-less kernel, 'materialize' when through
    process_2 (more than 8 sub-intervals, rows too wide for the kernel, or past the measured break-even)."""
    ok = load_library().dsi_alg2_plan(int(num_subintervals), int(n_events), int(nx), 1 if camera_time else 0)
    return "fused" if ok == 1 else "materialize"


def packetize_strided(ts_view, trajectory, T_rv_w):
    """packetize() with the timestamps read where they lie: ts_view is a 1-D float64 view with any stride -- a field of
    a structured array of events, say -- and is not copied (dsi_packetize_strided: one timestamp per packet is read)."""
    if ts_view.dtype != np.float64 or ts_view.ndim != 1:
        raise ValueError("packetize_strided: a 1-D float64 view is required")
    n = int(ts_view.shape[0])
    stride = int(ts_view.strides[0]) if n else 8
    if stride < 8:
        raise ValueError("packetize_strided: stride %d is smaller than a timestamp" % stride)
    times, poses = trajectory
    times, poses = _arr(times, np.float64), _arr(poses, np.float64).reshape(-1, 7)
    T = _arr(T_rv_w, np.float64)
    cap = n // PACKET_SIZE + 1
    first = np.empty(cap, np.uint32)
    Rt = np.empty((cap, 12), np.float32)
    npk = C.c_size_t()
    rc = load_library().dsi_packetize_strided(C.c_void_p(ts_view.ctypes.data if n else 0), stride, n, _ptr(times, C.c_double),
                                              _ptr(poses, C.c_double), times.shape[0], _ptr(T, C.c_double),
                                              _ptr(first, C.c_uint32), _ptr(Rt, C.c_float), C.byref(npk))
    if rc == ERR_TOO_FEW_EVENTS:
        return None
    _check(rc)
    return first[:npk.value].copy(), Rt[:npk.value].copy()


def pose_at(trajectory, t):
    """LinearTrajectory::getPoseAt (trajectory.hpp:92-126); None when it returns false."""
    times, poses = trajectory
    times, poses = _arr(times, np.float64), _arr(poses, np.float64).reshape(-1, 7)
    out = np.empty(7, np.float64)
    rc = load_library().dsi_pose_at(_ptr(times, C.c_double), _ptr(poses, C.c_double), times.shape[0],
                                    float(t), _ptr(out, C.c_double))
    if rc == ERR_INVALID:
        return None
    _check(rc)
    return out
