"""ctypes binding of include/dvo_amd.h (one Python method per C entry point).

Fails loudly when the HIP library has not been built or when no HIP device is present:
there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

DVO_MAX_LEVELS = 8
DVO_NUM_ACC = 29
DVO_OK, DVO_ERR_INVALID, DVO_ERR_NO_DEVICE, DVO_ERR_HIP, DVO_ERR_STATE, DVO_ERR_NOMEM = range(6)
DVO_FLAG_FINAL_OUTPUTS = 1
DVO_FLAG_IDENTITY_START = 2
DVO_FLAG_NORMAL_MATRIX = 4

_HERE = os.path.dirname(os.path.abspath(__file__))

#: every symbol include/dvo_amd.h declares (checked by tests/test_capi_symbols.py)
C_ABI_SYMBOLS = [
    "dvo_params_default", "dvo_create", "dvo_create_batch", "dvo_destroy", "dvo_last_error",
    "dvo_num_pairs", "dvo_set_stream", "dvo_use_own_stream", "dvo_synchronize", "dvo_set_keep_warm", "dvo_set_keep_warm2", "dvo_set_intrinsics",
    "dvo_set_ref_level", "dvo_set_ref_level_pair", "dvo_set_now_level", "dvo_set_now_level_pair",
    "dvo_set_ref_level_device", "dvo_set_now_level_device", "dvo_set_ref_level_from_images",
    "dvo_run_iterations", "dvo_run_iterations_pair", "dvo_align_pyramid", "dvo_align_batch",
    "dvo_set_poses", "dvo_align_batch_enqueue", "dvo_get_poses", "dvo_get_poses_rows", "dvo_get_enqueue_counts", "dvo_get_level_report",
    "dvo_get_final_outputs", "dvo_get_level_normal_matrix", "dvo_eval_points", "dvo_accumulate", "dvo_device_se3_exp",
    "dvo_device_se3_log", "dvo_device_rotationize", "dvo_algorithmic_bytes", "dvo_point_iterations",
    "dvo_debug_stamps", "dvo_get_level_texel_mode", "dvo_get_level_exact_fallback", "dvo_get_level_energy_sweeps", "dvo_get_level_points4", "dvo_get_level_points4_direct", "dvo_get_level_final_fused", "dvo_get_level_ranks_in_lds", "dvo_now_prepare", "dvo_set_direct_compact", "dvo_host_alloc_mapped", "dvo_host_free_mapped", "dvo_get_now_compact_info", "dvo_get_now_compact_partial", "dvo_get_last_launch_shape", "dvo_replicate_pairs", "dvo_set_now_level_from_edges", "dvo_get_now_level", "dvo_iter_begin", "dvo_iter_accumulate", "dvo_iter_update", "dvo_iter_end",
    "dvo_align_pyramid_wide", "dvo_tiled_attach", "dvo_tiled_detach", "dvo_align_pyramid_tiled", "dvo_tiled_shard", "dvo_tiled_graph_replayed", "dvo_wide_packed_levels", "dvo_wide_team_levels",
    "dvo_get_ref_level", "dvo_frames_reserve", "dvo_frames_upload_pyramids", "dvo_frames_upload_cameras", "dvo_frames_upload_cameras_fmt", "dvo_frames_set_undistort", "dvo_undistort_map_host",
    "dvo_mask_levels_host", "dvo_frames_set_pair_mask", "dvo_frames_get_pair_mask_level", "dvo_tracker_set_stream_mask",
    "dvo_depth_register_host", "dvo_frames_set_pair_depth_rig", "dvo_frames_register_depth", "dvo_frames_get_registered_depth",
    "dvo_tracker_set_stream_depth_rig", "dvo_tracker_step_raw_depth",
    "dvo_photo_params_default", "dvo_photo_configure", "dvo_photo_set_ref", "dvo_photo_align", "dvo_photo_get_jacobian", "dvo_frames_as_now",
    "dvo_frames_as_ref", "dvo_frame_get_level", "dvo_frames_num_levels",
    "dvo_tracker_params_default", "dvo_tracker_create", "dvo_tracker_destroy", "dvo_tracker_last_error", "dvo_tracker_set_intrinsics",
    "dvo_tracker_reset_stream", "dvo_tracker_step", "dvo_tracker_step_fmt", "dvo_tracker_step_pyramids", "dvo_tracker_get_signals", "dvo_tracker_get_stats",
    "dvo_tracker_set_information", "dvo_tracker_get_information",
    "dvo_tracker_set_archive", "dvo_tracker_key_frame_id", "dvo_tracker_archive_info", "dvo_tracker_archive_get_points",
    "dvo_tracker_archive_stats", "dvo_tracker_score", "dvo_tracker_match",
    "dvo_tracker_set_places", "dvo_tracker_archive_get_descriptor", "dvo_tracker_query_places",
    "dvo_tracker_place_shifts", "dvo_tracker_place_guess",
    "dvo_tracker_verify_params_default", "dvo_tracker_verify",
    "dvo_archive_blob_info", "dvo_tracker_archive_export_size", "dvo_tracker_archive_export", "dvo_tracker_archive_import",
    "dvo_tracker_archive_origin",
    "dvo_tracker_set_views", "dvo_tracker_get_residue_histogram", "dvo_tracker_view_size", "dvo_tracker_get_view", "dvo_tracker_view_device",
    "dvo_tracker_context", "dvo_tracker_set_stream_intrinsics", "dvo_tracker_set_stream_undistort", "dvo_tracker_clear_stream_camera",
    "dvo_photo_streams_params_default", "dvo_photo_streams_create", "dvo_photo_streams_destroy", "dvo_photo_streams_last_error",
    "dvo_photo_streams_reset_stream", "dvo_photo_streams_step", "dvo_photo_streams_step_fmt", "dvo_photo_streams_get_jacobian", "dvo_photo_streams_get_stats",
    "dvo_photo_streams_context", "dvo_photo_streams_set_stream_intrinsics",
    "dvo_graph_params_default", "dvo_graph_solve_host", "dvo_graph_create", "dvo_graph_destroy", "dvo_graph_last_error", "dvo_graph_set",
    "dvo_graph_solve", "dvo_graph_get_poses", "dvo_graph_get_report", "dvo_graph_stats", "dvo_graph_information",
    "dvo_graph_marginals_host", "dvo_graph_marginals", "dvo_graph_edge_chi2",
    "dvo_tsdf_params_default", "dvo_tsdf_integrate_host", "dvo_tsdf_extract_host", "dvo_tsdf_create", "dvo_tsdf_destroy", "dvo_tsdf_last_error",
    "dvo_tsdf_set_volume", "dvo_tsdf_clear", "dvo_tsdf_integrate", "dvo_tsdf_extract_points", "dvo_tsdf_get_voxels", "dvo_tsdf_set_voxels",
    "dvo_tsdf_stats", "dvo_raycast_params_default", "dvo_raycast_host", "dvo_raycast_views", "dvo_mesh_host", "dvo_mesh_extract",
    "dvo_colour_integrate_host", "dvo_colour_raycast_host", "dvo_colour_mesh_host", "dvo_colour_enable", "dvo_colour_integrate",
    "dvo_colour_get_words", "dvo_colour_set_words", "dvo_colour_raycast_views", "dvo_colour_mesh_extract",
    "dvo_esdf_params_default", "dvo_esdf_host", "dvo_esdf_distances_host", "dvo_esdf_query_host", "dvo_esdf_enable", "dvo_esdf_update",
    "dvo_esdf_get_words", "dvo_esdf_get_distances", "dvo_esdf_query",
    "dvo_icp_params_default", "dvo_icp_align_host", "dvo_icp_create", "dvo_icp_destroy", "dvo_icp_last_error", "dvo_icp_align", "dvo_icp_stats",
    "dvo_icp_prepare_params_default", "dvo_icp_prepare_params_gaussian", "dvo_icp_prepare_host", "dvo_icp_prepare", "dvo_icp_align_gated_host",
    "dvo_icp_align_gated",
]

DVO_PIX_U8, DVO_PIX_U16, DVO_PIX_F32 = 0, 1, 2
DVO_LAYOUT_COL_MAJOR, DVO_LAYOUT_ROW_MAJOR = 0, 1
DVO_UPLOAD_ASYNC = 1
DVO_UPLOAD_DEPTH_RAW = 2
DVO_UPLOAD_DIRECT = 4
DVO_UPLOAD_DEVICE = 8
DVO_UPLOAD_MAPPED = 16
DVO_CAM_BGR8, DVO_CAM_RGB8, DVO_CAM_MONO8 = 0, 1, 2      # camera image formats (dvo_frames_upload_cameras_fmt)
DVO_DEPTH_F32, DVO_DEPTH_U16 = 0, 1                      # camera depth formats: float (metres / sensor units), 16-bit millimetres
DVO_VIEW_REPROJ_ON_DT, DVO_VIEW_RESIDUE_HEAT = 0, 1      # the tracker's views (dvo_tracker_get_view)
DVO_TRACKER_VIEW_LAUNCHES = 2                            # launches one rendering of the views adds to a step
DVO_VIEW_HISTOGRAM_BINS = 260
DVO_TRACKER_PLACE_STORE_LAUNCHES = 1                     # launches a store of new key frames adds while place descriptors are on
DVO_TRACKER_PLACE_QUERY_LAUNCHES = 2                     # launches of one dvo_tracker_query_places
DVO_TRACKER_PLACES_MAX_K = 32
DVO_TRACKER_PLACE_SHIFT_LAUNCHES = 1                     # launches of one dvo_tracker_place_shifts
DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS = 8
DVO_TRACKER_VERIFY_LAUNCHES = 1                          # launches of one dvo_tracker_verify
DVO_TRACKER_EXPORT_LAUNCHES = 1                          # launches of one dvo_tracker_archive_export
DVO_TRACKER_IMPORT_LAUNCHES = 2                          # launches of one dvo_tracker_archive_import
DVO_MASK_MAX_MARGIN = 8                                  # ignore masks: the largest dilation, in level pixels
DVO_FRAMES_MASK_LAUNCHES = 1                             # launches a chunk of an upload adds when one of its pairs has a mask
DVO_DEPTH_SPLAT_MAX = 8                                  # depth registration: the widest footprint of one depth pixel, in colour pixels
DVO_DEPTH_REGISTER_LAUNCHES = 2                          # launches of one dvo_frames_register_depth, whatever its count
DVO_GRAPH_EDGE_ROBUST = 1                                # pose graphs: the edge takes the Huber cost
DVO_GRAPH_MAX_NODES, DVO_GRAPH_MAX_EDGES = 4096, 32768   # per graph
DVO_GRAPH_CONVERGED, DVO_GRAPH_MAX_ITERATIONS, DVO_GRAPH_NUMERIC = 0, 1, 2      # dvo_graph_report.status
DVO_GRAPH_LAUNCHES = 1                                   # launches of one dvo_graph_solve, whatever its count
DVO_GRAPH_MARGINAL_MAX_NODES = 16                        # nodes of one marginals query
DVO_GRAPH_MARGINAL_LAUNCHES = 2                          # launches of one dvo_graph_marginals, whatever its count and m
DVO_TSDF_MAX_DIM = 1024                                  # depth fusion: voxels along one axis of a volume
DVO_TSDF_INTEGRATE_LAUNCHES = 1                          # launches of one dvo_tsdf_integrate, whatever its count
DVO_TSDF_EXTRACT_LAUNCHES = 3                            # launches of one dvo_tsdf_extract_points: count, scan, write
DVO_RAYCAST_LAUNCHES = 1                                 # launches of one dvo_raycast_views, whatever its count
DVO_RAYCAST_MAX_STEPS = 65536                            # ray casting: samples of one view's march
DVO_MESH_LAUNCHES = 4                                    # launches of one dvo_mesh_extract: count, scan, vertices, triangles
DVO_ESDF_UPDATE_LAUNCHES = 3                             # launches of one dvo_esdf_update, whatever its list: pass x, pass y, pass z
DVO_ESDF_SITES_SURFACE, DVO_ESDF_SITES_SURFACE_AND_UNKNOWN = 0, 1
DVO_ESDF_NO_SITE = 0xFFFFFF                              # d2 of every voxel of a volume without a site
DVO_ESDF_INSIDE, DVO_ESDF_UNKNOWN = 0x40000000, 0x80000000   # bits 30 and 31 of an ESDF word
DVO_ESDF_FOUND, DVO_ESDF_OUTSIDE, DVO_ESDF_NO_DISTANCE = 0, 1, 2   # dvo_esdf_sample.status
DVO_ICP_MAX_LEVELS, DVO_ICP_MAX_ITERATIONS = 4, 64       # frame-to-model alignment: levels of a call, sweeps of one level
DVO_ICP_MAX_PIXELS = 1 << 24                             # rows * cols of one dvo_icp_align
DVO_ICP_OK, DVO_ICP_FEW, DVO_ICP_DEGENERATE = 0, 1, 2    # dvo_icp_record.status
DVO_ICP_LAUNCHES_PER_SWEEP = 2                           # launches of each of a call's sum(iterations) + 1 sweeps
DVO_ICP_PREPARE_MAX_RADIUS, DVO_ICP_PREPARE_RANGE_BINS = 6, 256      # dvo_icp_prepare_params: the window is (2 radius + 1)^2; range bins
DVO_ICP_PREPARE_LAUNCHES = 2                             # launches of a dvo_icp_prepare: filter and normals (1 without normals)


class DvoImage(C.Structure):
    """Mirror of ``struct dvo_image``."""
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("dtype", C.c_int), ("layout", C.c_int)]


class DvoDepthRig(C.Structure):
    """dvo_depth_rig (include/dvo_amd.h, "depth registration"): how a sensor's depth camera sits beside its colour camera"""
    _fields_ = [("depth_rows", C.c_int), ("depth_cols", C.c_int), ("Kd4", C.c_double * 4), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("Kc4", C.c_double * 4), ("has_Dc5", C.c_int), ("Dc5", C.c_double * 5)]

    @classmethod
    def make(cls, depth_shape, Kd4, Kc4, R=None, t=None, Dc5=None) -> "DvoDepthRig":
        """depth_shape: (rows, cols) of the raw depth image; Kd4 / Kc4: fx, fy, cx, cy of the depth and the colour camera; R (3, 3)
        and t (3,) metres: X_colour = R X_depth + t (identity / zero when None); Dc5: k1, k2, p1, p2, k3 of the colour camera or None"""
        g = cls()
        g.depth_rows, g.depth_cols = int(depth_shape[0]), int(depth_shape[1])
        g.Kd4[:] = [float(v) for v in Kd4]
        g.Kc4[:] = [float(v) for v in Kc4]
        Rm = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
        g.R[:] = [float(v) for v in Rm.T.ravel()]                # column-major
        g.t[:] = [0.0] * 3 if t is None else [float(v) for v in np.asarray(t).ravel()]
        g.has_Dc5 = 0 if Dc5 is None else 1
        g.Dc5[:] = [0.0] * 5 if Dc5 is None else [float(v) for v in Dc5]
        return g


class DvoGraphEdge(C.Structure):
    """dvo_graph_edge (include/dvo_amd.h, "pose graphs"): Z ~ T_i^-1 T_j with information Omega"""
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("R", C.c_double * 9), ("t", C.c_double * 3), ("info", C.c_double * 36), ("flags", C.c_int)]

    @classmethod
    def make(cls, i: int, j: int, R, t, info, robust: bool = False) -> "DvoGraphEdge":
        """R (3, 3) and t (3,) of Z; info (6, 6), tangent order [translation, rotation]"""
        e = cls()
        e.i, e.j = int(i), int(j)
        e.R[:] = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(3, 3).T.ravel()]      # column-major
        e.t[:] = [float(v) for v in np.asarray(t, dtype=np.float64).ravel()]
        e.info[:] = [float(v) for v in np.asarray(info, dtype=np.float64).reshape(36)]
        e.flags = DVO_GRAPH_EDGE_ROBUST if robust else 0
        return e


class DvoGraphParams(C.Structure):
    """dvo_graph_params"""
    _fields_ = [("max_iterations", C.c_int), ("cg_max_iterations", C.c_int), ("lambda0", C.c_double), ("lambda_up", C.c_double),
                ("lambda_down", C.c_double), ("lambda_min", C.c_double), ("lambda_max", C.c_double), ("cg_tol", C.c_double),
                ("step_tol", C.c_double), ("cost_tol", C.c_double), ("huber_delta", C.c_double)]

    @classmethod
    def default(cls, **changes) -> "DvoGraphParams":
        p = cls()
        load_library().dvo_graph_params_default(C.byref(p))
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class DvoGraphReport(C.Structure):
    """dvo_graph_report"""
    _fields_ = [("cost0", C.c_double), ("cost", C.c_double), ("lambda_", C.c_double), ("max_step", C.c_double), ("iterations", C.c_int),
                ("accepted", C.c_int), ("cg_iterations", C.c_int), ("status", C.c_int)]


class DvoGraphMarginalReport(C.Structure):
    """dvo_graph_marginal_report"""
    _fields_ = [("worst_residual", C.c_double), ("cg_iterations", C.c_int), ("cg_iterations_max", C.c_int), ("status", C.c_int)]


class DvoTsdfVolume(C.Structure):
    """dvo_tsdf_volume (include/dvo_amd.h, "depth fusion"): nx * ny * nz voxels, voxel (0, 0, 0) centred at origin"""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("voxel_size", C.c_double), ("origin", C.c_double * 3), ("trunc", C.c_double)]

    @classmethod
    def make(cls, dims, voxel_size: float, origin, trunc: float) -> "DvoTsdfVolume":
        """dims: (nx, ny, nz); origin: the world position of the centre of voxel (0, 0, 0); voxel_size and trunc in metres"""
        v = cls()
        v.nx, v.ny, v.nz = (int(d) for d in dims)
        v.voxel_size, v.trunc = float(voxel_size), float(trunc)
        v.origin[:] = [float(o) for o in origin]
        return v

    @property
    def voxels(self) -> int:
        return self.nx * self.ny * self.nz


class DvoRaycastParams(C.Structure):
    """dvo_raycast_params (include/dvo_amd.h, "from the map back to depth")"""
    _fields_ = [("z_near", C.c_double), ("z_far", C.c_double), ("step_trunc", C.c_double), ("min_weight", C.c_int)]

    @classmethod
    def default(cls, **changes) -> "DvoRaycastParams":
        p = cls()
        load_library().dvo_raycast_params_default(C.byref(p))
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class DvoIcpParams(C.Structure):
    """dvo_icp_params (include/dvo_amd.h, "frame-to-model alignment")"""
    _fields_ = [("levels", C.c_int), ("iterations", C.c_int * DVO_ICP_MAX_LEVELS), ("z_near", C.c_double), ("z_far", C.c_double),
                ("dist_max", C.c_double), ("huber", C.c_double), ("stop_norm", C.c_double), ("min_pivot_ratio", C.c_double), ("min_count", C.c_int)]

    @classmethod
    def default(cls, **changes) -> "DvoIcpParams":
        """the defaults with `changes` applied; iterations: a sequence of up to DVO_ICP_MAX_LEVELS counts, the rest 0"""
        p = cls()
        load_library().dvo_icp_params_default(C.byref(p))
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            if k == "iterations":
                v = list(v)
                p.iterations[:] = [int(x) for x in v] + [0] * (DVO_ICP_MAX_LEVELS - len(v))
            else:
                setattr(p, k, v)
        return p

    def sweeps(self) -> int:
        """the sweeps of a call: the updates of the levels in use, and the record's"""
        return sum(self.iterations[l] for l in range(self.levels)) + 1


class DvoIcpPrepareParams(C.Structure):
    """dvo_icp_prepare_params (include/dvo_amd.h, "preparing a depth frame"): the bilateral filter's two weight tables and the normals'
    edge_max"""
    _fields_ = [("radius", C.c_int), ("reserved", C.c_int), ("range_scale", C.c_double), ("edge_max", C.c_double),
                ("range", C.c_ushort * DVO_ICP_PREPARE_RANGE_BINS), ("spatial", C.c_ubyte * (13 * 13))]

    @classmethod
    def default(cls) -> "DvoIcpPrepareParams":
        """gaussian(3, 2.0, 0.03, 0.05)"""
        p = cls()
        load_library().dvo_icp_prepare_params_default(C.byref(p))
        return p

    @classmethod
    def gaussian(cls, radius: int, sigma_s_px: float, sigma_r_m: float, edge_max: float) -> "DvoIcpPrepareParams":
        """the tables of a Gaussian pair: spatial sigma in pixels, range sigma in metres (the range table ends at three sigmas)"""
        p = cls()
        rc = load_library().dvo_icp_prepare_params_gaussian(int(radius), float(sigma_s_px), float(sigma_r_m), float(edge_max), C.byref(p))
        if rc != DVO_OK:
            raise DvoError(rc, "dvo_icp_prepare_params_gaussian refused its arguments")
        return p

    def spatial_table(self) -> np.ndarray:
        """the (2 radius + 1)^2 spatial weights in use, as a square array"""
        side = 2 * self.radius + 1
        return np.array(self.spatial[:side * side], dtype=np.uint8).reshape(side, side)


class DvoIcpRecord(C.Structure):
    """dvo_icp_record"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("count", C.c_int), ("reserved", C.c_int), ("sum_r2", C.c_double),
                ("rms", C.c_double), ("info", C.c_double * 36)]


#: dvo_icp_record as a numpy record: what icp_align_host and DvoIcp.align return, one per view
ICP_RECORD_DTYPE = np.dtype([("status", np.int32), ("iterations", np.int32), ("count", np.int32), ("reserved", np.int32), ("sum_r2", np.float64),
                             ("rms", np.float64), ("info", np.float64, (6, 6))])


class DvoTsdfParams(C.Structure):
    """dvo_tsdf_params"""
    _fields_ = [("z_near", C.c_double), ("z_far", C.c_double), ("max_weight", C.c_int)]

    @classmethod
    def default(cls, **changes) -> "DvoTsdfParams":
        p = cls()
        load_library().dvo_tsdf_params_default(C.byref(p))
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class DvoEsdfParams(C.Structure):
    """dvo_esdf_params (include/dvo_amd.h, "distance fields")"""
    _fields_ = [("min_weight", C.c_int), ("sites", C.c_int)]

    @classmethod
    def default(cls, **changes) -> "DvoEsdfParams":
        p = cls()
        load_library().dvo_esdf_params_default(C.byref(p))
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class DvoEsdfSample(C.Structure):
    """dvo_esdf_sample"""
    _fields_ = [("status", C.c_int), ("unknown", C.c_int), ("distance", C.c_double), ("gradient", C.c_double * 3)]


#: dvo_esdf_sample as a numpy record: what esdf_query_host and DvoTsdfVolumes.esdf_query return, one per point
ESDF_SAMPLE_DTYPE = np.dtype([("status", np.int32), ("unknown", np.int32), ("distance", np.float64), ("gradient", np.float64, (3,))])


class DvoParams(C.Structure):
    """Mirror of ``struct dvo_params`` (defaults = the literals of SolveDVO.cpp:21-33,653-773)."""
    _fields_ = [
        ("beta", C.c_double), ("precond_rot", C.c_double), ("reg_lambda", C.c_double),
        ("step_a", C.c_double), ("step_b", C.c_double),
        ("step_decay_after", C.c_int), ("step_decay_offset", C.c_int),
        ("trust_radius", C.c_float), ("psi_norm_stop", C.c_float),
        ("enable_rotationize", C.c_int), ("enable_l2_reg", C.c_int), ("interpolate_dt", C.c_int),
        ("block_threads", C.c_int), ("points_in_flight", C.c_int), ("engine_variant", C.c_int),
        ("lds_point_bytes", C.c_int), ("debug_alias_mod", C.c_int),
        ("canny_threshold1", C.c_int), ("canny_threshold2", C.c_int), ("team_size", C.c_int),
    ]


class DvoTrackerScoreRecord(C.Structure):
    """Mirror of ``struct dvo_tracker_score_record`` (dvo_tracker_score / dvo_tracker_match)."""
    _fields_ = [("H36", C.c_double * 36), ("g6", C.c_double * 6), ("sum_eps2", C.c_double), ("n_points", C.c_int), ("n_visible", C.c_int)]


class DvoTrackerPlace(C.Structure):
    """Mirror of ``struct dvo_tracker_place`` (dvo_tracker_query_places)."""
    _fields_ = [("key_id", C.c_longlong), ("frame", C.c_longlong), ("stream", C.c_int), ("distance", C.c_uint)]


class DvoTrackerPlaceShift(C.Structure):
    """Mirror of ``struct dvo_tracker_place_shift`` (dvo_tracker_place_shifts)."""
    _fields_ = [("dy", C.c_int), ("dx", C.c_int), ("sad", C.c_uint), ("sad_zero", C.c_uint), ("sad_second", C.c_uint), ("area", C.c_int)]


class DvoTrackerVerifyParams(C.Structure):
    """Mirror of ``struct dvo_tracker_verify_params`` (defaults: dvo_tracker_verify_params_default)."""
    _fields_ = [("tol_mm", C.c_float), ("tol_rel", C.c_float), ("min_depth_mm", C.c_float), ("max_depth_mm", C.c_float)]


class DvoTrackerVerifyRecord(C.Structure):
    """Mirror of ``struct dvo_tracker_verify_record`` (dvo_tracker_verify)."""
    _fields_ = [("n_points", C.c_int), ("n_visible", C.c_int), ("n_depth", C.c_int), ("n_agree", C.c_int), ("n_front", C.c_int),
                ("n_behind", C.c_int), ("sum_abs_q4", C.c_ulonglong)]


class DvoArchiveBlobInfo(C.Structure):
    """Mirror of ``struct dvo_archive_blob_info`` (dvo_archive_blob_info)."""
    _fields_ = [("version", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("n_levels", C.c_int), ("first_shift", C.c_int),
                ("places_level", C.c_int), ("D", C.c_int), ("n_key_frames", C.c_int), ("total_bytes", C.c_ulonglong)]


def depth_verdict(record, min_agree_ratio: float, max_front_ratio: float, min_depth_points: int) -> bool:
    """dvo_amd::depthVerdict: whether a record of DvoTracker.verify() (a dict, or a DvoTrackerVerifyRecord) supports its candidate --
    enough points with a measurement, enough of them agreeing, few enough in front of the measured surface"""
    get = record.__getitem__ if isinstance(record, dict) else (lambda k: getattr(record, k))
    n_depth, n_agree, n_front = int(get("n_depth")), int(get("n_agree")), int(get("n_front"))
    return bool(n_depth >= min_depth_points and n_agree >= min_agree_ratio * n_depth and n_front <= max_front_ratio * n_depth)


class DvoTrackerParams(C.Structure):
    """Mirror of ``struct dvo_tracker_params`` (defaults: dvo_tracker_params_default)."""
    _fields_ = [
        ("iters", C.c_int * DVO_MAX_LEVELS), ("key_frame_every", C.c_int), ("adaptive", C.c_int),
        ("laplacian_b_thresh", C.c_float), ("visible_ratio_thresh", C.c_float), ("min_points", C.c_int),
        ("rows", C.c_int), ("cols", C.c_int), ("n_levels", C.c_int), ("first_shift", C.c_int),
        ("points_capacity", C.c_int * DVO_MAX_LEVELS),
    ]


class DvoPhotoParams(C.Structure):
    """Mirror of ``struct dvo_photo_params`` (defaults = the constants of RGBDOdometry.cpp:32-34, :545, :556)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("gradient_threshold", C.c_int), ("max_jacobian_size", C.c_int), ("min_required_pts", C.c_int),
                ("iterations", C.c_int), ("eps_norm_stop", C.c_double), ("fixed", C.c_int), ("reserved", C.c_int)]


class DvoPhotoStreamsParams(C.Structure):
    """Mirror of ``struct dvo_photo_streams_params`` (defaults: dvo_photo_streams_params_default)."""
    _fields_ = [("photo", DvoPhotoParams), ("ref_every", C.c_int), ("first_level", C.c_int), ("n_run", C.c_int),
                ("levels", C.c_int * DVO_MAX_LEVELS), ("rows", C.c_int), ("cols", C.c_int)]


class RcclComm:
    """A raw RCCL communicator made through ctypes (tests / tools of the C-driven tiled mode; a C++ node creates its
    ncclComm_t itself).  unique_id: 128 bytes from RcclComm.unique_id() of rank 0, distributed by the launcher."""
    RCCL = "/opt/rocm/lib/librccl.so.1"

    class _Id(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    @classmethod
    def _lib(cls):
        import torch  # noqa: F401  (one HIP runtime per process, see load_library)
        lib = C.CDLL(cls.RCCL, mode=C.RTLD_GLOBAL)
        lib.ncclGetUniqueId.argtypes = [C.POINTER(cls._Id)]
        lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, cls._Id, C.c_int]
        lib.ncclCommDestroy.argtypes = [C.c_void_p]
        return lib

    @classmethod
    def unique_id(cls) -> bytes:
        uid = cls._Id()
        rc = cls._lib().ncclGetUniqueId(C.byref(uid))
        if rc != 0:
            raise RuntimeError("ncclGetUniqueId failed: %d" % rc)
        return bytes(uid)

    def __init__(self, unique_id: bytes, rank: int, world: int):
        self.lib = self._lib()
        uid = self._Id.from_buffer_copy(unique_id)
        self.comm = C.c_void_p()
        rc = self.lib.ncclCommInitRank(C.byref(self.comm), world, uid, rank)
        if rc != 0:
            raise RuntimeError("ncclCommInitRank failed: %d" % rc)
        self.comm = self.comm.value
        self.rank, self.world = rank, world

    def count(self) -> int:
        """ncclCommCount: the number of ranks RCCL itself says this communicator has"""
        n = C.c_int(0)
        self.lib.ncclCommCount.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        rc = self.lib.ncclCommCount(C.c_void_p(self.comm), C.byref(n))
        if rc != 0:
            raise RuntimeError("ncclCommCount failed: %d" % rc)
        return n.value

    def close(self):
        if self.comm:
            self.lib.ncclCommDestroy(C.c_void_p(self.comm))
            self.comm = None


def _mapped_ok(flags: int, passed, given):
    """DVO_UPLOAD_MAPPED hands the GPU the caller's (pinned, mapped) buffer itself: a silent dtype / layout conversion here would
    hand it a pageable copy instead"""
    if flags & DVO_UPLOAD_MAPPED and not (isinstance(given, np.ndarray) and np.shares_memory(passed, given)):
        raise ValueError("DVO_UPLOAD_MAPPED needs the images as contiguous numpy views of pinned memory in their final dtype "
                         "(uint8 BGR / grey, float32 or uint16 depth): this one would have been copied")


def _camera_arrays(images, depths, rgb: bool, flags: int):
    """Camera frames as contiguous arrays in the format the arrays themselves name: a 2-D uint8 image is mono8, a (rows, cols, 3) one
    BGR8 (RGB8 with rgb=True); uint16 depth is 16-bit millimetres, any other depth dtype is taken as float32.  All frames of a call
    share one format.  Returns (image_format, image arrays, depth_format, depth arrays or None)"""
    il = [np.ascontiguousarray(b, dtype=np.uint8) for b in images]
    for b, src in zip(il, images):
        _mapped_ok(flags, b, src)
    mono = bool(il) and il[0].ndim == 2
    if any((b.ndim == 2) != mono or (b.ndim != 2 and (b.ndim != 3 or b.shape[2] != 3)) for b in il):
        raise ValueError("camera images must all be (rows, cols) mono8 or all (rows, cols, 3) BGR8 / RGB8")
    if mono and rgb:
        raise ValueError("rgb=True needs three-channel images")
    ifmt = DVO_CAM_MONO8 if mono else (DVO_CAM_RGB8 if rgb else DVO_CAM_BGR8)
    if depths is None:
        return ifmt, il, DVO_DEPTH_F32, None
    u16 = bool(len(depths)) and all(isinstance(d, np.ndarray) and d.dtype == np.uint16 for d in depths)
    dl = [np.ascontiguousarray(d, dtype=np.uint16 if u16 else np.float32) for d in depths]
    for d, src in zip(dl, depths):
        _mapped_ok(flags, d, src)
    return ifmt, il, DVO_DEPTH_U16 if u16 else DVO_DEPTH_F32, dl


class MappedHostArray:
    """A numpy array over pinned host memory the GPU can address (dvo_host_alloc_mapped): what DVO_UPLOAD_MAPPED wants, for
    callers without torch.  Keep the object alive while the array is in use; free() or garbage collection releases it."""

    def __init__(self, shape, dtype):
        lib = load_library()
        self._lib = lib
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = lib.dvo_host_alloc_mapped(self.nbytes)
        if not self._p:
            raise MemoryError("dvo_host_alloc_mapped(%d) failed" % self.nbytes)
        buf = (C.c_ubyte * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            self._lib.dvo_host_free_mapped(C.c_void_p(self._p))
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DvoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dvo error {code}: {msg}")
        self.code = code


def library_path() -> str:
    return os.path.join(_HERE, "lib", "libdvo_amd.so")


_lib = None


def _build_native():
    """make -C rgbd_odometry_amd/csrc: builds lib/libdvo_amd.so (gfx950), lib/libdvo_synth.so and the helper binaries.

    Serialised across processes with a file lock (N ranks of one torch.distributed launch on a fresh checkout would
    otherwise all run make at once and could dlopen a half-written library): whoever gets the lock builds, the others
    wait and find the library present.  A failed build raises with make's own output."""
    import fcntl
    import subprocess
    csrc = os.path.join(_HERE, "csrc")
    with open(os.path.join(csrc, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if os.path.exists(library_path()):
                return
            r = subprocess.run(["make", "-C", csrc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                raise RuntimeError("building the HIP extension failed (make -C %s):\n%s" % (csrc, r.stdout[-4000:]))
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def load_library() -> C.CDLL:
    """Load lib/libdvo_amd.so; raise if it is missing (build with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch's wheel bundles its own libamdhip64 (SONAME
    # libamdhip64.so.7, same as /opt/rocm's).  Importing torch FIRST makes the dynamic loader bind
    # libdvo_amd.so to that already-loaded copy, so torch streams / device pointers / RCCL and this
    # library share one runtime.  Loading in the other order would put two runtimes in the process.
    if os.environ.get("DVO_NO_TORCH", "0") != "1":
        import torch  # noqa: F401
    path = library_path()
    if not os.path.exists(path):
        _build_native()           # a fresh checkout: compile in-tree (hipcc), never fall back to anything else
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C rgbd_odometry_amd/csrc)")
    lib = C.CDLL(path)
    vp, ip, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
    i, f = C.c_int, C.c_float
    sig = {
        "dvo_params_default": [C.POINTER(DvoParams)],
        "dvo_create": [C.POINTER(DvoParams), C.POINTER(vp)],
        "dvo_create_batch": [C.POINTER(DvoParams), i, C.POINTER(vp)],
        "dvo_destroy": [vp],
        "dvo_num_pairs": [vp],
        "dvo_set_stream": [vp, vp],
        "dvo_use_own_stream": [vp],
        "dvo_synchronize": [vp],
        "dvo_set_keep_warm": [vp, i],
        "dvo_set_keep_warm2": [vp, i, i],
        "dvo_set_intrinsics": [vp, f, f, f, f],
        "dvo_set_ref_level": [vp, i, vp, i],
        "dvo_set_ref_level_pair": [vp, i, i, vp, i],
        "dvo_set_now_level": [vp, i, vp, vp, vp, i, i],
        "dvo_set_now_level_pair": [vp, i, i, vp, vp, vp, i, i],
        "dvo_set_ref_level_device": [vp, i, i, vp, i],
        "dvo_set_now_level_device": [vp, i, i, vp, vp, vp, i, i],
        "dvo_set_ref_level_from_images": [vp, i, i, vp, vp, i, i, vp, vp, i, ip],
        "dvo_run_iterations": [vp, i, i, vp, vp, vp, vp, vp, ip, fp],
        "dvo_run_iterations_pair": [vp, i, i, i, vp, vp, vp, vp, vp, ip, fp],
        "dvo_align_pyramid": [vp, i, ip, i, vp, vp],
        "dvo_align_batch": [vp, i, i, i, ip, i, vp, vp],
        "dvo_set_poses": [vp, i, i, vp, vp],
        "dvo_align_batch_enqueue": [vp, i, i, i, ip, i],
        "dvo_get_poses": [vp, i, i, vp, vp],
        "dvo_get_poses_rows": [vp, i, i, vp, vp],
        "dvo_get_enqueue_counts": [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)],
        "dvo_get_level_report": [vp, i, i, vp, i, ip, fp],
        "dvo_get_final_outputs": [vp, i, vp, vp, i, ip],
        "dvo_get_level_normal_matrix": [vp, i, i, i, vp],
        "dvo_eval_points": [vp, i, i, vp, vp, vp, vp, vp, vp, vp],
        "dvo_accumulate": [vp, i, i, vp, vp, vp],
        "dvo_device_se3_exp": [vp, vp, vp, vp],
        "dvo_device_se3_log": [vp, vp, vp, vp],
        "dvo_device_rotationize": [vp, vp],
        "dvo_debug_stamps": [vp, i, vp],
        "dvo_get_level_texel_mode": [vp, i, i, ip],
        "dvo_get_level_exact_fallback": [vp, i, i, ip],
        "dvo_get_level_energy_sweeps": [vp, i, i, ip],
        "dvo_get_level_points4": [vp, i, i, ip],
        "dvo_get_level_points4_direct": [vp, i, i, ip],
        "dvo_get_level_final_fused": [vp, i, i, ip],
        "dvo_get_level_ranks_in_lds": [vp, i, i, ip],
        "dvo_now_prepare": [vp, i, i],
        "dvo_get_last_launch_shape": [vp, ip, ip, ip],
        "dvo_get_now_compact_info": [vp, i, i, ip],
        "dvo_get_now_compact_partial": [vp, i, i, ip],
        "dvo_set_direct_compact": [vp, i],
        "dvo_host_alloc_mapped": [C.c_size_t],
        "dvo_host_free_mapped": [vp],
        "dvo_replicate_pairs": [vp, i, i, i],
        "dvo_set_now_level_from_edges": [vp, i, i, vp, i, i],
        "dvo_get_now_level": [vp, i, i, vp, vp, vp],
        "dvo_iter_begin": [vp, i, i, i, vp, vp],
        "dvo_iter_accumulate": [vp, i, i, i, i, vp],
        "dvo_iter_update": [vp, i, i, i, i, vp],
        "dvo_iter_end": [vp, i, i, vp, vp, vp, ip, fp],
        "dvo_align_pyramid_wide": [vp, i, i, ip, i, vp, vp],
        "dvo_frames_set_undistort": [vp, i, i, vp, vp],
        "dvo_undistort_map_host": [i, i, vp, vp, vp, vp],
        "dvo_mask_levels_host": [i, i, vp, i, i, i, C.POINTER(vp), ip, ip],
        "dvo_frames_set_pair_mask": [vp, i, i, i, vp, i, i, i],
        "dvo_frames_get_pair_mask_level": [vp, i, i, vp, i, ip, ip],
        "dvo_tracker_set_stream_mask": [vp, i, vp, i],
        "dvo_depth_register_host": [C.POINTER(DvoDepthRig), vp, i, i, i, vp],
        "dvo_frames_set_pair_depth_rig": [vp, i, C.POINTER(DvoDepthRig), i, i],
        "dvo_frames_register_depth": [vp, i, i, C.POINTER(vp), i, i, C.POINTER(vp)],
        "dvo_frames_get_registered_depth": [vp, i, vp, i, ip, ip],
        "dvo_tracker_set_stream_depth_rig": [vp, i, C.POINTER(DvoDepthRig)],
        "dvo_tracker_step_raw_depth": [vp, i, ip, C.POINTER(vp), i, C.POINTER(vp), i, i, i, i, vp, vp, ip],
        "dvo_photo_params_default": [C.POINTER(DvoPhotoParams)],
        "dvo_photo_configure": [vp, C.POINTER(DvoPhotoParams)],
        "dvo_photo_set_ref": [vp, i, i, ip],
        "dvo_photo_align": [vp, i, ip, i, vp, vp, ip],
        "dvo_photo_get_jacobian": [vp, i, vp, vp, vp, i, vp, ip],
        "dvo_tiled_attach": [vp, vp, i, i, C.c_char_p],
        "dvo_tiled_detach": [vp],
        "dvo_align_pyramid_tiled": [vp, i, i, ip, i, vp, vp],
        "dvo_tiled_shard": [vp, i, i, ip, ip],
        "dvo_tiled_graph_replayed": [vp, ip],
        "dvo_wide_packed_levels": [vp, ip, ip],
        "dvo_wide_team_levels": [vp, ip],
        "dvo_get_ref_level": [vp, i, i, vp, i, ip],
        "dvo_frames_reserve": [vp, i],
        "dvo_frames_upload_pyramids": [vp, i, i, i, C.POINTER(DvoImage), C.POINTER(DvoImage), i, i],
        "dvo_frames_upload_cameras": [vp, i, i, C.POINTER(vp), C.POINTER(vp), i, i, i, i, i, i],
        "dvo_frames_upload_cameras_fmt": [vp, i, i, C.POINTER(vp), i, C.POINTER(vp), i, i, i, i, i, i, i],
        "dvo_frames_as_now": [vp, i, i, i],
        "dvo_frames_as_ref": [vp, i, i, i, ip],
        "dvo_frame_get_level": [vp, i, i, ip, ip, vp, vp, vp, ip],
        "dvo_frames_num_levels": [vp],
        "dvo_algorithmic_bytes": [vp, i, i, ip, i, C.POINTER(C.c_uint64)],
        "dvo_point_iterations": [vp, i, i, ip, C.POINTER(C.c_uint64)],
        "dvo_tracker_params_default": [C.POINTER(DvoTrackerParams)],
        "dvo_tracker_create": [C.POINTER(DvoParams), i, C.POINTER(DvoTrackerParams), C.POINTER(vp)],
        "dvo_tracker_destroy": [vp],
        "dvo_tracker_set_intrinsics": [vp, f, f, f, f],
        "dvo_tracker_reset_stream": [vp, i],
        "dvo_tracker_set_stream_intrinsics": [vp, i, f, f, f, f],
        "dvo_tracker_set_stream_undistort": [vp, i, vp, vp],
        "dvo_tracker_clear_stream_camera": [vp, i],
        "dvo_tracker_step": [vp, i, ip, C.POINTER(vp), C.POINTER(vp), i, i, i, vp, vp, ip],
        "dvo_tracker_step_fmt": [vp, i, ip, C.POINTER(vp), i, C.POINTER(vp), i, i, i, i, vp, vp, ip],
        "dvo_tracker_step_pyramids": [vp, i, ip, C.POINTER(DvoImage), C.POINTER(DvoImage), i, vp, vp, ip],
        "dvo_tracker_get_signals": [vp, i, fp, fp, ip],
        "dvo_tracker_set_information": [vp, i],
        "dvo_tracker_get_information": [vp, i, vp, vp, C.POINTER(C.c_double), ip, ip],
        "dvo_tracker_set_archive": [vp, i, i, ip],
        "dvo_tracker_key_frame_id": [vp, i, C.POINTER(C.c_longlong)],
        "dvo_tracker_archive_info": [vp, C.c_longlong, ip, C.POINTER(C.c_longlong), ip],
        "dvo_tracker_archive_get_points": [vp, C.c_longlong, i, vp, i, ip],
        "dvo_tracker_archive_stats": [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), ip, ip],
        "dvo_tracker_score": [vp, i, ip, C.POINTER(C.c_longlong), i, vp, vp, C.POINTER(DvoTrackerScoreRecord)],
        "dvo_tracker_match": [vp, i, ip, C.POINTER(C.c_longlong), vp, vp, vp, vp, C.POINTER(DvoTrackerScoreRecord)],
        "dvo_tracker_set_places": [vp, i],
        "dvo_tracker_archive_get_descriptor": [vp, C.c_longlong, C.POINTER(C.c_ubyte), i, ip],
        "dvo_tracker_query_places": [vp, i, ip, i, C.c_longlong, C.POINTER(DvoTrackerPlace), ip],
        "dvo_tracker_place_shifts": [vp, i, ip, C.POINTER(C.c_longlong), i, C.POINTER(DvoTrackerPlaceShift)],
        "dvo_tracker_place_guess": [vp, i, i, i, vp, vp],
        "dvo_tracker_verify_params_default": [C.POINTER(DvoTrackerVerifyParams)],
        "dvo_tracker_verify": [vp, i, ip, C.POINTER(C.c_longlong), i, vp, vp, C.POINTER(DvoTrackerVerifyParams),
                               C.POINTER(DvoTrackerVerifyRecord)],
        "dvo_archive_blob_info": [vp, C.c_size_t, C.POINTER(DvoArchiveBlobInfo)],
        "dvo_tracker_archive_export_size": [vp, i, C.POINTER(C.c_longlong), C.POINTER(C.c_size_t)],
        "dvo_tracker_archive_export": [vp, i, C.POINTER(C.c_longlong), vp, C.c_size_t, C.POINTER(C.c_size_t)],
        "dvo_tracker_archive_import": [vp, vp, C.c_size_t, C.POINTER(C.c_longlong), i, ip],
        "dvo_tracker_archive_origin": [vp, C.c_longlong, C.POINTER(C.c_longlong), ip, C.POINTER(C.c_longlong)],
        "dvo_tracker_set_views": [vp, i],
        "dvo_tracker_get_residue_histogram": [vp, i, vp, ip, ip],
        "dvo_tracker_view_size": [vp, ip, ip, ip],
        "dvo_tracker_get_view": [vp, i, i, vp],
        "dvo_tracker_view_device": [vp, i, i, C.POINTER(vp)],
        "dvo_tracker_get_stats": [vp, ip, ip, ip, ip, ip],
        "dvo_photo_streams_params_default": [C.POINTER(DvoPhotoStreamsParams)],
        "dvo_photo_streams_create": [C.POINTER(DvoPhotoStreamsParams), i, C.POINTER(vp)],
        "dvo_photo_streams_destroy": [vp],
        "dvo_photo_streams_reset_stream": [vp, i],
        "dvo_photo_streams_set_stream_intrinsics": [vp, i, C.c_double, C.c_double, C.c_double, C.c_double],
        "dvo_photo_streams_step": [vp, i, ip, C.POINTER(vp), C.POINTER(vp), i, i, i, vp, vp, ip, ip],
        "dvo_photo_streams_step_fmt": [vp, i, ip, C.POINTER(vp), i, C.POINTER(vp), i, i, i, i, vp, vp, ip, ip],
        "dvo_photo_streams_get_jacobian": [vp, i, i, vp, vp, vp, i, vp, ip],
        "dvo_photo_streams_get_stats": [vp, ip, ip, ip, ip, ip],
        "dvo_graph_params_default": [C.POINTER(DvoGraphParams)],
        "dvo_graph_solve_host": [C.POINTER(DvoGraphParams), i, vp, vp, i, C.POINTER(DvoGraphEdge), C.POINTER(DvoGraphReport), vp, i],
        "dvo_graph_create": [i, i, i, C.POINTER(vp)],
        "dvo_graph_destroy": [vp],
        "dvo_graph_set": [vp, i, i, vp, vp, i, C.POINTER(DvoGraphEdge)],
        "dvo_graph_solve": [vp, C.POINTER(DvoGraphParams), i, ip],
        "dvo_graph_get_poses": [vp, i, vp],
        "dvo_graph_get_report": [vp, i, C.POINTER(DvoGraphReport), vp, i],
        "dvo_graph_stats": [vp, ip, ip],
        "dvo_graph_information": [vp, C.c_double, i, vp],
        "dvo_graph_marginals_host": [C.POINTER(DvoGraphParams), i, vp, vp, i, C.POINTER(DvoGraphEdge), i, ip, vp, C.POINTER(DvoGraphMarginalReport)],
        "dvo_graph_marginals": [vp, C.POINTER(DvoGraphParams), i, ip, i, ip, vp, C.POINTER(DvoGraphMarginalReport)],
        "dvo_graph_edge_chi2": [vp, vp, vp, C.POINTER(DvoGraphEdge), vp, vp, C.POINTER(C.c_double)],
        "dvo_tsdf_params_default": [C.POINTER(DvoTsdfParams)],
        "dvo_tsdf_integrate_host": [C.POINTER(DvoTsdfVolume), vp, C.POINTER(DvoTsdfParams), i, C.POINTER(vp), i, i, i, vp, vp],
        "dvo_tsdf_extract_host": [C.POINTER(DvoTsdfVolume), vp, i, vp, C.c_longlong, C.POINTER(C.c_longlong)],
        "dvo_tsdf_create": [i, C.c_longlong, C.POINTER(vp)],
        "dvo_tsdf_destroy": [vp],
        "dvo_tsdf_set_volume": [vp, i, C.POINTER(DvoTsdfVolume)],
        "dvo_tsdf_clear": [vp, i],
        "dvo_tsdf_integrate": [vp, C.POINTER(DvoTsdfParams), i, ip, C.POINTER(vp), i, i, i, vp, vp, i],
        "dvo_tsdf_extract_points": [vp, i, i, vp, C.c_longlong, C.POINTER(C.c_longlong)],
        "dvo_tsdf_get_voxels": [vp, i, vp],
        "dvo_tsdf_set_voxels": [vp, i, vp],
        "dvo_tsdf_stats": [vp, ip, ip],
        "dvo_raycast_params_default": [C.POINTER(DvoRaycastParams)],
        "dvo_raycast_host": [C.POINTER(DvoTsdfVolume), vp, C.POINTER(DvoRaycastParams), i, i, i, i, vp, vp, C.POINTER(vp), C.POINTER(vp)],
        "dvo_raycast_views": [vp, C.POINTER(DvoRaycastParams), i, ip, i, i, i, vp, vp, C.POINTER(vp), C.POINTER(vp), i],
        "dvo_mesh_host": [C.POINTER(DvoTsdfVolume), vp, i, vp, C.c_longlong, vp, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)],
        "dvo_mesh_extract": [vp, i, i, vp, C.c_longlong, vp, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), i],
        "dvo_colour_integrate_host": [C.POINTER(DvoTsdfVolume), vp, vp, C.POINTER(DvoTsdfParams), i, C.POINTER(vp), i, C.POINTER(vp), i, i, i, vp, vp],
        "dvo_colour_raycast_host": [C.POINTER(DvoTsdfVolume), vp, vp, C.POINTER(DvoRaycastParams), i, i, i, i, vp, vp, C.POINTER(vp), C.POINTER(vp),
                                    C.POINTER(vp), i],
        "dvo_colour_mesh_host": [C.POINTER(DvoTsdfVolume), vp, vp, i, vp, vp, C.c_longlong, vp, C.c_longlong, C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_longlong)],
        "dvo_colour_enable": [vp],
        "dvo_colour_integrate": [vp, C.POINTER(DvoTsdfParams), i, ip, C.POINTER(vp), i, C.POINTER(vp), i, i, i, vp, vp, i],
        "dvo_colour_get_words": [vp, i, vp],
        "dvo_colour_set_words": [vp, i, vp],
        "dvo_colour_raycast_views": [vp, C.POINTER(DvoRaycastParams), i, ip, i, i, i, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, i],
        "dvo_colour_mesh_extract": [vp, i, i, vp, vp, C.c_longlong, vp, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), i],
        "dvo_esdf_params_default": [C.POINTER(DvoEsdfParams)],
        "dvo_esdf_host": [C.POINTER(DvoTsdfVolume), vp, C.POINTER(DvoEsdfParams), vp],
        "dvo_esdf_distances_host": [C.POINTER(DvoTsdfVolume), vp, vp],
        "dvo_esdf_query_host": [C.POINTER(DvoTsdfVolume), vp, i, vp, vp],
        "dvo_esdf_enable": [vp],
        "dvo_esdf_update": [vp, C.POINTER(DvoEsdfParams), i, ip],
        "dvo_esdf_get_words": [vp, i, vp],
        "dvo_esdf_get_distances": [vp, i, i, i, vp, i],
        "dvo_esdf_query": [vp, i, i, vp, vp, i],
        "dvo_icp_params_default": [C.POINTER(DvoIcpParams)],
        "dvo_icp_align_host": [C.POINTER(DvoIcpParams), i, i, i, i, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp],
        "dvo_icp_create": [i, C.POINTER(vp)],
        "dvo_icp_destroy": [vp],
        "dvo_icp_align": [vp, C.POINTER(DvoIcpParams), i, i, i, i, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp, i],
        "dvo_icp_stats": [vp, ip, ip],
        "dvo_icp_prepare_params_default": [C.POINTER(DvoIcpPrepareParams)],
        "dvo_icp_prepare_params_gaussian": [i, C.c_double, C.c_double, C.c_double, C.POINTER(DvoIcpPrepareParams)],
        "dvo_icp_prepare_host": [C.POINTER(DvoIcpPrepareParams), i, i, i, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
        "dvo_icp_prepare": [vp, C.POINTER(DvoIcpPrepareParams), i, i, i, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i],
        "dvo_icp_align_gated_host": [C.POINTER(DvoIcpParams), i, i, i, i, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(vp),
                                     C.c_double, vp, vp],
        "dvo_icp_align_gated": [vp, C.POINTER(DvoIcpParams), i, i, i, i, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(vp),
                                C.c_double, vp, vp, i],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.dvo_last_error.argtypes = [vp]
    lib.dvo_last_error.restype = C.c_char_p
    lib.dvo_tracker_last_error.argtypes = [vp]
    lib.dvo_tracker_last_error.restype = C.c_char_p
    lib.dvo_tracker_context.argtypes = [vp]
    lib.dvo_tracker_context.restype = C.c_void_p
    lib.dvo_photo_streams_last_error.argtypes = [vp]
    lib.dvo_photo_streams_last_error.restype = C.c_char_p
    lib.dvo_photo_streams_context.argtypes = [vp]
    lib.dvo_photo_streams_context.restype = C.c_void_p
    lib.dvo_graph_last_error.argtypes = [vp]
    lib.dvo_graph_last_error.restype = C.c_char_p
    lib.dvo_tsdf_last_error.argtypes = [vp]
    lib.dvo_tsdf_last_error.restype = C.c_char_p
    lib.dvo_icp_last_error.argtypes = [vp]
    lib.dvo_icp_last_error.restype = C.c_char_p
    lib.dvo_host_alloc_mapped.restype = C.c_void_p
    lib.dvo_host_free_mapped.restype = None
    _lib = lib
    return lib


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mask_bytes(mask) -> np.ndarray:
    """a mask as the C ABI takes it: (rows, cols) bytes, row-major, non-zero = ignore (bool arrays are welcome)"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("a mask is a (rows, cols) array")
    return np.ascontiguousarray(m != 0 if m.dtype != np.uint8 else m, dtype=np.uint8)


def mask_levels_host(mask, n_levels: int, first_shift: int, margin: int = 2):
    """The keep planes of an ignore mask on the host (include/dvo_amd.h, "ignore masks": the definition; no device needed): a list
    over levels of (rows_l, cols_l) uint8 arrays, 0 where the level pixel is dropped and 255 where it is kept."""
    lib = load_library()
    m = _mask_bytes(mask)
    rows, cols = m.shape
    n = max(int(n_levels), 0)
    planes = [np.zeros(max(rows * cols, 1), np.uint8) for _ in range(n)]         # a level is never larger than the image
    keep = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in planes])
    lr, lc = (C.c_int * DVO_MAX_LEVELS)(), (C.c_int * DVO_MAX_LEVELS)()
    rc = lib.dvo_mask_levels_host(rows, cols, _ptr(m), n_levels, first_shift, margin, keep, lr, lc) if n <= DVO_MAX_LEVELS else \
        lib.dvo_mask_levels_host(rows, cols, _ptr(m), n_levels, first_shift, margin, None, None, None)
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_mask_levels_host refused its arguments")
    return [planes[l][:lr[l] * lc[l]].reshape(lc[l], lr[l]).T.copy() for l in range(n)]


def _raw_depth(depth, rig: "DvoDepthRig"):
    """a raw depth image as the C ABI takes it: uint16 millimetres stay, everything else becomes float32 metres; (format, array)"""
    d = np.asarray(depth)
    d = np.ascontiguousarray(d, dtype=np.uint16 if d.dtype == np.uint16 else np.float32)
    if d.shape != (rig.depth_rows, rig.depth_cols):
        raise ValueError("the raw depth image must have the rig's depth_rows x depth_cols")
    return (DVO_DEPTH_U16 if d.dtype == np.uint16 else DVO_DEPTH_F32), d


def depth_register_host(rig: "DvoDepthRig", depth, rows: int, cols: int) -> np.ndarray:
    """A raw depth image registered to the colour camera on the host (include/dvo_amd.h, "depth registration": the definition; no
    device needed): (rows, cols) uint16 millimetres in the colour image's pixel grid, 0 = hole.  depth: (depth_rows, depth_cols) of
    the rig, uint16 millimetres or float metres"""
    fmt, d = _raw_depth(depth, rig)
    out = np.zeros((rows, cols), np.uint16)
    rc = load_library().dvo_depth_register_host(C.byref(rig), _ptr(d), fmt, rows, cols, _ptr(out))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_depth_register_host refused its arguments")
    return out


def archive_blob_info(blob) -> dict:
    """Header and table of a key-frame archive blob (DvoTracker.export_archive), validated on the host -- no tracker, no device:
    dict(version, rows, cols, n_levels, first_shift, places_level, D, n_key_frames, total_bytes).  DvoError (DVO_ERR_INVALID) names the
    defect of a blob that is not valid"""
    lib = load_library()
    data = bytes(blob)
    info = DvoArchiveBlobInfo()
    rc = lib.dvo_archive_blob_info(data, len(data), C.byref(info))
    if rc != DVO_OK:
        raise DvoError(rc, lib.dvo_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in DvoArchiveBlobInfo._fields_}


def _iters(iters: Sequence[int]):
    arr = (C.c_int * len(iters))(*[int(x) for x in iters])
    return arr


class DvoContext:
    """One engine context = ``dvo_ctx`` (n_pairs frame pairs resident in HBM)."""

    def __init__(self, n_pairs: int = 1, params: Optional[DvoParams] = None, **overrides):
        self.lib = load_library()
        p = DvoParams()
        self.lib.dvo_params_default(C.byref(p))
        if params is not None:
            p = params
        for k, v in overrides.items():
            setattr(p, k, v)
        self.params = p
        self._h = C.c_void_p()
        rc = self.lib.dvo_create_batch(C.byref(p), int(n_pairs), C.byref(self._h))
        if rc != DVO_OK:
            raise DvoError(rc, (self.lib.dvo_last_error(None) or b"").decode())
        self.n_pairs = int(n_pairs)
        self._N = {}      # (pair, level) -> N
        self._dims = {}   # level -> (rows, cols)
        self._frame_keep = []   # host buffers borrowed by DVO_UPLOAD_ASYNC uploads, released at the next synchronisation
        self._depth_shapes = {}  # pair -> (depth_rows, depth_cols) of its depth rig: what register_depth checks host arrays against

    # -- plumbing -----------------------------------------------------------
    def _chk(self, rc: int):
        if rc != DVO_OK:
            raise DvoError(rc, (self.lib.dvo_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.dvo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, hip_stream: int):
        self._chk(self.lib.dvo_set_stream(self._h, C.c_void_p(hip_stream)))

    def use_own_stream(self):
        self._chk(self.lib.dvo_use_own_stream(self._h))

    def set_keep_warm(self, period_us: int):
        """launch a no-op kernel every period_us microseconds from a thread of the context (0 = stop): holds the GPU's active
        clocks between the frames of a single camera stream"""
        self._chk(self.lib.dvo_set_keep_warm(self._h, int(period_us)))

    def set_keep_warm2(self, busy_us: int, pause_us: int = 0):
        """one wave busy for busy_us microseconds, pause_us apart (0 = back to back), from a thread of the context; busy_us = 0 stops"""
        self._chk(self.lib.dvo_set_keep_warm2(self._h, int(busy_us), int(pause_us)))

    def synchronize(self):
        self._chk(self.lib.dvo_synchronize(self._h))
        self._frame_keep.clear()

    # -- inputs -------------------------------------------------------------
    def set_intrinsics(self, fx, fy, cx, cy):
        self._chk(self.lib.dvo_set_intrinsics(self._h, fx, fy, cx, cy))

    def set_ref_level(self, level: int, xyz, pair: int = 0):
        xyz = _f32(xyz).reshape(-1)
        n = xyz.size // 3
        self._chk(self.lib.dvo_set_ref_level_pair(self._h, pair, level, _ptr(xyz), n))
        self._N[(pair, level)] = n

    def set_now_level(self, level: int, dt, gx, gy, rows: int, cols: int, pair: int = 0):
        dt, gx, gy = _f32(dt).reshape(-1), _f32(gx).reshape(-1), _f32(gy).reshape(-1)
        assert dt.size == gx.size == gy.size == rows * cols
        self._chk(self.lib.dvo_set_now_level_pair(self._h, pair, level, _ptr(dt), _ptr(gx), _ptr(gy), rows, cols))
        self._dims[level] = (rows, cols)

    def set_ref_level_device(self, level: int, d_xyz_ptr: int, n: int, pair: int = 0):
        self._chk(self.lib.dvo_set_ref_level_device(self._h, pair, level, C.c_void_p(d_xyz_ptr), n))
        self._N[(pair, level)] = n

    def set_now_level_device(self, level: int, d_dt: int, d_gx: int, d_gy: int, rows: int, cols: int, pair: int = 0):
        self._chk(self.lib.dvo_set_now_level_device(self._h, pair, level, C.c_void_p(d_dt), C.c_void_p(d_gx),
                                                    C.c_void_p(d_gy), rows, cols))
        self._dims[level] = (rows, cols)

    def set_now_level_from_edges(self, level: int, edge, rows: int, cols: int, pair: int = 0):
        """computeDistTransfrmOfNow after Canny, on the GPU: uint8 edge mask -> resident now level"""
        edge = np.ascontiguousarray(edge, dtype=np.uint8).reshape(-1)
        assert edge.size == rows * cols
        self._chk(self.lib.dvo_set_now_level_from_edges(self._h, pair, level, _ptr(edge), rows, cols))
        self._dims[level] = (rows, cols)

    def get_now_level(self, level: int, pair: int = 0):
        rows, cols = self._dims[level]
        dt, gx, gy = (np.zeros(rows * cols, np.float32) for _ in range(3))
        self._chk(self.lib.dvo_get_now_level(self._h, pair, level, _ptr(dt), _ptr(gx), _ptr(gy)))
        return dt, gx, gy

    def get_ref_level(self, level: int, pair: int = 0):
        n = C.c_int()
        self._chk(self.lib.dvo_get_ref_level(self._h, pair, level, None, 0, C.byref(n)))
        xyz = np.zeros(3 * n.value, np.float32)
        self._chk(self.lib.dvo_get_ref_level(self._h, pair, level, _ptr(xyz), n.value, C.byref(n)))
        return xyz.reshape(-1, 3)

    def replicate_pairs(self, n_src: int, dst_first: int = 0, dst_count: Optional[int] = None):
        """slot p <- device copy of pair (p - dst_first) % n_src, for every level that is set"""
        dst_count = self.n_pairs - dst_first if dst_count is None else dst_count
        self._chk(self.lib.dvo_replicate_pairs(self._h, n_src, dst_first, dst_count))
        for (p, l), n in list(self._N.items()):
            if p < n_src:
                for q in range(dst_first, dst_first + dst_count):
                    if (q - dst_first) % n_src == p:
                        self._N[(q, l)] = n

    def set_ref_level_from_images(self, level: int, edge, depth_mm, rows: int, cols: int, pair: int = 0):
        """selectedPts + enlistRefEdgePts on the GPU; returns (xyz[N,3], uv[N,2])."""
        edge = np.ascontiguousarray(edge, dtype=np.int32).reshape(-1)
        depth = _f32(depth_mm).reshape(-1)
        cap = rows * cols
        xyz = np.zeros(3 * cap, np.float32)
        uv = np.zeros(2 * cap, np.float32)
        n = C.c_int(0)
        self._chk(self.lib.dvo_set_ref_level_from_images(self._h, pair, level, _ptr(edge), _ptr(depth), rows, cols,
                                                         _ptr(xyz), _ptr(uv), cap, C.byref(n)))
        self._N[(pair, level)] = n.value
        return xyz[:3 * n.value].reshape(-1, 3).copy(), uv[:2 * n.value].reshape(-1, 2).copy()

    # -- hot path -----------------------------------------------------------
    def run_iterations(self, level: int, max_iters: int, R, t, pair: int = 0, want_final: bool = True):
        """SolveDVO::runIterations.  Returns dict(R, t, energy, final_eps, final_reproj, best_idx, visible_ratio)."""
        R = np.array(R, dtype=np.float64, order="F").copy(order="F")
        t = np.array(t, dtype=np.float64).copy()
        n = self._N[(pair, level)]
        energy = np.zeros(max_iters, np.float32)
        feps = np.zeros(n, np.float32) if want_final else None
        frep = np.zeros(3 * n, np.float32) if want_final else None
        best = C.c_int(-2)
        ratio = C.c_float(0)
        self._chk(self.lib.dvo_run_iterations_pair(self._h, pair, level, max_iters, _ptr(R), _ptr(t), _ptr(energy),
                                                   _ptr(feps), _ptr(frep), C.byref(best), C.byref(ratio)))
        return dict(R=R, t=t, energy=energy, final_eps=feps,
                    final_reproj=None if frep is None else frep.reshape(-1, 3),
                    best_idx=best.value, visible_ratio=ratio.value)

    def align_batch(self, iters: Sequence[int], R, t, first_pair: int = 0, n_pairs: Optional[int] = None,
                    flags: int = 0):
        """Level schedule of SolveDVO::loop for a range of pairs.  R: [n,3,3] (math layout), t: [n,3]."""
        n_pairs = self.n_pairs - first_pair if n_pairs is None else n_pairs
        Rm = np.asarray(R, dtype=np.float64).reshape(n_pairs, 3, 3)
        Rc = np.ascontiguousarray(np.transpose(Rm, (0, 2, 1)))   # column-major per pair
        tc = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(n_pairs, 3))
        self._chk(self.lib.dvo_align_batch(self._h, first_pair, n_pairs, len(iters), _iters(iters), flags,
                                           _ptr(Rc), _ptr(tc)))
        return np.transpose(Rc, (0, 2, 1)).copy(), tc

    def set_poses(self, R, t, first_pair: int = 0):
        Rm = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
        n = Rm.shape[0]
        Rc = np.ascontiguousarray(np.transpose(Rm, (0, 2, 1)))
        tc = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(n, 3))
        self._chk(self.lib.dvo_set_poses(self._h, first_pair, n, _ptr(Rc), _ptr(tc)))

    def enqueue(self, iters: Sequence[int], first_pair: int = 0, n_pairs: Optional[int] = None, flags: int = 0):
        n_pairs = self.n_pairs - first_pair if n_pairs is None else n_pairs
        self._chk(self.lib.dvo_align_batch_enqueue(self._h, first_pair, n_pairs, len(iters), _iters(iters), flags))

    def get_poses(self, first_pair: int = 0, n_pairs: Optional[int] = None):
        n_pairs = self.n_pairs - first_pair if n_pairs is None else n_pairs
        R = np.empty((n_pairs, 3, 3))
        t = np.empty((n_pairs, 3))
        self._chk(self.lib.dvo_get_poses_rows(self._h, first_pair, n_pairs, _ptr(R), _ptr(t)))      # row-major, as numpy holds them
        self._frame_keep.clear()          # dvo_get_poses_rows synchronises the context stream
        return R, t

    def enqueue_counts(self):
        """(full passes, launches served from the memo) of enqueue() since the context was made (dvo_get_enqueue_counts)"""
        full, hits = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(self.lib.dvo_get_enqueue_counts(self._h, C.byref(full), C.byref(hits)))
        return full.value, hits.value

    def level_report(self, pair: int, level: int, n_energy: int):
        energy = np.zeros(n_energy, np.float32)
        best = C.c_int(-2)
        ratio = C.c_float(0)
        self._chk(self.lib.dvo_get_level_report(self._h, pair, level, _ptr(energy), n_energy, C.byref(best),
                                                C.byref(ratio)))
        return energy, best.value, ratio.value

    def final_outputs(self, pair: int, capacity: int):
        feps = np.zeros(capacity, np.float32)
        frep = np.zeros(3 * capacity, np.float32)
        n = C.c_int(0)
        self._chk(self.lib.dvo_get_final_outputs(self._h, pair, _ptr(feps), _ptr(frep), capacity, C.byref(n)))
        return feps[:n.value].copy(), frep[:3 * n.value].reshape(-1, 3).copy()

    # -- frames in: rows f1 + f2 (Canny, distance transform, point extraction, pyramid on the GPU) -----
    def frames_reserve(self, n_slots: int):
        self._chk(self.lib.dvo_frames_reserve(self._h, n_slots))

    @staticmethod
    def _image(a, kind: str, layout: int):
        """kind 'grey': uint8 or float32; 'depth': uint16 (mm) or float32 (mm).  `a` is a 2-D (rows, cols) array
        for ROW_MAJOR, or the same 2-D array given in Fortran order / a transposed buffer for COL_MAJOR."""
        a = np.asarray(a)
        rows, cols = a.shape
        if a.dtype == np.uint8 and kind == "grey":
            dt = DVO_PIX_U8
        elif a.dtype == np.uint16 and kind == "depth":
            dt = DVO_PIX_U16
        else:
            a = a.astype(np.float32, copy=False)
            dt = DVO_PIX_F32
        buf = np.ascontiguousarray(a) if layout == DVO_LAYOUT_ROW_MAJOR else np.ascontiguousarray(a.T)
        return DvoImage(buf.ctypes.data, rows, cols, dt, layout), buf

    def frames_upload_pyramids(self, frames, first_slot: int = 0, layout: int = DVO_LAYOUT_ROW_MAJOR, flags: int = 0,
                               now_first_pair: int = -1):
        """frames: list of frames; a frame = list over levels of (grey, depth) or (grey, None); 2-D (rows, cols) arrays."""
        count, nl = len(frames), len(frames[0])
        keep, G, D = [], (DvoImage * (count * nl))(), (DvoImage * (count * nl))()
        have_depth = frames[0][0][1] is not None
        for f, fr in enumerate(frames):
            for l, (g, d) in enumerate(fr):
                G[f * nl + l], b = self._image(g, "grey", layout); keep.append(b)
                _mapped_ok(flags, b, g)
                if have_depth:
                    D[f * nl + l], b = self._image(d, "depth", layout); keep.append(b)
                    _mapped_ok(flags, b, d)
        self._chk(self.lib.dvo_frames_upload_pyramids(self._h, first_slot, count, nl, G, D if have_depth else None,
                                                      now_first_pair, flags))
        if flags & DVO_UPLOAD_ASYNC:
            self._frame_keep.append(keep)
        for l, (g, _) in enumerate(frames[0]):
            self._dims[l] = tuple(np.asarray(g).shape)

    def _upload_cameras(self, first_slot, count, B, ifmt, Dp, dfmt, rows, cols, n_levels, first_shift, now_first_pair, flags):
        if (ifmt, dfmt) == (DVO_CAM_BGR8, DVO_DEPTH_F32):
            return self.lib.dvo_frames_upload_cameras(self._h, first_slot, count, B, Dp, rows, cols, n_levels, first_shift, now_first_pair, flags)
        return self.lib.dvo_frames_upload_cameras_fmt(self._h, first_slot, count, B, ifmt, Dp, dfmt, rows, cols, n_levels, first_shift,
                                                      now_first_pair, flags)

    def frames_upload_cameras(self, bgr_list, depth_list=None, n_levels: int = 4, first_shift: int = 1,
                              first_slot: int = 0, flags: int = 0, now_first_pair: int = -1, rgb: bool = False):
        """bgr_list: list of (rows, cols, 3) uint8 BGR images (RGB with rgb=True) or of (rows, cols) uint8 mono8 images; depth_list:
        list of (rows, cols) float32 metres, or of uint16 millimetres (DVO_DEPTH_U16), or None"""
        count = len(bgr_list)
        ifmt, bl, dfmt, dl = _camera_arrays(bgr_list, depth_list, rgb, flags)
        rows, cols = bl[0].shape[:2]
        B = (C.c_void_p * count)(*[b.ctypes.data for b in bl])
        Dp = None if dl is None else (C.c_void_p * count)(*[d.ctypes.data for d in dl])
        self._chk(self._upload_cameras(first_slot, count, B, ifmt, Dp, dfmt, rows, cols, n_levels, first_shift, now_first_pair, flags))
        if now_first_pair >= 0:
            self._note_dims(first_slot)
        if flags & DVO_UPLOAD_ASYNC:
            self._frame_keep.append((bl, dl))

    def frames_upload_cameras_device(self, bgr_ptrs, depth_ptrs, rows: int, cols: int, n_levels: int = 4, first_shift: int = 1,
                                     first_slot: int = 0, flags: int = 0, now_first_pair: int = -1,
                                     image_format: int = DVO_CAM_BGR8, depth_format: int = DVO_DEPTH_F32):
        """camera frames by address: in this GPU's memory (DVO_UPLOAD_DEVICE, the default) or, with flags | DVO_UPLOAD_MAPPED, in
        pinned host memory the GPU addresses (pulled over PCIe by a kernel).  Lists of addresses (ints) of (rows, cols, 3) uint8
        BGR images and, or None, (rows, cols) float32 depth images; image_format / depth_format (DVO_CAM_* / DVO_DEPTH_*) name
        other layouts behind the addresses"""
        count = len(bgr_ptrs)
        # a caller that feeds the same buffers every step (a decoder's ring) passes prepared tables: pointer_table(addresses)
        B = bgr_ptrs if isinstance(bgr_ptrs, C.Array) else (C.c_void_p * count)(*[int(p) for p in bgr_ptrs])
        Dp = None if depth_ptrs is None else (depth_ptrs if isinstance(depth_ptrs, C.Array) else (C.c_void_p * count)(*[int(p) for p in depth_ptrs]))
        if not flags & DVO_UPLOAD_MAPPED:
            flags |= DVO_UPLOAD_DEVICE
        self._chk(self._upload_cameras(first_slot, count, B, image_format, Dp, depth_format, rows, cols, n_levels, first_shift,
                                       now_first_pair, flags))
        if now_first_pair >= 0:
            self._note_dims(first_slot)

    @staticmethod
    def pointer_table(addresses):
        """a list of addresses as the C array frames_upload_cameras_device takes (built once, passed every step)"""
        return (C.c_void_p * len(addresses))(*[int(p) for p in addresses])

    def frames_as_now(self, first_slot: int = 0, first_pair: int = 0, count: int = 1):
        self._chk(self.lib.dvo_frames_as_now(self._h, first_slot, first_pair, count))
        self._note_dims(first_slot)

    def _note_dims(self, first_slot: int):
        for l in range(self.lib.dvo_frames_num_levels(self._h)):
            r, c_ = C.c_int(), C.c_int()
            self._chk(self.lib.dvo_frame_get_level(self._h, first_slot, l, C.byref(r), C.byref(c_), None, None, None, None))
            self._dims[l] = (r.value, c_.value)

    def frames_as_ref(self, first_slot: int = 0, first_pair: int = 0, count: int = 1):
        nl = self.lib.dvo_frames_num_levels(self._h)
        N = (C.c_int * (count * max(nl, 1)))()
        self._chk(self.lib.dvo_frames_as_ref(self._h, first_slot, first_pair, count, N))
        N = np.array(N[:], dtype=np.int64).reshape(count, max(nl, 1))
        for i in range(count):
            for l in range(nl):
                self._N[(first_pair + i, l)] = int(N[i, l])
        return N

    def frame_level(self, slot: int, level: int, want_depth: bool = True):
        """resident (grey u8, depth mm f32 or None, edge u8 0/255, n_edges) of a stored level, as 2-D (rows, cols) arrays"""
        r, c_ = C.c_int(), C.c_int()
        self._chk(self.lib.dvo_frame_get_level(self._h, slot, level, C.byref(r), C.byref(c_), None, None, None, None))
        rows, cols = r.value, c_.value
        grey, edge = np.zeros(rows * cols, np.uint8), np.zeros(rows * cols, np.uint8)
        depth = np.zeros(rows * cols, np.float32) if want_depth else None
        ne = C.c_int()
        self._chk(self.lib.dvo_frame_get_level(self._h, slot, level, None, None, _ptr(grey), _ptr(depth), _ptr(edge), C.byref(ne)))
        cm = lambda a: None if a is None else a.reshape(cols, rows).T.copy()      # column-major buffer -> (rows, cols)
        return cm(grey), cm(depth), cm(edge), ne.value

    # -- depth registration: raw depth of the depth camera -> the colour camera's pixel grid ---------
    def set_pair_depth_rig(self, pair: int, rig: Optional[DvoDepthRig], rows: int = 0, cols: int = 0):
        """depth rig of `pair` (-1: every pair) for colour images of rows x cols; None removes it (include/dvo_amd.h, "depth
        registration")"""
        self._chk(self.lib.dvo_frames_set_pair_depth_rig(self._h, pair, None if rig is None else C.byref(rig), rows, cols))
        for p in (range(self.n_pairs) if pair < 0 else [pair]):
            self._depth_shapes[p] = None if rig is None else (rig.depth_rows, rig.depth_cols)

    def register_depth(self, depths, first_pair: int = 0, flags: int = 0, depth_format: int = DVO_DEPTH_U16):
        """registers the raw depth images under the rigs of pairs first_pair ..: host arrays (uint16 millimetres, or float metres), or,
        with DVO_UPLOAD_DEVICE, their device addresses (ints) in depth_format.  Returns the device addresses of the registered 16-bit
        images, valid until the next registration: what frames_upload_cameras_device takes with depth_format=DVO_DEPTH_U16"""
        n = len(depths)
        keep = None
        if flags & DVO_UPLOAD_DEVICE:
            D = (C.c_void_p * n)(*[int(p) for p in depths])
        else:
            keep = [np.asarray(d) for d in depths]
            u16 = n > 0 and all(d.dtype == np.uint16 for d in keep)
            keep = [np.ascontiguousarray(d, dtype=np.uint16 if u16 else np.float32) for d in keep]
            for k, d in enumerate(keep):                         # the library reads depth_rows x depth_cols values behind each pointer
                shape = self._depth_shapes.get(first_pair + k)
                if shape is not None and d.shape != shape:
                    raise ValueError("raw depth image %d must have its rig's depth_rows x depth_cols %s" % (k, shape))
            depth_format = DVO_DEPTH_U16 if u16 else DVO_DEPTH_F32
            D = (C.c_void_p * n)(*[d.ctypes.data for d in keep])
        out = (C.c_void_p * max(n, 1))()
        self._chk(self.lib.dvo_frames_register_depth(self._h, first_pair, n, D, depth_format, flags, out))
        del keep                                                 # host sources are free again when the call returns
        return [int(out[k]) for k in range(n)]

    def get_registered_depth(self, pair: int) -> np.ndarray:
        """the registered image of `pair` from the last registration: (rows, cols) uint16 millimetres, 0 = hole"""
        r, c_ = C.c_int(), C.c_int()
        self._chk(self.lib.dvo_frames_get_registered_depth(self._h, pair, None, 0, C.byref(r), C.byref(c_)))
        out = np.zeros((r.value, c_.value), np.uint16)
        self._chk(self.lib.dvo_frames_get_registered_depth(self._h, pair, _ptr(out), out.size, None, None))
        return out

    # -- host-driven iteration (large frames / multi-GPU tiled mode) ---------
    def n_points(self, level: int, pair: int = 0) -> int:
        return self._N[(pair, level)]

    def iter_begin(self, level: int, max_iters: int, R, t, pair: int = 0):
        R = np.array(R, dtype=np.float64, order="F")
        t = np.array(t, dtype=np.float64)
        self._chk(self.lib.dvo_iter_begin(self._h, pair, level, max_iters, _ptr(R), _ptr(t)))
        self._iter_max = max_iters

    def iter_accumulate(self, level: int, first: int, count: int, d_acc32_ptr: int, pair: int = 0):
        self._chk(self.lib.dvo_iter_accumulate(self._h, pair, level, first, count, C.c_void_p(d_acc32_ptr)))

    def iter_update(self, level: int, itr: int, n_total: int, d_acc32_ptr: int, pair: int = 0):
        self._chk(self.lib.dvo_iter_update(self._h, pair, level, itr, n_total, C.c_void_p(d_acc32_ptr)))

    def iter_end(self, level: int, pair: int = 0):
        R, t = np.zeros((3, 3), order="F"), np.zeros(3)
        energy = np.zeros(self._iter_max, np.float32)
        best, ratio = C.c_int(-2), C.c_float(0)
        self._chk(self.lib.dvo_iter_end(self._h, pair, level, _ptr(R), _ptr(t), _ptr(energy), C.byref(best),
                                        C.byref(ratio)))
        return dict(R=R, t=t, energy=energy, best_idx=best.value, visible_ratio=ratio.value)

    def align_pyramid_wide(self, iters: Sequence[int], R, t, pair: int = 0, flags: int = 0):
        """level schedule with every iteration spread over all CUs (large single frames), driven from C"""
        R = np.array(R, dtype=np.float64, order="F").copy(order="F")
        t = np.array(t, dtype=np.float64).copy()
        self._chk(self.lib.dvo_align_pyramid_wide(self._h, pair, len(iters), _iters(iters), flags, _ptr(R), _ptr(t)))
        return R, t

    def frames_set_undistort(self, rows: int, cols: int, K4=None, D5=None):
        """cv::undistort with the camera-info calibration on every camera frame uploaded from now on; None, None = off"""
        if K4 is None and D5 is None:
            self._chk(self.lib.dvo_frames_set_undistort(self._h, rows, cols, None, None))
            return
        K = np.asarray(K4, np.float64).copy(); D = np.asarray(D5, np.float64).copy()
        assert K.size == 4 and D.size == 5
        self._chk(self.lib.dvo_frames_set_undistort(self._h, rows, cols, _ptr(K), _ptr(D)))

    def frames_set_pair_mask(self, pair: int, mask, n_levels: int = 4, first_shift: int = 1, margin: int = 2):
        """ignore mask of `pair` (-1: every pair, one device copy): (rows, cols), non-zero = ignore; None removes it.  Applied to the
        edge maps of the frames uploaded as the pair's now frame from now on (include/dvo_amd.h, "ignore masks")"""
        if mask is None:
            self._chk(self.lib.dvo_frames_set_pair_mask(self._h, pair, 0, 0, None, 0, 0, 0))
            return
        m = _mask_bytes(mask)
        self._chk(self.lib.dvo_frames_set_pair_mask(self._h, pair, m.shape[0], m.shape[1], _ptr(m), n_levels, first_shift, margin))

    def frames_get_pair_mask_level(self, pair: int, level: int) -> np.ndarray:
        """the resident keep plane of one level of the pair's mask: (rows_l, cols_l) uint8, 0 = dropped, 255 = kept"""
        r, c = C.c_int(), C.c_int()
        self._chk(self.lib.dvo_frames_get_pair_mask_level(self._h, pair, level, None, 0, C.byref(r), C.byref(c)))
        keep = np.zeros(r.value * c.value, np.uint8)
        self._chk(self.lib.dvo_frames_get_pair_mask_level(self._h, pair, level, _ptr(keep), keep.size, None, None))
        return keep.reshape(c.value, r.value).T.copy()

    # -- photometric Gauss-Newton (RGBDOdometry's engine) ------------------------
    def photo_configure(self, K, fixed: bool = False, **overrides):
        p = DvoPhotoParams()
        self.lib.dvo_photo_params_default(C.byref(p))
        p.fx, p.fy, p.cx, p.cy = (float(k) for k in K)
        p.fixed = int(fixed)
        for k, v in overrides.items():
            setattr(p, k, v)
        self._chk(self.lib.dvo_photo_configure(self._h, C.byref(p)))
        self._photo_iters = p.iterations

    def photo_set_ref(self, slot: int, first_level: int = 1):
        n = (C.c_int * DVO_MAX_LEVELS)()
        self._chk(self.lib.dvo_photo_set_ref(self._h, slot, first_level, n))
        return list(n)

    def photo_align(self, now_slot: int, T, levels=(3, 2)):
        T = np.array(T, dtype=np.float64, order="C").copy()
        lv = (C.c_int * len(levels))(*levels)
        norms = np.zeros((len(levels), getattr(self, "_photo_iters", 3)), np.float64)
        upd = (C.c_int * len(levels))()
        self._chk(self.lib.dvo_photo_align(self._h, now_slot, lv, len(levels), _ptr(T), _ptr(norms), upd))
        return T, norms, list(upd)

    def photo_jacobian(self, level: int, capacity: int = 50000):
        J = np.zeros((capacity, 6), np.float64); si = np.zeros(capacity, np.int32); sj = np.zeros(capacity, np.int32)
        A = np.zeros((6, 6), np.float64); n = C.c_int(0)
        self._chk(self.lib.dvo_photo_get_jacobian(self._h, level, _ptr(J), _ptr(si), _ptr(sj), capacity, _ptr(A), C.byref(n)))
        return dict(J=J[:n.value].copy(), sel_i=si[:n.value].copy(), sel_j=sj[:n.value].copy(), A=A, n=n.value)

    # -- tiled mode driven from C (RCCL) ---------------------------------------
    def tiled_attach(self, comm, rank: int, world: int, rccl_library: Optional[str] = None):
        """comm: the rank's ncclComm_t (integer / c_void_p), e.g. RcclComm(...).comm"""
        lib = rccl_library.encode() if rccl_library else None
        self._chk(self.lib.dvo_tiled_attach(self._h, C.c_void_p(int(comm)), rank, world, lib))

    def tiled_detach(self):
        self._chk(self.lib.dvo_tiled_detach(self._h))

    def align_pyramid_tiled(self, iters: Sequence[int], R, t, pair: int = 0, flags: int = 0):
        """dvo_align_pyramid_tiled: this rank's share of every iteration + ncclAllReduce of the 32 sums + identical update"""
        R = np.array(R, dtype=np.float64, order="F").copy(order="F")
        t = np.array(t, dtype=np.float64).copy()
        self._chk(self.lib.dvo_align_pyramid_tiled(self._h, pair, len(iters), _iters(iters), flags, _ptr(R), _ptr(t)))
        return R, t

    def tiled_graph_replayed(self) -> bool:
        """the last align_pyramid_tiled replayed its captured graph (kernel + ncclAllReduce per iteration, no host work between)"""
        g = C.c_int(0)
        self._chk(self.lib.dvo_tiled_graph_replayed(self._h, C.byref(g)))
        return bool(g.value)

    def wide_packed_levels(self) -> int:
        """bit l set: level l of the last enqueued align_pyramid_wide / _tiled schedule ran the packed step kernel (compact list)"""
        g = C.c_int(0)
        self._chk(self.lib.dvo_wide_packed_levels(self._h, C.byref(g), None))
        return g.value

    def wide_team_levels(self) -> int:
        """bit l set: level l of the last align_pyramid_wide ran inside the fused kernel's team launch (coarse levels of a large frame)"""
        g = C.c_int(0)
        self._chk(self.lib.dvo_wide_team_levels(self._h, C.byref(g)))
        return g.value

    def wide_solo_levels(self) -> int:
        """bit l set: level l of that schedule ran as ONE launch of one workgroup for all its iterations (small levels)"""
        g, s = C.c_int(0), C.c_int(0)
        self._chk(self.lib.dvo_wide_packed_levels(self._h, C.byref(g), C.byref(s)))
        return s.value

    def tiled_shard(self, level: int, pair: int = 0):
        """(first, count): the index range of `level`'s reference list this rank works on"""
        f, n = C.c_int(0), C.c_int(0)
        self._chk(self.lib.dvo_tiled_shard(self._h, pair, level, C.byref(f), C.byref(n)))
        return f.value, n.value

    # -- inspection -----------------------------------------------------------
    def eval_points(self, level: int, R, t, pair: int = 0):
        n = self._N[(pair, level)]
        R = np.array(R, dtype=np.float64, order="F")
        t = np.array(t, dtype=np.float64)
        rep, J = np.zeros(3 * n, np.float32), np.zeros(6 * n, np.float32)
        eps, w, vis = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        self._chk(self.lib.dvo_eval_points(self._h, pair, level, _ptr(R), _ptr(t), _ptr(rep), _ptr(J), _ptr(eps),
                                           _ptr(w), _ptr(vis)))
        return dict(reproj=rep.reshape(-1, 3), J=J.reshape(-1, 6), eps=eps, w=w, visible=vis)

    def accumulate(self, level: int, R, t, pair: int = 0) -> np.ndarray:
        R = np.array(R, dtype=np.float64, order="F")
        t = np.array(t, dtype=np.float64)
        acc = np.zeros(DVO_NUM_ACC)
        self._chk(self.lib.dvo_accumulate(self._h, pair, level, _ptr(R), _ptr(t), _ptr(acc)))
        return acc

    def se3_exp(self, psi):
        psi = np.array(psi, dtype=np.float64)
        R = np.zeros((3, 3), order="F")
        t = np.zeros(3)
        self._chk(self.lib.dvo_device_se3_exp(self._h, _ptr(psi), _ptr(R), _ptr(t)))
        return R, t

    def se3_log(self, R, t):
        R = np.array(R, dtype=np.float64, order="F")
        t = np.array(t, dtype=np.float64)
        psi = np.zeros(6)
        self._chk(self.lib.dvo_device_se3_log(self._h, _ptr(R), _ptr(t), _ptr(psi)))
        return psi

    def rotationize(self, R):
        R = np.array(R, dtype=np.float64, order="F").copy(order="F")
        self._chk(self.lib.dvo_device_rotationize(self._h, _ptr(R)))
        return R

    def debug_stamps(self, pair: int = 0) -> np.ndarray:
        out = np.zeros(64, np.uint64)
        self._chk(self.lib.dvo_debug_stamps(self._h, pair, _ptr(out)))
        return out.reshape(8, 8)

    def level_normal_matrix(self, pair: int, level: int, itr: int = -1) -> np.ndarray:
        """H = sum w J^T J (6x6) of iterate `itr` (default: the best) of the last align made with DVO_FLAG_NORMAL_MATRIX"""
        H = np.zeros(36, np.float64)
        self._chk(self.lib.dvo_get_level_normal_matrix(self._h, pair, level, itr, _ptr(H)))
        return H.reshape(6, 6)

    def level_texel_mode(self, pair: int, level: int) -> int:
        """0 = 16-byte texels gathered from HBM/L2, 1 = the level's texels staged in LDS, 2 = the compact form, -1 = not run"""
        m = C.c_int(-2)
        self._chk(self.lib.dvo_get_level_texel_mode(self._h, pair, level, C.byref(m)))
        return m.value

    def level_energy_sweeps(self, pair: int, level: int) -> int:
        """iterations of that level whose energy came from the exact sweep of the residuals (the certificate of the fast sum failed,
        or engine_variant = 5)"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_level_energy_sweeps(self._h, pair, level, C.byref(m)))
        return m.value

    def level_exact_fallback(self, pair: int, level: int) -> bool:
        """True if a wave of the packed kernel took its literal-division fallback at that level of the last launch"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_level_exact_fallback(self._h, pair, level, C.byref(m)))
        return bool(m.value)

    def level_points4(self, pair: int, level: int) -> bool:
        """True if that level's reference points were read in their 4-byte form during the last launch"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_level_points4(self._h, pair, level, C.byref(m)))
        return bool(m.value)

    def level_points4_direct(self, pair: int, level: int) -> bool:
        """True if the 4-byte points of that level that lived in LDS during the last launch were held there in the direct form
        (column | row << 10 | millimetres << 19; never with engine_variant = 6)"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_level_points4_direct(self._h, pair, level, C.byref(m)))
        return bool(m.value)

    def level_final_fused(self, pair: int, level: int) -> bool:
        """True if that level's final outputs were written by its last sweep during the last launch (at the best of the iterates
        before the last one) and the separate pass over the level was skipped"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_level_final_fused(self._h, pair, level, C.byref(m)))
        return bool(m.value)

    def level_ranks_in_lds(self, pair: int, level: int) -> bool:
        """True if the last fused launch looked that level's ranks up in an LDS copy of the whole level (round 5)"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_level_ranks_in_lds(self._h, pair, level, C.byref(m)))
        return bool(m.value)

    def last_launch_shape(self):
        """(threads per workgroup, workgroups per pair, packed kernel?) of the last fused launch"""
        b, t, k = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.dvo_get_last_launch_shape(self._h, C.byref(b), C.byref(t), C.byref(k)))
        return b.value, t.value, bool(k.value)

    def now_prepare(self, first_pair: int = 0, count: Optional[int] = None):
        """build the compact (4 bytes per pixel) form of the resident now levels of these pairs now"""
        count = self.n_pairs - first_pair if count is None else count
        self._chk(self.lib.dvo_now_prepare(self._h, first_pair, count))

    def set_direct_compact(self, on: bool = True):
        """float now levels (set_now_level*) are turned into the compact form at installation (off by default)"""
        self._chk(self.lib.dvo_set_direct_compact(self._h, 1 if on else 0))

    def now_compact_info(self, pair: int, level: int) -> int:
        """> 0 palette size of the compact form, 0 not built, < 0 the builder's reason for keeping the 16-byte form"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_now_compact_info(self._h, pair, level, C.byref(m)))
        return m.value

    # -- measurement ----------------------------------------------------------
    def now_compact_partial(self, pair: int, level: int) -> bool:
        """True if that compact form is PARTIAL (round 5): the image's lowest ranks are in the compact form, the pixels it cannot express
        (too many distinct distances, 512 px or more from every edge, a rank step beyond +-127) are looked up in its 16-byte texels"""
        m = C.c_int(0)
        self._chk(self.lib.dvo_get_now_compact_partial(self._h, pair, level, C.byref(m)))
        return bool(m.value)

    def algorithmic_bytes(self, iters: Sequence[int], pair: int = 0, flags: int = 0) -> int:
        b = C.c_uint64(0)
        self._chk(self.lib.dvo_algorithmic_bytes(self._h, pair, len(iters), _iters(iters), flags, C.byref(b)))
        return b.value

    def point_iterations(self, iters: Sequence[int], pair: int = 0) -> int:
        b = C.c_uint64(0)
        self._chk(self.lib.dvo_point_iterations(self._h, pair, len(iters), _iters(iters), C.byref(b)))
        return b.value


def pose_covariance(H, sum_eps2: float, n_visible: int):
    """C = s^2 H^-1 with s^2 = sum_eps2 / (n_visible - 6), by Cholesky in double -- dvo_amd::poseCovariance of include/dvo_amd.hpp,
    the same formula.  The Gauss-Newton approximation with the robust weights held fixed, in the units of the distance-transform
    residual: a relative, uncalibrated scale that a consumer may rescale.  None when n_visible <= 6 or H is not positive definite."""
    H = np.asarray(H, dtype=np.float64).reshape(6, 6)
    if n_visible <= 6 or not np.all(np.isfinite(H)):
        return None
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    Li = np.zeros((6, 6))                      # L^-1 by forward substitution; H^-1 = L^-T L^-1
    for k in range(6):
        for i in range(k, 6):
            Li[i, k] = ((1.0 if i == k else 0.0) - np.dot(L[i, k:i], Li[k:i, k])) / L[i, i]
    return (float(sum_eps2) / (n_visible - 6)) * (Li.T @ Li)


def graph_information(H, sum_eps2: float, n_visible: int) -> np.ndarray:
    """An edge's information from a tracker information record or a score record: H (n_visible - 6) / sum_eps2, the inverse of
    pose_covariance, (6, 6).  DvoError (DVO_ERR_INVALID) where pose_covariance returns None, and for a sum_eps2 that is not positive"""
    Hm = np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(36))
    out = np.zeros(36)
    rc = load_library().dvo_graph_information(_ptr(Hm), float(sum_eps2), int(n_visible), _ptr(out))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_graph_information refused its arguments")
    return out.reshape(6, 6)


def _graph_arrays(poses, fixed, edges):
    """(poses (n, 12) float64, fixed (n,) uint8, ctypes edge array or None, n_edges).  poses: (n, 12) {R column-major, t} or (n, 3, 4)
    [R | t]"""
    P = np.asarray(poses, dtype=np.float64)
    if P.ndim == 3 and P.shape[1:] == (3, 4):
        P = np.concatenate([P[:, :, :3].transpose(0, 2, 1).reshape(len(P), 9), P[:, :, 3]], axis=1)
    P = np.ascontiguousarray(P.reshape(-1, 12))
    f = np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.uint8)
    if len(f) != len(P):
        raise ValueError("one fixed flag per node")
    edges = list(edges)
    arr = (DvoGraphEdge * len(edges))(*edges) if edges else None
    return P, f, arr, len(edges)


def _graph_report(rep: "DvoGraphReport", trace) -> dict:
    return dict(cost0=rep.cost0, cost=rep.cost, lambda_=rep.lambda_, max_step=rep.max_step, iterations=rep.iterations, accepted=rep.accepted,
                cg_iterations=rep.cg_iterations, status=rep.status, cost_trace=np.array(trace[:rep.iterations + 1]))


def pose_graph_solve_host(poses, fixed, edges, params: Optional["DvoGraphParams"] = None):
    """dvo_graph_solve_host: the definition of the pose-graph solver on the host, no device needed.  edges: DvoGraphEdge objects.
    Returns (poses (n, 12), report dict with cost_trace)"""
    lib = load_library()
    P, f, arr, ne = _graph_arrays(poses, fixed, edges)
    P = P.copy()
    p = params if params is not None else DvoGraphParams.default()
    rep = DvoGraphReport()
    trace = np.zeros(max(int(p.max_iterations), 0) + 1)
    rc = lib.dvo_graph_solve_host(C.byref(p), len(P), _ptr(P), _ptr(f), ne, arr, C.byref(rep), _ptr(trace), len(trace))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_graph_solve_host refused its arguments")
    return P, _graph_report(rep, trace)


def _marginal_report(rep: "DvoGraphMarginalReport") -> dict:
    return dict(worst_residual=rep.worst_residual, cg_iterations=rep.cg_iterations, cg_iterations_max=rep.cg_iterations_max, status=rep.status)


def pose_graph_marginals_host(poses, fixed, edges, nodes, params: Optional["DvoGraphParams"] = None):
    """dvo_graph_marginals_host: the definition of the marginal covariances on the host, no device needed.  nodes: the m nodes whose
    joint covariance is wanted.  Returns (cov (6m, 6m), report dict)"""
    lib = load_library()
    P, f, arr, ne = _graph_arrays(poses, fixed, edges)
    q = (C.c_int * len(nodes))(*[int(v) for v in nodes])
    cov = np.zeros((6 * len(nodes), 6 * len(nodes)))
    rep = DvoGraphMarginalReport()
    rc = lib.dvo_graph_marginals_host(C.byref(params) if params is not None else None, len(P), _ptr(P), _ptr(f), ne, arr, len(nodes), q,
                                      _ptr(cov), C.byref(rep))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_graph_marginals_host refused its arguments")
    return cov, _marginal_report(rep)


def pose_graph_edge_chi2(pose_i, pose_j, cov, edge: "DvoGraphEdge"):
    """dvo_graph_edge_chi2: the gate for a closure candidate.  pose_i, pose_j: 12 doubles {R column-major, t} each; cov: the joint
    (12, 12) covariance of (i, j) or None (zero).  Returns (r (6,), S (6, 6), chi2)"""
    Pi = np.ascontiguousarray(np.asarray(pose_i, dtype=np.float64).reshape(12))
    Pj = np.ascontiguousarray(np.asarray(pose_j, dtype=np.float64).reshape(12))
    Cv = None if cov is None else np.ascontiguousarray(np.asarray(cov, dtype=np.float64).reshape(144))
    r, S, chi2 = np.zeros(6), np.zeros((6, 6)), C.c_double(0.0)
    rc = load_library().dvo_graph_edge_chi2(_ptr(Pi), _ptr(Pj), None if Cv is None else _ptr(Cv), C.byref(edge), _ptr(r), _ptr(S), C.byref(chi2))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_graph_edge_chi2 refused its arguments")
    return r, S, chi2.value


class DvoPoseGraphs:
    """A dvo_graph_batch (include/dvo_amd.h, "pose graphs"): up to max_graphs pose graphs solved together, one workgroup per graph,
    one launch per solve.  Stand-alone: no DvoContext, no tracker."""

    def __init__(self, max_graphs: int, max_nodes_total: int, max_edges_total: int):
        self.lib = load_library()
        self._h = C.c_void_p()
        rc = self.lib.dvo_graph_create(max_graphs, max_nodes_total, max_edges_total, C.byref(self._h))
        if rc != DVO_OK:
            self._h = C.c_void_p()
            raise DvoError(rc, self.lib.dvo_graph_last_error(None).decode())
        self._n = {}

    def _chk(self, rc: int):
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_graph_last_error(self._h).decode())

    def close(self):
        if self._h:
            self.lib.dvo_graph_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, graph: int, poses, fixed, edges):
        """stage graph `graph` on the host (validated; no device work)"""
        P, f, arr, ne = _graph_arrays(poses, fixed, edges)
        self._chk(self.lib.dvo_graph_set(self._h, graph, len(P), _ptr(P), _ptr(f), ne, arr))
        self._n[graph] = len(P)

    def solve(self, graphs: Sequence[int], params: Optional["DvoGraphParams"] = None):
        g = (C.c_int * len(graphs))(*[int(q) for q in graphs])
        self._chk(self.lib.dvo_graph_solve(self._h, C.byref(params) if params is not None else None, len(graphs), g))

    def marginals(self, graphs: Sequence[int], nodes, params: Optional["DvoGraphParams"] = None):
        """dvo_graph_marginals: the joint covariance of nodes[k] (m nodes, the same m for every graph) of graphs[k] at its current poses.
        Returns (cov (count, 6m, 6m), list of report dicts)"""
        count = len(graphs)
        q = np.ascontiguousarray(np.asarray(nodes, dtype=np.int32).reshape(count, -1) if count else np.zeros((0, 1), np.int32))
        m = q.shape[1]
        g = (C.c_int * count)(*[int(v) for v in graphs])
        cov = np.zeros((count, 6 * m, 6 * m))
        reps = (DvoGraphMarginalReport * max(count, 1))()
        self._chk(self.lib.dvo_graph_marginals(self._h, C.byref(params) if params is not None else None, count, g, m,
                                               q.ctypes.data_as(C.POINTER(C.c_int)), _ptr(cov), reps))
        return cov, [_marginal_report(reps[k]) for k in range(count)]

    def poses(self, graph: int) -> np.ndarray:
        if graph not in self._n:
            raise DvoError(DVO_ERR_STATE, "graph %d was never set" % graph)
        P = np.zeros((self._n[graph], 12))
        self._chk(self.lib.dvo_graph_get_poses(self._h, graph, _ptr(P)))
        return P

    def report(self, graph: int) -> dict:
        rep = DvoGraphReport()
        self._chk(self.lib.dvo_graph_get_report(self._h, graph, C.byref(rep), None, 0))
        trace = np.zeros(rep.iterations + 1)
        self._chk(self.lib.dvo_graph_get_report(self._h, graph, C.byref(rep), _ptr(trace), len(trace)))
        return _graph_report(rep, trace)

    def stats(self):
        """(kernel launches, host synchronisations) of the last solve or marginals call"""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.dvo_graph_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _tsdf_frames(depth, K4, poses):
    """(depth as a list, n, K (n, 4), poses (n, 12)) of a frame list.  K4: one fx, fy, cx, cy for all frames or one per frame; poses:
    (n, 12) {R column-major, t} or (n, 3, 4) [R | t], camera to world"""
    depth = list(depth)
    n = len(depth)
    P = np.asarray(poses, dtype=np.float64)
    if P.ndim == 3 and P.shape[1:] == (3, 4):
        P = np.concatenate([P[:, :, :3].transpose(0, 2, 1).reshape(len(P), 9), P[:, :, 3]], axis=1)
    P = np.ascontiguousarray(P.reshape(-1, 12))
    K = np.asarray(K4, dtype=np.float64)
    K = np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 4), (n, 4)) if K.size == 4 else K.reshape(-1, 4))
    if len(P) != n or len(K) != n:
        raise ValueError("one pose and one K4 per frame")
    return depth, n, K, P


def _tsdf_host_images(depth):
    imgs = [np.ascontiguousarray(d) for d in depth]
    if not imgs:
        return imgs, None, DVO_DEPTH_F32, 0, 0
    dt, shape = imgs[0].dtype, imgs[0].shape
    if dt not in (np.uint16, np.float32) or len(shape) != 2 or any(d.dtype != dt or d.shape != shape for d in imgs):
        raise ValueError("depth images: same-shape (rows, cols) arrays, all uint16 (millimetres) or all float32 (metres)")
    ptrs = (C.c_void_p * len(imgs))(*[d.ctypes.data for d in imgs])
    return imgs, ptrs, DVO_DEPTH_U16 if dt == np.uint16 else DVO_DEPTH_F32, shape[0], shape[1]


def tsdf_integrate_host(volume: "DvoTsdfVolume", voxels, depth, K4, poses, params: Optional["DvoTsdfParams"] = None) -> np.ndarray:
    """dvo_tsdf_integrate_host: the definition of depth fusion on the host, no device needed.  voxels: the volume's nx * ny * nz words
    (uint32) or None for a cleared volume; returns the words after the frames, applied in list order (the input is not changed)"""
    depth, n, K, P = _tsdf_frames(depth, K4, poses)
    imgs, ptrs, fmt, rows, cols = _tsdf_host_images(depth)
    words = np.zeros(volume.voxels, np.uint32) if voxels is None else np.array(voxels, dtype=np.uint32).reshape(-1)
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    p = params if params is not None else DvoTsdfParams.default()
    rc = load_library().dvo_tsdf_integrate_host(C.byref(volume), _ptr(words), C.byref(p), n, ptrs, fmt, rows, cols, _ptr(K), _ptr(P))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_tsdf_integrate_host refused its arguments")
    return words


def tsdf_extract_host(volume: "DvoTsdfVolume", voxels, min_weight: int = 1, capacity: Optional[int] = None):
    """dvo_tsdf_extract_host: the surface points of a volume in the definition's order.  Returns (points (min(n, capacity), 3) float32,
    n the full count); capacity None: all of them"""
    lib = load_library()
    words = np.ascontiguousarray(np.asarray(voxels, dtype=np.uint32).reshape(-1))
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    n = C.c_longlong(0)
    rc = lib.dvo_tsdf_extract_host(C.byref(volume), _ptr(words), int(min_weight), None, 0, C.byref(n))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_tsdf_extract_host refused its arguments")
    cap = n.value if capacity is None else int(capacity)
    pts = np.zeros((max(cap, 0), 3), np.float32)
    rc = lib.dvo_tsdf_extract_host(C.byref(volume), _ptr(words), int(min_weight), _ptr(pts) if cap > 0 else None, cap, C.byref(n))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_tsdf_extract_host refused its arguments")
    return pts[:min(n.value, max(cap, 0))], n.value


def _raycast_views(K4, poses):
    """(n, K (n, 4), poses (n, 12)) of a view list; K4 and poses as _tsdf_frames takes them"""
    P = np.asarray(poses, dtype=np.float64)
    n = len(P) if P.ndim >= 2 else P.size // 12
    _, n, K, P = _tsdf_frames([None] * n, K4, poses)
    return n, K, P


def _raycast_format(fmt) -> int:
    if fmt in ("u16", DVO_DEPTH_U16):
        return DVO_DEPTH_U16
    if fmt in ("f32", DVO_DEPTH_F32):
        return DVO_DEPTH_F32
    raise ValueError('fmt: "u16" (millimetres) or "f32" (metres)')


def tsdf_raycast_host(volume: "DvoTsdfVolume", voxels, K4, poses, rows: int, cols: int, params: Optional["DvoRaycastParams"] = None,
                      fmt="u16", normals: bool = False):
    """dvo_raycast_host: the definition of the ray cast on the host, no device needed.  One view per pose of the volume whose nx * ny * nz
    words are `voxels`.  Returns depth (n, rows, cols) uint16 millimetres or float32 metres (0 = a hole), and with normals=True a pair
    (depth, normals (n, rows, cols, 3) float32, world axes, zero where there is none)"""
    n, K, P = _raycast_views(K4, poses)
    code = _raycast_format(fmt)
    words = np.ascontiguousarray(np.asarray(voxels, dtype=np.uint32).reshape(-1))
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    rows, cols = int(rows), int(cols)
    depth = np.zeros((n, max(rows, 0), max(cols, 0)), np.uint16 if code == DVO_DEPTH_U16 else np.float32)
    nrm = np.zeros((n, max(rows, 0), max(cols, 0), 3), np.float32) if normals else None
    dp = (C.c_void_p * max(n, 1))(*[depth[i].ctypes.data for i in range(n)])
    np_ = (C.c_void_p * max(n, 1))(*[nrm[i].ctypes.data for i in range(n)]) if normals else None
    p = params if params is not None else DvoRaycastParams.default()
    rc = load_library().dvo_raycast_host(C.byref(volume), _ptr(words), C.byref(p), n, code, rows, cols, _ptr(K), _ptr(P), dp, np_)
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_raycast_host refused its arguments")
    return (depth, nrm) if normals else depth


def tsdf_mesh_host(volume: "DvoTsdfVolume", voxels, min_weight: int = 1):
    """dvo_mesh_host: the triangle mesh of a volume by the definition on the host, no device needed.  Returns (vertices (n, 3) float32,
    triangles (m, 3) int32) in the definition's order: one call for the counts and one for the mesh"""
    lib = load_library()
    words = np.ascontiguousarray(np.asarray(voxels, dtype=np.uint32).reshape(-1))
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    nv, nt = C.c_longlong(0), C.c_longlong(0)
    rc = lib.dvo_mesh_host(C.byref(volume), _ptr(words), int(min_weight), None, 0, None, 0, C.byref(nv), C.byref(nt))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_mesh_host refused its arguments")
    xyz, tri = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
    rc = lib.dvo_mesh_host(C.byref(volume), _ptr(words), int(min_weight), _ptr(xyz) if nv.value else None, nv.value,
                           _ptr(tri) if nt.value else None, nt.value, C.byref(nv), C.byref(nt))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_mesh_host refused its arguments")
    return xyz, tri


_IMAGE_FORMATS = {"bgr8": DVO_CAM_BGR8, "rgb8": DVO_CAM_RGB8, "mono8": DVO_CAM_MONO8}


def _image_format(fmt) -> int:
    """"bgr8", "rgb8", "mono8" or the DVO_CAM_* code"""
    if fmt in _IMAGE_FORMATS:
        return _IMAGE_FORMATS[fmt]
    if fmt in _IMAGE_FORMATS.values():
        return int(fmt)
    raise ValueError('image format: "bgr8", "rgb8" or "mono8"')


def _image_shape(code: int, rows: int, cols: int):
    return (rows, cols) if code == DVO_CAM_MONO8 else (rows, cols, 3)


def _tsdf_host_colour_images(images, code: int, rows: int, cols: int):
    imgs = [np.ascontiguousarray(m) for m in images]
    shape = _image_shape(code, rows, cols)
    if any(m.dtype != np.uint8 or m.shape != shape for m in imgs):
        raise ValueError("images: uint8 arrays of the depth images' rows x cols, (rows, cols, 3) or, for mono8, (rows, cols)")
    return imgs, (C.c_void_p * max(len(imgs), 1))(*[m.ctypes.data for m in imgs])


def _colour_words(volume: "DvoTsdfVolume", colours, copy: bool) -> np.ndarray:
    if colours is None:
        return np.zeros(volume.voxels, np.uint64)
    c = np.array(colours, dtype=np.uint64).reshape(-1) if copy else np.ascontiguousarray(np.asarray(colours, dtype=np.uint64).reshape(-1))
    if c.size != volume.voxels:
        raise ValueError("colours: nx * ny * nz words of 64 bits")
    return c


def tsdf_integrate_colour_host(volume: "DvoTsdfVolume", voxels, colours, depth, images, K4, poses, image_format="bgr8",
                               params: Optional["DvoTsdfParams"] = None):
    """dvo_colour_integrate_host: the definition of depth fusion with colour on the host, no device needed.  voxels, colours: the volume's
    words (uint32) and colour words (uint64), or None for cleared ones; images[i]: uint8, (rows, cols, 3) or, for "mono8", (rows, cols).
    Returns (words, colour words) after the frames, applied in list order (the inputs are not changed)"""
    depth, n, K, P = _tsdf_frames(depth, K4, poses)
    imgs, ptrs, fmt, rows, cols = _tsdf_host_images(depth)
    code = _image_format(image_format)
    images = list(images)
    if len(images) != n:
        raise ValueError("one image per frame")
    keep, iptrs = _tsdf_host_colour_images(images, code, rows, cols)
    words = np.zeros(volume.voxels, np.uint32) if voxels is None else np.array(voxels, dtype=np.uint32).reshape(-1)
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    cw = _colour_words(volume, colours, copy=True)
    p = params if params is not None else DvoTsdfParams.default()
    rc = load_library().dvo_colour_integrate_host(C.byref(volume), _ptr(words), _ptr(cw), C.byref(p), n, ptrs, fmt, iptrs, code, rows, cols,
                                                  _ptr(K), _ptr(P))
    del keep, imgs
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_colour_integrate_host refused its arguments")
    return words, cw


def tsdf_raycast_colour_host(volume: "DvoTsdfVolume", voxels, colours, K4, poses, rows: int, cols: int,
                             params: Optional["DvoRaycastParams"] = None, fmt="u16", image_format="bgr8", normals: bool = False):
    """dvo_colour_raycast_host: the definition of the coloured ray cast on the host.  Returns (depth, image) or, with normals=True,
    (depth, normals, image): depth and normals as tsdf_raycast_host gives them, image (n, rows, cols, 3) uint8 or, for "mono8",
    (n, rows, cols); a pixel without colour is 0"""
    n, K, P = _raycast_views(K4, poses)
    code, icode = _raycast_format(fmt), _image_format(image_format)
    words = np.ascontiguousarray(np.asarray(voxels, dtype=np.uint32).reshape(-1))
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    cw = _colour_words(volume, colours, copy=False)
    rows, cols = int(rows), int(cols)
    depth = np.zeros((n, max(rows, 0), max(cols, 0)), np.uint16 if code == DVO_DEPTH_U16 else np.float32)
    nrm = np.zeros((n, max(rows, 0), max(cols, 0), 3), np.float32) if normals else None
    img = np.zeros((n,) + _image_shape(icode, max(rows, 0), max(cols, 0)), np.uint8)
    dp = (C.c_void_p * max(n, 1))(*[depth[i].ctypes.data for i in range(n)])
    np_ = (C.c_void_p * max(n, 1))(*[nrm[i].ctypes.data for i in range(n)]) if normals else None
    ip_ = (C.c_void_p * max(n, 1))(*[img[i].ctypes.data for i in range(n)])
    p = params if params is not None else DvoRaycastParams.default()
    rc = load_library().dvo_colour_raycast_host(C.byref(volume), _ptr(words), _ptr(cw), C.byref(p), n, code, rows, cols, _ptr(K), _ptr(P), dp, np_,
                                                ip_, icode)
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_colour_raycast_host refused its arguments")
    return (depth, nrm, img) if normals else (depth, img)


def tsdf_mesh_colour_host(volume: "DvoTsdfVolume", voxels, colours, min_weight: int = 1):
    """dvo_colour_mesh_host: the coloured triangle mesh of a volume by the definition on the host.  Returns (vertices (n, 3) float32,
    triangles (m, 3) int32, colours (n, 3) uint8 R, G, B) in the definition's order: one call for the counts and one for the mesh"""
    lib = load_library()
    words = np.ascontiguousarray(np.asarray(voxels, dtype=np.uint32).reshape(-1))
    if words.size != volume.voxels:
        raise ValueError("voxels: nx * ny * nz words")
    cw = _colour_words(volume, colours, copy=False)
    nv, nt = C.c_longlong(0), C.c_longlong(0)
    rc = lib.dvo_colour_mesh_host(C.byref(volume), _ptr(words), _ptr(cw), int(min_weight), None, None, 0, None, 0, C.byref(nv), C.byref(nt))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_colour_mesh_host refused its arguments")
    xyz, tri, rgb = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32), np.zeros((nv.value, 3), np.uint8)
    rc = lib.dvo_colour_mesh_host(C.byref(volume), _ptr(words), _ptr(cw), int(min_weight), _ptr(xyz) if nv.value else None,
                                  _ptr(rgb) if nv.value else None, nv.value, _ptr(tri) if nt.value else None, nt.value, C.byref(nv), C.byref(nt))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_colour_mesh_host refused its arguments")
    return xyz, tri, rgb


def _esdf_words(volume: "DvoTsdfVolume", words) -> np.ndarray:
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(-1))
    if w.size != volume.voxels:
        raise ValueError("words: nx * ny * nz words")
    return w


def _esdf_points(points) -> np.ndarray:
    P = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    return P


def esdf_host(volume: "DvoTsdfVolume", voxels, params: Optional["DvoEsdfParams"] = None) -> np.ndarray:
    """dvo_esdf_host: the definition of the Euclidean distance field on the host, no device needed.  voxels: the volume's nx * ny * nz
    TSDF words; returns its ESDF words (uint32: d2 in bits 0..23, inside in bit 30, not observed in bit 31)"""
    w = _esdf_words(volume, voxels)
    out = np.zeros(volume.voxels, np.uint32)
    p = params if params is not None else DvoEsdfParams.default()
    rc = load_library().dvo_esdf_host(C.byref(volume), _ptr(w), C.byref(p), _ptr(out))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_esdf_host refused its arguments")
    return out


def esdf_distances_host(volume: "DvoTsdfVolume", words) -> np.ndarray:
    """dvo_esdf_distances_host: metres (float32, negative inside, +-inf without a site) of a volume's ESDF words"""
    w = _esdf_words(volume, words)
    out = np.zeros(volume.voxels, np.float32)
    rc = load_library().dvo_esdf_distances_host(C.byref(volume), _ptr(w), _ptr(out))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_esdf_distances_host refused its arguments")
    return out


def esdf_query_host(volume: "DvoTsdfVolume", words, points) -> np.ndarray:
    """dvo_esdf_query_host: the point query of points (n, 3) float64, world coordinates, against a volume's ESDF words.  Returns n
    records of ESDF_SAMPLE_DTYPE: status, unknown corners, distance in metres and its gradient"""
    w = _esdf_words(volume, words)
    P = _esdf_points(points)
    out = np.zeros(len(P), ESDF_SAMPLE_DTYPE)
    rc = load_library().dvo_esdf_query_host(C.byref(volume), _ptr(w), len(P), _ptr(P), _ptr(out))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_esdf_query_host refused its arguments")
    return out


def save_ply(path, vertices, triangles, colours=None):
    """a mesh as a binary little-endian PLY file: vertices (n, 3) float32, triangles (m, 3) int32 as lists of three vertex numbers, and
    with colours (n, 3) uint8 R, G, B the properties red, green, blue after z"""
    v = np.ascontiguousarray(np.asarray(vertices).reshape(-1, 3), dtype="<f4")
    t = np.asarray(triangles).reshape(-1, 3)
    faces = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    rgb_lines = ""
    if colours is not None:
        c = np.asarray(colours, dtype=np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("colours: one R, G, B per vertex")
        rec = np.zeros(len(v), dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
        rec["p"] = v
        rec["c"] = c
        v = rec
        rgb_lines = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = ("ply\nformat binary_little_endian 1.0\ncomment rgbd_odometry_amd triangle mesh\nelement vertex %d\nproperty float x\n"
              "property float y\nproperty float z\n%selement face %d\nproperty list uchar int vertex_indices\nend_header\n"
              % (len(v), rgb_lines, len(t)))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


class DvoTsdfVolumes:
    """A dvo_tsdf_batch (include/dvo_amd.h, "depth fusion"): up to max_volumes TSDF volumes in one pool of max_voxels_total voxels, any
    list of depth frames fused into them in one launch, their surface extracted as points, ray-cast views and triangle meshes; with
    enable_colour() the volumes also keep the colour of the frames' images ("colour in the map").  Stand-alone: no DvoContext, no tracker."""

    def __init__(self, max_volumes: int, max_voxels_total: int):
        self.lib = load_library()
        self._h = C.c_void_p()
        rc = self.lib.dvo_tsdf_create(max_volumes, max_voxels_total, C.byref(self._h))
        if rc != DVO_OK:
            self._h = C.c_void_p()
            raise DvoError(rc, self.lib.dvo_tsdf_last_error(None).decode())
        self._vol = {}
        self._dims = {}

    def _chk(self, rc: int):
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_tsdf_last_error(self._h).decode())

    def close(self):
        if self._h:
            self.lib.dvo_tsdf_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _n(self, volume: int) -> int:
        if volume not in self._vol:
            raise DvoError(DVO_ERR_STATE, "volume %d was never set" % volume)
        return self._vol[volume]

    def set_volume(self, volume: int, vol: "DvoTsdfVolume"):
        """the volume's geometry; it is cleared.  Volumes sit in the pool back to back in the order they are set"""
        self._chk(self.lib.dvo_tsdf_set_volume(self._h, volume, C.byref(vol)))
        self._vol[volume] = vol.voxels
        self._dims[volume] = (vol.nx, vol.ny, vol.nz)

    def clear(self, volume: int):
        self._chk(self.lib.dvo_tsdf_clear(self._h, volume))

    def integrate(self, volumes: Sequence[int], depth, K4, poses, params: Optional["DvoTsdfParams"] = None, device: bool = False,
                  shape=None, depth_format: Optional[int] = None):
        """dvo_tsdf_integrate: frame i -- depth[i], K4[i], poses[i] -- into volume volumes[i], one launch for the whole list.  depth: host
        arrays (uint16 millimetres or float32 metres); device=True: torch tensors on the handle's GPU (or raw device addresses with
        shape=(rows, cols) and depth_format), read in place"""
        depth, n, K, P = _tsdf_frames(depth, K4, poses)
        if len(volumes) != n:
            raise ValueError("one volume per frame")
        if device:
            if shape is None:
                shape = tuple(depth[0].shape)
                depth_format = DVO_DEPTH_U16 if depth[0].element_size() == 2 else DVO_DEPTH_F32
                if any(not d.is_contiguous() or tuple(d.shape) != shape for d in depth):
                    raise ValueError("device depth images: contiguous, all of one shape")
            keep = depth
            ptrs = (C.c_void_p * n)(*[int(d.data_ptr()) if hasattr(d, "data_ptr") else int(d) for d in depth])
            fmt, rows, cols = int(depth_format), int(shape[0]), int(shape[1])
        else:
            keep, ptrs, fmt, rows, cols = _tsdf_host_images(depth)
        v = (C.c_int * max(n, 1))(*[int(q) for q in volumes])
        p = params if params is not None else DvoTsdfParams.default()
        self._chk(self.lib.dvo_tsdf_integrate(self._h, C.byref(p), n, v, ptrs, fmt, rows, cols, _ptr(K), _ptr(P), DVO_UPLOAD_DEVICE if device else 0))
        del keep

    def enable_colour(self):
        """dvo_colour_enable: the handle gets its colour pool (8 bytes per voxel of max_voxels_total); a second call changes nothing"""
        self._chk(self.lib.dvo_colour_enable(self._h))

    def integrate_colour(self, volumes: Sequence[int], depth, images, K4, poses, image_format="bgr8", params: Optional["DvoTsdfParams"] = None,
                         device: bool = False, shape=None, depth_format: Optional[int] = None):
        """dvo_colour_integrate: integrate() with an image per frame -- uint8, (rows, cols, 3) "bgr8" / "rgb8" or (rows, cols) "mono8" --
        fused into the colour words beside the depth, one launch for the whole list.  device=True: depth and images are torch tensors on
        the handle's GPU (or raw device addresses with shape=(rows, cols) and depth_format), read in place"""
        depth, n, K, P = _tsdf_frames(depth, K4, poses)
        images = list(images)
        if len(volumes) != n or len(images) != n:
            raise ValueError("one volume and one image per frame")
        code = _image_format(image_format)
        if device:
            if shape is None:
                shape = tuple(depth[0].shape)
                depth_format = DVO_DEPTH_U16 if depth[0].element_size() == 2 else DVO_DEPTH_F32
                want = _image_shape(code, int(shape[0]), int(shape[1]))
                if any(not d.is_contiguous() or tuple(d.shape) != shape for d in depth):
                    raise ValueError("device depth images: contiguous, all of one shape")
                if any(not m.is_contiguous() or tuple(m.shape) != want or m.element_size() != 1 for m in images):
                    raise ValueError("device images: contiguous bytes of the depth images' rows x cols")
            keep = (depth, images)
            addr = lambda d: int(d.data_ptr()) if hasattr(d, "data_ptr") else int(d)
            ptrs = (C.c_void_p * n)(*[addr(d) for d in depth])
            iptrs = (C.c_void_p * n)(*[addr(m) for m in images])
            fmt, rows, cols = int(depth_format), int(shape[0]), int(shape[1])
        else:
            keep, ptrs, fmt, rows, cols = _tsdf_host_images(depth)
            keep2, iptrs = _tsdf_host_colour_images(images, code, rows, cols)
            keep = (keep, keep2)
        v = (C.c_int * max(n, 1))(*[int(q) for q in volumes])
        p = params if params is not None else DvoTsdfParams.default()
        self._chk(self.lib.dvo_colour_integrate(self._h, C.byref(p), n, v, ptrs, fmt, iptrs, code, rows, cols, _ptr(K), _ptr(P),
                                                DVO_UPLOAD_DEVICE if device else 0))
        del keep

    def get_colours(self, volume: int) -> np.ndarray:
        """dvo_colour_get_words: the volume's nx * ny * nz colour words (uint64: r, g, b in 1/256 levels and the count wc, 16 bits each)"""
        out = np.zeros(self._n(volume), np.uint64)
        self._chk(self.lib.dvo_colour_get_words(self._h, volume, _ptr(out)))
        return out

    def set_colours(self, volume: int, colours):
        c = np.ascontiguousarray(np.asarray(colours, dtype=np.uint64).reshape(-1))
        if c.size != self._n(volume):
            raise ValueError("colours: nx * ny * nz words of 64 bits")
        self._chk(self.lib.dvo_colour_set_words(self._h, volume, _ptr(c)))

    def points(self, volume: int, min_weight: int = 1, capacity: Optional[int] = None):
        """dvo_tsdf_extract_points: (points (min(n, capacity), 3) float32 in the definition's order, n the full count).  capacity None:
        all of them, which takes one extraction for the count and one for the points"""
        n = C.c_longlong(0)
        if capacity is None:
            self._chk(self.lib.dvo_tsdf_extract_points(self._h, volume, int(min_weight), None, 0, C.byref(n)))
            capacity = n.value
        cap = int(capacity)
        pts = np.zeros((max(cap, 0), 3), np.float32)
        self._chk(self.lib.dvo_tsdf_extract_points(self._h, volume, int(min_weight), _ptr(pts) if cap > 0 else None, cap, C.byref(n)))
        return pts[:min(n.value, max(cap, 0))], n.value

    def voxels(self, volume: int) -> np.ndarray:
        """the volume's nx * ny * nz words (uint32: q in the low half, w in the high half)"""
        out = np.zeros(self._n(volume), np.uint32)
        self._chk(self.lib.dvo_tsdf_get_voxels(self._h, volume, _ptr(out)))
        return out

    def set_voxels(self, volume: int, words):
        w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(-1))
        if w.size != self._n(volume):
            raise ValueError("voxels: nx * ny * nz words")
        self._chk(self.lib.dvo_tsdf_set_voxels(self._h, volume, _ptr(w)))

    def raycast(self, volumes: Sequence[int], K4, poses, rows: int, cols: int, params: Optional["DvoRaycastParams"] = None, fmt="u16",
                normals: bool = False, device: bool = False, image_format=None):
        """dvo_raycast_views: view i -- K4[i], poses[i] -- of volume volumes[i], one launch for the whole list.  Returns depth
        (n, rows, cols) uint16 millimetres or float32 metres (0 = a hole), and with normals=True a pair (depth, normals (n, rows, cols, 3)
        float32).  device=True: torch tensors on the handle's GPU, written in place by the kernel (16-bit depth as int16: the same bits),
        nothing copied back -- depth[i] is what integrate(..., device=True) takes.
        image_format "bgr8", "rgb8" or "mono8": dvo_colour_raycast_views, and the rendered images -- (n, rows, cols, 3) uint8 or, for
        "mono8", (n, rows, cols) -- come last in the result: (depth, image) or (depth, normals, image)"""
        n, K, P = _raycast_views(K4, poses)
        if len(volumes) != n:
            raise ValueError("one volume per view")
        code = _raycast_format(fmt)
        icode = None if image_format is None else _image_format(image_format)
        rows, cols = int(rows), int(cols)
        shape = (n, max(rows, 0), max(cols, 0))
        ishape = None if icode is None else (n,) + _image_shape(icode, shape[1], shape[2])
        if device:
            import torch
            depth = torch.zeros(shape, dtype=torch.int16 if code == DVO_DEPTH_U16 else torch.float32, device="cuda")
            nrm = torch.zeros(shape + (3,), dtype=torch.float32, device="cuda") if normals else None
            img = torch.zeros(ishape, dtype=torch.uint8, device="cuda") if icode is not None else None
            torch.cuda.synchronize()
            addr = lambda t, k: int(t[k].data_ptr())
        else:
            depth = np.zeros(shape, np.uint16 if code == DVO_DEPTH_U16 else np.float32)
            nrm = np.zeros(shape + (3,), np.float32) if normals else None
            img = np.zeros(ishape, np.uint8) if icode is not None else None
            addr = lambda a, k: a[k].ctypes.data
        dp = (C.c_void_p * max(n, 1))(*[addr(depth, k) for k in range(n)])
        np_ = (C.c_void_p * max(n, 1))(*[addr(nrm, k) for k in range(n)]) if normals else None
        v = (C.c_int * max(n, 1))(*[int(q) for q in volumes])
        p = params if params is not None else DvoRaycastParams.default()
        flags = DVO_UPLOAD_DEVICE if device else 0
        if icode is None:
            self._chk(self.lib.dvo_raycast_views(self._h, C.byref(p), n, v, code, rows, cols, _ptr(K), _ptr(P), dp, np_, flags))
            return (depth, nrm) if normals else depth
        ip_ = (C.c_void_p * max(n, 1))(*[addr(img, k) for k in range(n)])
        self._chk(self.lib.dvo_colour_raycast_views(self._h, C.byref(p), n, v, code, rows, cols, _ptr(K), _ptr(P), dp, np_, ip_, icode, flags))
        return (depth, nrm, img) if normals else (depth, img)

    def extract_mesh(self, volume: int, min_weight: int = 1, device: bool = False, colours: bool = False):
        """dvo_mesh_extract: the triangle mesh of a volume, (vertices (n, 3) float32, triangles (m, 3) int32) in the definition's order.
        One call with zero capacities for the counts, one for the mesh.  device=True: torch tensors on the handle's GPU, written in place
        by the kernels; only the counts come back.  colours=True: dvo_colour_mesh_extract, and the result is (vertices, triangles,
        colours (n, 3) uint8 R, G, B)"""
        nv, nt = C.c_longlong(0), C.c_longlong(0)
        flags = DVO_UPLOAD_DEVICE if device else 0
        if colours:
            self._chk(self.lib.dvo_colour_mesh_extract(self._h, volume, int(min_weight), None, None, 0, None, 0, C.byref(nv), C.byref(nt), 0))
        else:
            self._chk(self.lib.dvo_mesh_extract(self._h, volume, int(min_weight), None, 0, None, 0, C.byref(nv), C.byref(nt), 0))
        n, m = nv.value, nt.value
        if device:
            import torch
            xyz = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            tri = torch.zeros((m, 3), dtype=torch.int32, device="cuda")
            rgb = torch.zeros((n, 3), dtype=torch.uint8, device="cuda") if colours else None
            torch.cuda.synchronize()
            px, pt = (int(xyz.data_ptr()) if n else None), (int(tri.data_ptr()) if m else None)
            pc = int(rgb.data_ptr()) if colours and n else None
        else:
            xyz, tri = np.zeros((n, 3), np.float32), np.zeros((m, 3), np.int32)
            rgb = np.zeros((n, 3), np.uint8) if colours else None
            px, pt = (_ptr(xyz) if n else None), (_ptr(tri) if m else None)
            pc = _ptr(rgb) if colours and n else None
        if colours:
            self._chk(self.lib.dvo_colour_mesh_extract(self._h, volume, int(min_weight), px, pc, n, pt, m, C.byref(nv), C.byref(nt), flags))
            return xyz, tri, rgb
        self._chk(self.lib.dvo_mesh_extract(self._h, volume, int(min_weight), px, n, pt, m, C.byref(nv), C.byref(nt), flags))
        return xyz, tri

    def enable_esdf(self):
        """dvo_esdf_enable: the handle gets its distance-field pool (4 bytes per voxel of max_voxels_total); a second call changes nothing"""
        self._chk(self.lib.dvo_esdf_enable(self._h))

    def update_esdf(self, volumes: Sequence[int], params: Optional["DvoEsdfParams"] = None):
        """dvo_esdf_update: the Euclidean distance fields of the listed volumes from their words as they are now:
        DVO_ESDF_UPDATE_LAUNCHES launches and one synchronisation for the whole list"""
        volumes = [int(q) for q in volumes]
        v = (C.c_int * max(len(volumes), 1))(*volumes)
        p = params if params is not None else DvoEsdfParams.default()
        self._chk(self.lib.dvo_esdf_update(self._h, C.byref(p), len(volumes), v))

    def esdf_words(self, volume: int) -> np.ndarray:
        """dvo_esdf_get_words: the volume's nx * ny * nz ESDF words (uint32: d2 in bits 0..23, inside in bit 30, not observed in bit 31)"""
        n = self._n(volume)
        out = np.zeros(n, np.uint32)
        self._chk(self.lib.dvo_esdf_get_words(self._h, volume, _ptr(out)))
        return out

    def esdf_distances(self, volume: int, iz0: int = 0, nz: Optional[int] = None, device: bool = False):
        """dvo_esdf_get_distances: metres (float32, negative inside) of the nz z-planes from iz0 (nz None: all of them), nz * ny * nx
        values in index order, converted on the device in one launch.  device=True: a torch tensor on the handle's GPU, written in place"""
        self._n(volume)
        dims = self._dims[volume]
        nz = dims[2] if nz is None else int(nz)
        count = max(nz, 0) * dims[0] * dims[1]
        if device:
            import torch
            out = torch.zeros(max(count, 1), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            self._chk(self.lib.dvo_esdf_get_distances(self._h, volume, int(iz0), int(nz), int(out.data_ptr()), DVO_UPLOAD_DEVICE))
            return out[:count]
        out = np.zeros(max(count, 1), np.float32)
        self._chk(self.lib.dvo_esdf_get_distances(self._h, volume, int(iz0), int(nz), _ptr(out), 0))
        return out[:count]

    def esdf_query(self, volume: int, points, device: bool = False):
        """dvo_esdf_query: the batched point query, one launch.  points: (n, 3) float64 world coordinates; returns n records of
        ESDF_SAMPLE_DTYPE.  device=True: points is a contiguous float64 torch tensor on the handle's GPU and the result a uint8 tensor
        of n * 40 bytes there (view it as ESDF_SAMPLE_DTYPE after a copy to the host)"""
        if device:
            import torch
            n = points.numel() // 3
            out = torch.zeros(max(n, 1) * ESDF_SAMPLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            self._chk(self.lib.dvo_esdf_query(self._h, volume, n, int(points.data_ptr()), int(out.data_ptr()), DVO_UPLOAD_DEVICE))
            return out[:n * ESDF_SAMPLE_DTYPE.itemsize]
        P = _esdf_points(points)
        out = np.zeros(len(P), ESDF_SAMPLE_DTYPE)
        self._chk(self.lib.dvo_esdf_query(self._h, volume, len(P), _ptr(P), _ptr(out), 0))
        return out

    def stats(self):
        """(kernel launches, host synchronisations) of the last integrate, points, raycast or extract_mesh call, colour variants included,
        or of the last update_esdf, esdf_distances or esdf_query"""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.dvo_tsdf_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _icp_host_views(now_depth, model_depth, model_normals):
    """host images of a view list: (kept arrays, three pointer lists, now format, model format, rows, cols)"""
    now, nptr, nfmt, rows, cols = _tsdf_host_images(list(now_depth))
    model, mptr, mfmt, mrows, mcols = _tsdf_host_images(list(model_depth))
    nrm = [np.ascontiguousarray(a, dtype=np.float32) for a in model_normals]
    if len(model) != len(now) or len(nrm) != len(now) or (mrows, mcols) != (rows, cols) or any(a.shape != (rows, cols, 3) for a in nrm):
        raise ValueError("one model depth image and one (rows, cols, 3) float32 normal image per now image, all of the same rows x cols")
    return (now, model, nrm), nptr, mptr, (C.c_void_p * max(len(nrm), 1))(*[a.ctypes.data for a in nrm]), nfmt, mfmt, rows, cols


def _icp_poses(model_poses, start_poses, n):
    _, _, _, Pm = _tsdf_frames([None] * n, (1.0, 1.0, 0.0, 0.0), model_poses)
    _, _, _, Ps = _tsdf_frames([None] * n, (1.0, 1.0, 0.0, 0.0), start_poses)
    return Pm, Ps


def _icp_host_now_normals(now_normals, n, rows, cols):
    """host now normals of a gated call: (kept arrays, pointer list)"""
    g = [np.ascontiguousarray(a, dtype=np.float32) for a in now_normals]
    if len(g) != n or any(a.shape != (rows, cols, 3) for a in g):
        raise ValueError("one (rows, cols, 3) float32 now-normal image per now image")
    return g, (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in g])


def icp_align_host(now_depth, model_depth, model_normals, K4, model_poses, start_poses, params: Optional["DvoIcpParams"] = None,
                   now_normals=None, normal_cos_min: float = 0.0):
    """dvo_icp_align_host: the definition of the frame-to-model alignment on the host, no device needed.  One view per now image: host
    arrays (uint16 millimetres or float32 metres; the now and the model images may differ in format), normals (rows, cols, 3) float32;
    K4 one fx, fy, cx, cy for all views or one per view; poses (n, 12) {R column-major, t} or (n, 3, 4).  now_normals: one (rows, cols,
    3) float32 image per view in the now camera's axes (icp_prepare_host's) -- dvo_icp_align_gated_host: a pair whose model normal and
    rotated now normal have a dot product below normal_cos_min is skipped.  Returns (poses (n, 12), records: n entries of
    ICP_RECORD_DTYPE)"""
    keep, nptr, mptr, qptr, nfmt, mfmt, rows, cols = _icp_host_views(now_depth, model_depth, model_normals)
    _, n, K, _ = _tsdf_frames(keep[0], K4, np.zeros((len(keep[0]), 12)))
    Pm, Ps = _icp_poses(model_poses, start_poses, n)
    poses, rec = np.zeros((n, 12), np.float64), np.zeros(n, ICP_RECORD_DTYPE)
    p = params if params is not None else DvoIcpParams.default()
    if now_normals is not None:
        gate, gptr = _icp_host_now_normals(now_normals, n, rows, cols)
        rc = load_library().dvo_icp_align_gated_host(C.byref(p), n, nfmt, mfmt, rows, cols, _ptr(K), nptr, mptr, qptr, _ptr(Pm), _ptr(Ps), gptr,
                                                     float(normal_cos_min), _ptr(poses), _ptr(rec))
        del gate
    else:
        rc = load_library().dvo_icp_align_host(C.byref(p), n, nfmt, mfmt, rows, cols, _ptr(K), nptr, mptr, qptr, _ptr(Pm), _ptr(Ps), _ptr(poses), _ptr(rec))
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_icp_align_host refused its arguments")
    return poses, rec


def icp_prepare_host(depth, K4, params: Optional["DvoIcpPrepareParams"] = None, normals: bool = True):
    """dvo_icp_prepare_host: the definition of the depth front end on the host, no device needed.  depth: same-shape (rows, cols) host
    arrays, all uint16 millimetres or all float32 metres; K4 one fx, fy, cx, cy for all images or one per image.  Returns (filtered:
    a list of (rows, cols) float32 metres, 0 = a hole; normals: a list of (rows, cols, 3) float32 in the now camera's axes, (0, 0, 0) =
    none) or, with normals=False, the filtered list alone"""
    imgs, ptrs, fmt, rows, cols = _tsdf_host_images(list(depth))
    _, n, K, _ = _tsdf_frames(imgs, K4, np.zeros((len(imgs), 12)))
    out = [np.zeros((rows, cols), np.float32) for _ in range(n)]
    nrm = [np.zeros((rows, cols, 3), np.float32) for _ in range(n)] if normals else None
    p = params if params is not None else DvoIcpPrepareParams.default()
    optr = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in out])
    qptr = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in nrm]) if normals else None
    rc = load_library().dvo_icp_prepare_host(C.byref(p), n, fmt, rows, cols, _ptr(K), ptrs, optr, qptr)
    if rc != DVO_OK:
        raise DvoError(rc, "dvo_icp_prepare_host refused its arguments")
    return (out, nrm) if normals else out


def icp_information_right(info, pose12) -> np.ndarray:
    """dvo_icp_record.info -- tangent order (v, w) of a world-frame LEFT increment of the now frame's pose -- in the pose graphs'
    convention, order [translation, rotation] of a RIGHT (body-frame) increment T <- T Exp(d): Ad^T info Ad with Ad = [[R, [t]x R],
    [0, R]] of pose12 = {R column-major, t}, the pose the alignment returned (x = Ad d to first order).  With the record's sum_r2 and
    count it is what graph_information takes as H for an edge from the model view's node to the now frame's"""
    H = np.asarray(info, dtype=np.float64).reshape(6, 6)
    P = np.asarray(pose12, dtype=np.float64).reshape(12)
    R, t = P[:9].reshape(3, 3).T, P[9:]
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ad = np.zeros((6, 6))
    Ad[:3, :3], Ad[:3, 3:], Ad[3:, 3:] = R, tx @ R, R
    out = Ad.T @ H @ Ad
    return 0.5 * (out + out.T)


class DvoIcp:
    """A dvo_icp_batch (include/dvo_amd.h, "frame-to-model alignment"): projective point-to-plane ICP of up to max_views depth frames
    against ray-cast model views per call.  Stand-alone: no DvoContext, no tracker, no DvoTsdfVolumes."""

    def __init__(self, max_views: int):
        self.lib = load_library()
        self._h = C.c_void_p()
        rc = self.lib.dvo_icp_create(max_views, C.byref(self._h))
        if rc != DVO_OK:
            self._h = C.c_void_p()
            raise DvoError(rc, self.lib.dvo_icp_last_error(None).decode())

    def _chk(self, rc: int):
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_icp_last_error(self._h).decode())

    def close(self):
        if self._h:
            self.lib.dvo_icp_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, depth, K4, params: Optional["DvoIcpPrepareParams"] = None, normals: bool = True, device: bool = False):
        """dvo_icp_prepare: the bilateral filter and the now-frame normals of every listed image in two launches (one without normals) and
        one synchronisation.  Host arrays as icp_prepare_host takes them, returned as it returns them; device=True: contiguous torch
        tensors on the handle's GPU (16-bit depth as int16: the same bits), read in place -- the outputs are new torch tensors on the
        GPU, float32 (rows, cols) and (rows, cols, 3), ready for align(..., now_normals=..., device=True) and
        DvoTsdfVolumes.integrate(..., device=True); nothing is copied back"""
        if device:
            import torch
            src = list(depth)
            shape = tuple(src[0].shape)
            if len(shape) != 2 or any(not d.is_contiguous() or tuple(d.shape) != shape or d.element_size() != src[0].element_size() for d in src):
                raise ValueError("device images: contiguous, all of one (rows, cols) and format")
            n, rows, cols = len(src), int(shape[0]), int(shape[1])
            dfmt = DVO_DEPTH_U16 if src[0].element_size() == 2 else DVO_DEPTH_F32
            out = [torch.zeros((rows, cols), dtype=torch.float32, device=src[0].device) for _ in range(n)]
            nrm = [torch.zeros((rows, cols, 3), dtype=torch.float32, device=src[0].device) for _ in range(n)] if normals else None
            torch.cuda.synchronize()
            ptrs = (C.c_void_p * max(n, 1))(*[int(d.data_ptr()) for d in src])
            optr = (C.c_void_p * max(n, 1))(*[int(a.data_ptr()) for a in out])
            qptr = (C.c_void_p * max(n, 1))(*[int(a.data_ptr()) for a in nrm]) if normals else None
            keep = src
        else:
            keep, ptrs, dfmt, rows, cols = _tsdf_host_images(list(depth))
            n = len(keep)
            out = [np.zeros((rows, cols), np.float32) for _ in range(n)]
            nrm = [np.zeros((rows, cols, 3), np.float32) for _ in range(n)] if normals else None
            optr = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in out])
            qptr = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in nrm]) if normals else None
        _, n, K, _ = _tsdf_frames([None] * n, K4, np.zeros((n, 12)))
        self._chk(self.lib.dvo_icp_prepare(self._h, C.byref(params) if params is not None else None, n, dfmt, rows, cols, _ptr(K), ptrs, optr, qptr,
                                           DVO_UPLOAD_DEVICE if device else 0))
        del keep
        return (out, nrm) if normals else out

    def align(self, now_depth, model_depth, model_normals, K4, model_poses, start_poses, params: Optional["DvoIcpParams"] = None,
              device: bool = False, now_normals=None, normal_cos_min: float = 0.0):
        """dvo_icp_align, or dvo_icp_align_gated with now_normals (one (rows, cols, 3) float32 image per view in the now camera's axes:
        what prepare returns; a pair whose model normal and rotated now normal have a dot product below normal_cos_min is skipped):
        view i -- now_depth[i] against model_depth[i] and model_normals[i] seen from model_poses[i], started at
        start_poses[i] -- all views in one call: two launches per sweep, one synchronisation.  Host arrays as icp_align_host takes
        them; device=True: torch tensors on the handle's GPU, read in place (16-bit depth as int16: the same bits) -- what
        DvoTsdfVolumes.raycast(..., normals=True, device=True) returns.  Returns (poses (n, 12), records: n entries of ICP_RECORD_DTYPE)"""
        if device:
            now, model, nrm = list(now_depth), list(model_depth), list(model_normals)
            shape = tuple(now[0].shape)
            if len(shape) != 2 or len(model) != len(now) or len(nrm) != len(now):
                raise ValueError("one model depth image and one normal image per now image")
            if any(not d.is_contiguous() or tuple(d.shape) != shape or d.element_size() != now[0].element_size() for d in now) or \
               any(not d.is_contiguous() or tuple(d.shape) != shape or d.element_size() != model[0].element_size() for d in model) or \
               any(not a.is_contiguous() or tuple(a.shape) != shape + (3,) or a.element_size() != 4 for a in nrm):
                raise ValueError("device images: contiguous, depth all of one (rows, cols) and format per list, normals (rows, cols, 3) float32")
            keep = (now, model, nrm)
            n = len(now)
            lists = [(C.c_void_p * max(n, 1))(*[int(d.data_ptr()) for d in lst]) for lst in keep]
            nptr, mptr, qptr = lists
            if now_normals is not None:
                gate = list(now_normals)
                if len(gate) != n or any(not a.is_contiguous() or tuple(a.shape) != shape + (3,) or a.element_size() != 4 for a in gate):
                    raise ValueError("device now normals: one contiguous (rows, cols, 3) float32 image per view")
                gptr = (C.c_void_p * max(n, 1))(*[int(a.data_ptr()) for a in gate])
            nfmt = DVO_DEPTH_U16 if now[0].element_size() == 2 else DVO_DEPTH_F32
            mfmt = DVO_DEPTH_U16 if model[0].element_size() == 2 else DVO_DEPTH_F32
            rows, cols = int(shape[0]), int(shape[1])
        else:
            keep, nptr, mptr, qptr, nfmt, mfmt, rows, cols = _icp_host_views(now_depth, model_depth, model_normals)
            n = len(keep[0])
            if now_normals is not None:
                gate, gptr = _icp_host_now_normals(now_normals, n, rows, cols)
        _, n, K, _ = _tsdf_frames([None] * n, K4, np.zeros((n, 12)))
        Pm, Ps = _icp_poses(model_poses, start_poses, n)
        poses, rec = np.zeros((n, 12), np.float64), np.zeros(n, ICP_RECORD_DTYPE)
        if now_normals is not None:
            self._chk(self.lib.dvo_icp_align_gated(self._h, C.byref(params) if params is not None else None, n, nfmt, mfmt, rows, cols, _ptr(K), nptr, mptr,
                                                   qptr, _ptr(Pm), _ptr(Ps), gptr, float(normal_cos_min), _ptr(poses), _ptr(rec),
                                                   DVO_UPLOAD_DEVICE if device else 0))
            del gate
        else:
            self._chk(self.lib.dvo_icp_align(self._h, C.byref(params) if params is not None else None, n, nfmt, mfmt, rows, cols, _ptr(K), nptr, mptr, qptr,
                                             _ptr(Pm), _ptr(Ps), _ptr(poses), _ptr(rec), DVO_UPLOAD_DEVICE if device else 0))
        del keep
        return poses, rec

    def stats(self):
        """(kernel launches, host synchronisations) of the last align or prepare"""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.dvo_icp_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def jet_colour(i: int):
    """(B, G, R) of entry i of the 64-entry jet map the residue heat map is coloured with (FColorMap), from its closed form"""
    r = lambda j: 0 if j <= 0 else min(255, 16 * j - 1)
    return min(r(i + 9), r(39 - i)), min(r(i - 7), r(55 - i)), min(r(i - 23), r(71 - i))


class DvoTracker:
    """K camera streams tracked like dvo_amd::SolveDVO tracks one (include/dvo_amd.h, "many camera streams").

    step(streams, bgr_list, depth_list) advances the listed streams by one frame each and returns (R, t, event): R (n, 3, 3) and
    t (n, 3) the key-frame relative poses, event (n,) 0 ordinary / 1 first frame / 2..5 reasonForChange of a key-frame switch."""

    def __init__(self, max_streams: int, params: Optional[DvoParams] = None, iters: Optional[Sequence[int]] = None,
                 key_frame_every: int = 5, adaptive: bool = False, laplacian_b_thresh: float = 3.0,
                 visible_ratio_thresh: float = 0.8, min_points: int = 50, rows: int = 480, cols: int = 640, n_levels: int = 4,
                 first_shift: int = 1, points_capacity: Optional[Sequence[int]] = None):
        self.lib = load_library()
        self._h = None
        tp = DvoTrackerParams()
        self.lib.dvo_tracker_params_default(C.byref(tp))
        if iters is not None:
            for l in range(DVO_MAX_LEVELS):
                tp.iters[l] = int(iters[l]) if l < len(iters) else 0
        for l, v in enumerate(points_capacity or []):
            tp.points_capacity[l] = int(v)
        tp.key_frame_every, tp.adaptive = key_frame_every, int(bool(adaptive))
        tp.laplacian_b_thresh, tp.visible_ratio_thresh, tp.min_points = laplacian_b_thresh, visible_ratio_thresh, min_points
        tp.rows, tp.cols, tp.n_levels, tp.first_shift = rows, cols, n_levels, first_shift
        self.params, self.max_streams, self.n_levels = tp, max_streams, n_levels
        self._depth_shapes = {}  # stream -> (depth_rows, depth_cols) of its depth rig: what step_raw_depth checks host arrays against
        h = C.c_void_p()
        rc = self.lib.dvo_tracker_create(C.byref(params) if params is not None else None, max_streams, C.byref(tp), C.byref(h))
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_tracker_last_error(None).decode())
        self._h = h

    def _chk(self, rc: int):
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_tracker_last_error(self._h).decode())

    def close(self):
        if self._h is not None:
            self.lib.dvo_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_intrinsics(self, fx, fy, cx, cy):
        self._chk(self.lib.dvo_tracker_set_intrinsics(self._h, fx, fy, cx, cy))

    def reset_stream(self, stream: int):
        self._chk(self.lib.dvo_tracker_reset_stream(self._h, stream))

    def set_stream_intrinsics(self, stream: int, fx, fy, cx, cy):
        """the stream's own camera model (only before its first frame, or after reset_stream)"""
        self._chk(self.lib.dvo_tracker_set_stream_intrinsics(self._h, stream, fx, fy, cx, cy))

    def set_stream_undistort(self, stream: int, K4=None, D5=None):
        """cv::undistort of the stream's frames with K4 = (fx, fy, cx, cy), D5 = (k1, k2, p1, p2, k3); both None: none for this stream"""
        K = np.ascontiguousarray(K4, dtype=np.float64) if K4 is not None else None
        D = np.ascontiguousarray(D5, dtype=np.float64) if D5 is not None else None
        if (K is not None and K.size != 4) or (D is not None and D.size != 5):
            raise ValueError("K4 has 4 entries, D5 has 5")
        self._chk(self.lib.dvo_tracker_set_stream_undistort(self._h, stream, _ptr(K), _ptr(D)))

    def set_stream_mask(self, stream: int, mask, margin: int = 2):
        """ignore mask of the stream (-1: every stream): (rows, cols) of the tracker, non-zero = ignore; None removes it.  Allowed at
        any time, takes effect with the stream's next frame; reset_stream keeps it"""
        m = None if mask is None else _mask_bytes(mask)
        if m is not None and m.shape != (self.params.rows, self.params.cols):
            raise ValueError("the mask must have the tracker's rows x cols")
        self._chk(self.lib.dvo_tracker_set_stream_mask(self._h, stream, _ptr(m), margin))

    def set_stream_depth_rig(self, stream: int, rig: Optional[DvoDepthRig]):
        """depth rig of the stream for step_raw_depth (only before its first frame, or after reset_stream); None removes it.  Kc4 / Dc5
        of the rig are the caller's to keep consistent with set_stream_undistort"""
        self._chk(self.lib.dvo_tracker_set_stream_depth_rig(self._h, stream, None if rig is None else C.byref(rig)))
        self._depth_shapes[stream] = None if rig is None else (rig.depth_rows, rig.depth_cols)

    def step_raw_depth(self, streams: Sequence[int], image_list, depth_list, flags: int = 0, rgb: bool = False,
                       image_format: int = DVO_CAM_BGR8, depth_format: int = DVO_DEPTH_U16):
        """step() for UNREGISTERED depth: depth_list[i] is the raw depth image of streams[i] in the geometry of the stream's rig (uint16
        millimetres, or float metres), registered to the colour camera on the device.  Host arrays, or with DVO_UPLOAD_DEVICE addresses
        (ints) in image_format / depth_format"""
        n = len(streams)
        S = (C.c_int * n)(*[int(s) for s in streams])
        keep = None
        if flags & DVO_UPLOAD_DEVICE:
            B = (C.c_void_p * n)(*[int(p) for p in image_list])
            D = (C.c_void_p * n)(*[int(p) for p in depth_list])
            rows, cols = self.params.rows, self.params.cols
        else:
            image_format, bl, _, _ = _camera_arrays(image_list, None, rgb, 0)
            dl = [np.asarray(d) for d in depth_list]
            u16 = n > 0 and all(d.dtype == np.uint16 for d in dl)
            dl = [np.ascontiguousarray(d, dtype=np.uint16 if u16 else np.float32) for d in dl]
            for s_, d in zip(streams, dl):                       # the library reads depth_rows x depth_cols values behind each pointer
                shape = self._depth_shapes.get(int(s_))
                if shape is not None and d.shape != shape:
                    raise ValueError("the raw depth image of stream %d must have its rig's depth_rows x depth_cols %s" % (s_, shape))
            depth_format = DVO_DEPTH_U16 if u16 else DVO_DEPTH_F32
            B = (C.c_void_p * n)(*[b.ctypes.data for b in bl])
            D = (C.c_void_p * n)(*[d.ctypes.data for d in dl])
            rows, cols = bl[0].shape[:2] if n else (0, 0)
            keep = (bl, dl)
        Rc, t, ev = self._outputs(n)
        self._chk(self.lib.dvo_tracker_step_raw_depth(self._h, n, S, B, image_format, D, depth_format, rows, cols, flags, _ptr(Rc), _ptr(t),
                                                      ev.ctypes.data_as(C.POINTER(C.c_int))))
        del keep
        return np.transpose(Rc, (0, 2, 1)).copy(), t, ev

    def clear_stream_camera(self, stream: int):
        """back to the handle-wide intrinsics and undistortion"""
        self._chk(self.lib.dvo_tracker_clear_stream_camera(self._h, stream))

    def _outputs(self, n):
        return np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)

    def step(self, streams: Sequence[int], bgr_list, depth_list, flags: int = 0, rgb: bool = False,
             image_format: int = DVO_CAM_BGR8, depth_format: int = DVO_DEPTH_F32):
        """bgr_list / depth_list: (rows, cols, 3) uint8 and (rows, cols) float32 metres per listed stream (host arrays), or, with
        flags DVO_UPLOAD_DEVICE / DVO_UPLOAD_MAPPED, their addresses (ints).  Host arrays name their format themselves: (rows, cols)
        uint8 images are mono8, rgb=True marks RGB8, uint16 depth is 16-bit millimetres; image_format / depth_format (DVO_CAM_* /
        DVO_DEPTH_*) say what lies behind addresses"""
        n = len(streams)
        S = (C.c_int * n)(*[int(s) for s in streams])
        if flags & (DVO_UPLOAD_DEVICE | DVO_UPLOAD_MAPPED):
            B = (C.c_void_p * n)(*[int(p) for p in bgr_list])
            D = (C.c_void_p * n)(*[int(p) for p in depth_list])
            rows, cols = self.params.rows, self.params.cols
            keep = None
        else:
            image_format, bl, depth_format, dl = _camera_arrays(bgr_list, depth_list, rgb, 0)
            B = (C.c_void_p * n)(*[b.ctypes.data for b in bl])
            D = (C.c_void_p * n)(*[d.ctypes.data for d in dl])
            rows, cols = bl[0].shape[:2] if n else (0, 0)
            keep = (bl, dl)
        Rc, t, ev = self._outputs(n)
        if (image_format, depth_format) == (DVO_CAM_BGR8, DVO_DEPTH_F32):
            self._chk(self.lib.dvo_tracker_step(self._h, n, S, B, D, rows, cols, flags, _ptr(Rc), _ptr(t),
                                                ev.ctypes.data_as(C.POINTER(C.c_int))))
        else:
            self._chk(self.lib.dvo_tracker_step_fmt(self._h, n, S, B, image_format, D, depth_format, rows, cols, flags, _ptr(Rc), _ptr(t),
                                                    ev.ctypes.data_as(C.POINTER(C.c_int))))
        del keep
        return np.transpose(Rc, (0, 2, 1)).copy(), t, ev

    def step_pyramids(self, streams: Sequence[int], frames, flags: int = 0):
        """frames[i] = list over levels of (grey uint8, depth uint16 mm) row-major 2-D arrays of stream streams[i]"""
        n, nl = len(streams), self.n_levels
        S = (C.c_int * n)(*[int(s) for s in streams])
        G, Dm, keep = (DvoImage * max(n * nl, 1))(), (DvoImage * max(n * nl, 1))(), []
        for i, fr in enumerate(frames):
            for l, (g, d) in enumerate(fr):
                G[i * nl + l], b = DvoContext._image(g, "grey", DVO_LAYOUT_ROW_MAJOR); keep.append(b)
                Dm[i * nl + l], b = DvoContext._image(d, "depth", DVO_LAYOUT_ROW_MAJOR); keep.append(b)
        Rc, t, ev = self._outputs(n)
        self._chk(self.lib.dvo_tracker_step_pyramids(self._h, n, S, G, Dm, flags, _ptr(Rc), _ptr(t),
                                                     ev.ctypes.data_as(C.POINTER(C.c_int))))
        del keep
        return np.transpose(Rc, (0, 2, 1)).copy(), t, ev

    def signals(self, stream: int):
        """(b_cap, visible_ratio, n_points) of the stream's last first alignment (np.float32, np.float32, int)"""
        b, r, n = C.c_float(), C.c_float(), C.c_int()
        self._chk(self.lib.dvo_tracker_get_signals(self._h, stream, C.byref(b), C.byref(r), C.byref(n)))
        return np.float32(b.value), np.float32(r.value), n.value

    def set_information(self, on: bool = True):
        """the 6x6 information matrix with every pose of the steps that follow (off by default): one more launch per step, no
        more host synchronisations"""
        self._chk(self.lib.dvo_tracker_set_information(self._h, int(bool(on))))

    def information(self, stream: int) -> dict:
        """H (6, 6) = sum w J J^T, g (6,) = J^T W eps, sum_eps2, n_visible and level at the pose the stream's last step returned;
        component order [translation x, y, z, rotation x, y, z].  A first frame (event 1) has the zero record with level -1"""
        H, g = np.zeros((6, 6)), np.zeros(6)
        e2, nv, lv = C.c_double(), C.c_int(), C.c_int()
        self._chk(self.lib.dvo_tracker_get_information(self._h, stream, _ptr(H), _ptr(g), C.byref(e2), C.byref(nv), C.byref(lv)))
        return dict(H=H, g=g, sum_eps2=e2.value, n_visible=nv.value, level=lv.value)

    def covariance(self, stream: int):
        """pose_covariance of the stream's record: (6, 6), or None (fewer than 7 visible points, H not positive definite)"""
        r = self.information(stream)
        return pose_covariance(r["H"], r["sum_eps2"], r["n_visible"])

    def set_views(self, on: bool = True):
        """the reference's debug views for the steps that follow (off by default): the reprojections on the distance transform, the
        residue heat map and the residue histogram of every listed stream, DVO_TRACKER_VIEW_LAUNCHES more launches per rendering, no
        more host synchronisations; the images stay on the device until view() asks for one"""
        self._chk(self.lib.dvo_tracker_set_views(self._h, int(bool(on))))

    def view_size(self):
        """(rows, cols, level) of the views: the finest level that runs"""
        r, c, l = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.dvo_tracker_view_size(self._h, C.byref(r), C.byref(c), C.byref(l)))
        return r.value, c.value, l.value

    def residue_histogram(self, stream: int) -> dict:
        """hist (260,) uint32 with hist[int(eps_i) + 1] counted over the stream's reference points at the pose its last step returned,
        n_points (= hist.sum()) and level.  A first frame (event 1) has the zero record with level -1"""
        hist = np.zeros(DVO_VIEW_HISTOGRAM_BINS, np.uint32)
        n, lv = C.c_int(), C.c_int()
        self._chk(self.lib.dvo_tracker_get_residue_histogram(self._h, stream, _ptr(hist), C.byref(n), C.byref(lv)))
        return dict(hist=hist, n_points=n.value, level=lv.value)

    def view(self, stream: int, which: int) -> np.ndarray:
        """the stream's view `which` (DVO_VIEW_REPROJ_ON_DT / DVO_VIEW_RESIDUE_HEAT) of its last step: (rows, cols, 3) uint8, B G R"""
        rows, cols, _ = self.view_size()
        img = np.zeros((rows, cols, 3), np.uint8)
        self._chk(self.lib.dvo_tracker_get_view(self._h, stream, which, _ptr(img)))
        return img

    def view_device(self, stream: int, which: int) -> int:
        """device address of the resident image view() copies, valid until the stream's next step"""
        d = C.c_void_p()
        self._chk(self.lib.dvo_tracker_view_device(self._h, stream, which, C.byref(d)))
        return d.value

    # ---- key-frame archive and loop-closure alignment (include/dvo_amd.h) ----
    def set_archive(self, capacity: int, max_matches: int = 1, points_capacity: Optional[Sequence[int]] = None):
        """keep the key frames of the steps that follow in a ring of `capacity` slots in HBM (0: off); match() takes up to max_matches
        candidates; points_capacity[l]: longest list of level l a slot holds (0 / None: rows_l * cols_l / 8)"""
        pc = (C.c_int * DVO_MAX_LEVELS)(*([int(v) for v in points_capacity] + [0] * (DVO_MAX_LEVELS - len(points_capacity)))) \
            if points_capacity is not None else None
        self._chk(self.lib.dvo_tracker_set_archive(self._h, int(capacity), int(max_matches), pc))

    def key_frame_id(self, stream: int) -> int:
        """id of the stream's current key frame in the archive, -1 if it is not archived"""
        v = C.c_longlong()
        self._chk(self.lib.dvo_tracker_key_frame_id(self._h, stream, C.byref(v)))
        return v.value

    def archive_info(self, key_id: int) -> dict:
        s, f = C.c_int(), C.c_longlong()
        n = (C.c_int * DVO_MAX_LEVELS)()
        self._chk(self.lib.dvo_tracker_archive_info(self._h, int(key_id), C.byref(s), C.byref(f), n))
        return dict(stream=s.value, frame=f.value, n_points=[n[l] for l in range(self.n_levels)])

    def archive_points(self, key_id: int, level: int) -> np.ndarray:
        """(N, 3) float32: the archived reference list of `level`, as dvo_get_ref_level gave it when the key frame was made"""
        n = C.c_int()
        self._chk(self.lib.dvo_tracker_archive_get_points(self._h, int(key_id), level, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32)
        self._chk(self.lib.dvo_tracker_archive_get_points(self._h, int(key_id), level, _ptr(xyz), n.value, C.byref(n)))
        return xyz

    def archive_stats(self) -> dict:
        a, r, e = C.c_longlong(), C.c_longlong(), C.c_longlong()
        l, s = C.c_int(), C.c_int()
        self._chk(self.lib.dvo_tracker_archive_stats(self._h, C.byref(a), C.byref(r), C.byref(e), C.byref(l), C.byref(s)))
        return dict(archived=a.value, refused=r.value, evicted=e.value, last_launches=l.value, last_syncs=s.value)

    @staticmethod
    def _records(rec, n):
        return [dict(H=np.array(rec[i].H36).reshape(6, 6), g=np.array(rec[i].g6), sum_eps2=rec[i].sum_eps2, n_points=rec[i].n_points,
                     n_visible=rec[i].n_visible) for i in range(n)]

    def _candidates(self, streams, key_ids, R, t):
        n = len(streams)
        S = (C.c_int * max(n, 1))(*[int(s) for s in streams])
        I = (C.c_longlong * max(n, 1))(*[int(k) for k in key_ids])
        Rc = np.ascontiguousarray(np.transpose(np.asarray(R, np.float64).reshape(-1, 3, 3), (0, 2, 1)))      # column-major, as step()
        tc = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1, 3))
        if len(key_ids) != n or Rc.shape[0] != n or tc.shape[0] != n:
            raise ValueError("streams, key_ids, R and t must list the same candidates")
        return n, S, I, Rc, tc, (DvoTrackerScoreRecord * max(n, 1))()

    def score(self, streams: Sequence[int], key_ids: Sequence[int], level: int, R, t) -> list:
        """per candidate i: archived key frame key_ids[i] against the current now frame of streams[i] at the pose (R[i], t[i]) (as step()
        returns them) on the points of `level`: dict(H, g, sum_eps2, n_points, n_visible).  One launch, one synchronisation"""
        n, S, I, Rc, tc, rec = self._candidates(streams, key_ids, R, t)
        self._chk(self.lib.dvo_tracker_score(self._h, n, S, I, level, _ptr(Rc), _ptr(tc), rec))
        return self._records(rec, n)

    def match(self, streams: Sequence[int], key_ids: Sequence[int], R0=None, t0=None):
        """the tracker's level schedule for every candidate from the guess (R0[i], t0[i]) (default: the identity): (R, t, records) with the
        records at the resulting poses on the finest level that ran.  Tracking is not disturbed"""
        n = len(streams)
        R0 = np.tile(np.eye(3), (n, 1, 1)) if R0 is None else R0
        t0 = np.zeros((n, 3)) if t0 is None else t0
        n, S, I, Rc, tc, rec = self._candidates(streams, key_ids, R0, t0)
        Ro, to = np.zeros((max(n, 1), 3, 3)), np.zeros((max(n, 1), 3))
        self._chk(self.lib.dvo_tracker_match(self._h, n, S, I, _ptr(Rc), _ptr(tc), _ptr(Ro), _ptr(to), rec))
        return np.transpose(Ro[:n], (0, 2, 1)).copy(), to[:n], self._records(rec, n)

    # ---- place descriptors and top-k key-frame retrieval (include/dvo_amd.h) ----
    def set_places(self, level: Optional[int] = None):
        """one place descriptor (brightness-normalised grey image of pyramid level `level`; None: the coarsest) per key frame archived
        from now on; -1: off.  Needs the archive; DVO_TRACKER_PLACE_STORE_LAUNCHES more launch per store, no more synchronisations"""
        self._chk(self.lib.dvo_tracker_set_places(self._h, self.n_levels - 1 if level is None else int(level)))

    def archive_descriptor(self, key_id: int) -> np.ndarray:
        """(D,) uint8: the descriptor stored with the archived key frame, D = rows * cols of the descriptor level, column-major"""
        n = C.c_int()
        self._chk(self.lib.dvo_tracker_archive_get_descriptor(self._h, int(key_id), None, 0, C.byref(n)))
        d = np.zeros(n.value, np.uint8)
        self._chk(self.lib.dvo_tracker_archive_get_descriptor(self._h, int(key_id), d.ctypes.data_as(C.POINTER(C.c_ubyte)), n.value, C.byref(n)))
        return d

    def places_raw(self, streams: Sequence[int], k: int, min_frame_gap: int = 0):
        """dvo_tracker_query_places as it is: the (n, k) array of DvoTrackerPlace records, unused entries included, and n_found (n,)"""
        n = len(streams)
        S = (C.c_int * max(n, 1))(*[int(s) for s in streams])
        out = (DvoTrackerPlace * max(n * max(int(k), 0), 1))()
        found = (C.c_int * max(n, 1))()
        self._chk(self.lib.dvo_tracker_query_places(self._h, n, S, int(k), int(min_frame_gap), out, found))
        rec = np.frombuffer(out, dtype=np.dtype(DvoTrackerPlace), count=n * k).reshape(n, k).copy()
        return rec, np.array(found[:n], np.int32)

    def places(self, streams: Sequence[int], k: int, min_frame_gap: int = 0) -> list:
        """per listed stream the up to k archived key frames whose descriptors are nearest to the stream's current frame, ordered by
        (distance, key_id): a list of lists of dict(key_id, frame, stream, distance).  Never returned: key frames under another camera
        model, the stream's own current key frame, and its own key frames younger than min_frame_gap frames"""
        rec, found = self.places_raw(streams, k, min_frame_gap)
        return [[dict(key_id=int(r["key_id"]), frame=int(r["frame"]), stream=int(r["stream"]), distance=int(r["distance"]))
                 for r in rec[i, :found[i]]] for i in range(len(streams))]

    # ---- shift search on place descriptors, and a pose guess from the shift (include/dvo_amd.h) ----
    PLACE_SHIFT_FIELDS = ("dy", "dx", "sad", "sad_zero", "sad_second", "area")

    def place_shifts_raw(self, streams: Sequence[int], key_ids: Sequence[int], radius: int) -> np.ndarray:
        """dvo_tracker_place_shifts as it is: the (n,) array of DvoTrackerPlaceShift records"""
        n = len(streams)
        if len(key_ids) != n:
            raise ValueError("streams and key_ids must list the same candidates")
        S = (C.c_int * max(n, 1))(*[int(s) for s in streams])
        I = (C.c_longlong * max(n, 1))(*[int(k) for k in key_ids])
        rec = (DvoTrackerPlaceShift * max(n, 1))()
        self._chk(self.lib.dvo_tracker_place_shifts(self._h, n, S, I, int(radius), rec))
        return np.frombuffer(rec, dtype=np.dtype(DvoTrackerPlaceShift), count=n).copy()

    def place_shifts(self, streams: Sequence[int], key_ids: Sequence[int], radius: int) -> list:
        """per candidate i the integer shift, |dy|, |dx| <= radius, that best lays the descriptor of archived key frame key_ids[i] onto
        the current frame of streams[i] (what the key frame shows at (y, x) the current frame shows at (y + dy, x + dx)):
        dict(dy, dx, sad, sad_zero, sad_second, area).  One launch, one synchronisation; nothing but the records is written"""
        rec = self.place_shifts_raw(streams, key_ids, radius)
        return [{k: int(r[k]) for k in self.PLACE_SHIFT_FIELDS} for r in rec]

    def place_guess(self, stream: int, dy: int, dx: int):
        """(R0, t0) for match(): the smallest rotation that explains a shift of (dy, dx) pixels of the descriptor level, and t0 = 0.
        A first-order guess, not an estimate.  Host arithmetic only"""
        Rc, t0 = np.zeros((3, 3)), np.zeros(3)
        self._chk(self.lib.dvo_tracker_place_guess(self._h, int(stream), int(dy), int(dx), _ptr(Rc), _ptr(t0)))
        return Rc.T.copy(), t0

    # ---- depth verification of loop-closure candidates (include/dvo_amd.h) ----
    VERIFY_FIELDS = ("n_points", "n_visible", "n_depth", "n_agree", "n_front", "n_behind", "sum_abs_q4")

    def verify_params(self, **tolerances) -> DvoTrackerVerifyParams:
        """dvo_tracker_verify_params_default with the given fields (tol_mm, tol_rel, min_depth_mm, max_depth_mm) replaced"""
        p = DvoTrackerVerifyParams()
        self.lib.dvo_tracker_verify_params_default(C.byref(p))
        for k, v in tolerances.items():
            if k not in ("tol_mm", "tol_rel", "min_depth_mm", "max_depth_mm"):
                raise TypeError(f"unknown tolerance {k!r}")
            setattr(p, k, float(v))
        return p

    def verify(self, streams: Sequence[int], key_ids: Sequence[int], level: int, R, t, **tolerances) -> list:
        """per candidate i: the points of `level` of archived key frame key_ids[i], warped by the pose (R[i], t[i]) (as step() returns
        them), against the DEPTH of the current frame of streams[i]: dict(n_points, n_visible, n_depth, n_agree, n_front, n_behind,
        sum_abs_q4).  tolerances: tol_mm, tol_rel, min_depth_mm, max_depth_mm (none given: the library's defaults).  One launch, one
        synchronisation; nothing but the records is written"""
        n, S, I, Rc, tc, _ = self._candidates(streams, key_ids, R, t)
        rec = (DvoTrackerVerifyRecord * max(n, 1))()
        vp = C.byref(self.verify_params(**tolerances)) if tolerances else None
        self._chk(self.lib.dvo_tracker_verify(self._h, n, S, I, level, _ptr(Rc), _ptr(tc), vp, rec))
        return [{k: int(getattr(rec[i], k)) for k in self.VERIFY_FIELDS} for i in range(n)]

    # ---- export and import of the key-frame archive (include/dvo_amd.h) ----
    def _id_list(self, ids):
        if ids is None:
            return 0, None
        return len(ids), (C.c_longlong * max(len(ids), 1))(*[int(k) for k in ids])

    def export_size(self, ids: Optional[Sequence[int]] = None) -> int:
        """bytes of the blob export_archive(ids) returns"""
        n, I = self._id_list(ids)
        size = C.c_size_t()
        self._chk(self.lib.dvo_tracker_archive_export_size(self._h, n, I, C.byref(size)))
        return size.value

    def export_archive(self, ids: Optional[Sequence[int]] = None) -> bytes:
        """the archived key frames `ids`, in that order (None: every live one in ascending id), as one self-describing blob: what
        import_archive of any tracker with the same geometry takes.  One launch, one synchronisation"""
        n, I = self._id_list(ids)
        cap = self.export_size(ids)
        buf = np.zeros(max(cap, 1), np.uint8)
        size = C.c_size_t()
        self._chk(self.lib.dvo_tracker_archive_export(self._h, n, I, _ptr(buf), cap, C.byref(size)))
        return buf[:size.value].tobytes()

    def import_archive(self, blob) -> list:
        """the key frames of a blob into the next slots of the ring: their new ids in the blob's order, -1 for one the archive's
        points_capacity refuses.  Nothing changes unless the whole blob is valid.  Two launches, one synchronisation"""
        data = bytes(blob)
        n = C.c_int()
        try:
            cap = archive_blob_info(data)["n_key_frames"]
        except DvoError:
            cap = 0                                        # the import itself names the defect
        ids = (C.c_longlong * max(cap, 1))()
        self._chk(self.lib.dvo_tracker_archive_import(self._h, data, len(data), ids, cap, C.byref(n)))
        return [int(ids[k]) for k in range(min(cap, n.value))]

    def archive_origin(self, key_id: int) -> dict:
        """who made the key frame: dict(id, stream, frame) in the tracker that archived it first (itself, for a native one)"""
        o, s, f = C.c_longlong(), C.c_int(), C.c_longlong()
        self._chk(self.lib.dvo_tracker_archive_origin(self._h, int(key_id), C.byref(o), C.byref(s), C.byref(f)))
        return dict(id=o.value, stream=s.value, frame=f.value)

    def stats(self) -> dict:
        v = [C.c_int() for _ in range(5)]
        self._chk(self.lib.dvo_tracker_get_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("launches", "syncs", "runs", "key_frames", "slab_growths"), (x.value for x in v)))

    def context_handle(self) -> int:
        """the underlying dvo_ctx* (pair = stream)"""
        return self.lib.dvo_tracker_context(self._h)


class DvoPhotoStreams:
    """K camera streams on the photometric engine, each run as dvo_amd::RGBDOdometry::processFrame runs one (include/dvo_amd.h,
    "many camera streams on the photometric engine").

    step(streams, bgr, depth) advances the listed streams by one frame each and returns a dict: T (n, 4, 4) the key-frame relative
    T, event (n,) 1 reference tick / 0 ordinary / -1 new reference refused, norms (n, n_run, iterations) the |eps| of every
    iteration (-1 where not run) and updates (n, n_run).  K = (fx, fy, cx, cy) of the level-0 camera matrix; photo_overrides set
    fields of dvo_photo_params (gradient_threshold, max_jacobian_size, min_required_pts, iterations, eps_norm_stop)."""

    def __init__(self, max_streams: int, K, fixed: bool = False, ref_every: int = 10000, first_level: int = 1,
                 levels: Sequence[int] = (3, 2), rows: int = 480, cols: int = 640, **photo_overrides):
        self.lib = load_library()
        self._h = None
        p = DvoPhotoStreamsParams()
        self.lib.dvo_photo_streams_params_default(C.byref(p))
        p.photo.fx, p.photo.fy, p.photo.cx, p.photo.cy = (float(k) for k in K)
        p.photo.fixed = int(bool(fixed))
        for k, v in photo_overrides.items():
            setattr(p.photo, k, v)
        p.ref_every, p.first_level, p.n_run = ref_every, first_level, len(levels)
        for r, l in enumerate(levels[:DVO_MAX_LEVELS]):
            p.levels[r] = int(l)
        p.rows, p.cols = rows, cols
        self.params, self.max_streams = p, max_streams
        self.levels, self.iterations = tuple(int(l) for l in levels), p.photo.iterations
        h = C.c_void_p()
        rc = self.lib.dvo_photo_streams_create(C.byref(p), max_streams, C.byref(h))
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_photo_streams_last_error(None).decode())
        self._h = h

    def _chk(self, rc: int):
        if rc != DVO_OK:
            raise DvoError(rc, self.lib.dvo_photo_streams_last_error(self._h).decode())

    def close(self):
        if self._h is not None:
            self.lib.dvo_photo_streams_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self, stream: int):
        self._chk(self.lib.dvo_photo_streams_reset_stream(self._h, stream))

    def set_stream_intrinsics(self, stream: int, fx, fy, cx, cy):
        """the stream's own level-0 camera matrix (only before its first frame, or after reset)"""
        self._chk(self.lib.dvo_photo_streams_set_stream_intrinsics(self._h, stream, float(fx), float(fy), float(cx), float(cy)))

    def step(self, streams: Sequence[int], bgr, depth, flags: int = 0, rgb: bool = False,
             image_format: int = DVO_CAM_BGR8, depth_format: int = DVO_DEPTH_F32) -> dict:
        """bgr / depth: (rows, cols, 3) uint8 and (rows, cols) depth in sensor units per listed stream (host arrays; uint16 depth goes
        up as 16 bits, any other dtype is taken as float32; (rows, cols) uint8 images are mono8, rgb=True marks RGB8), or, with flags
        DVO_UPLOAD_DEVICE / DVO_UPLOAD_MAPPED, their addresses (ints) in image_format / depth_format (default BGR8, float32)"""
        n = len(streams)
        S = (C.c_int * max(n, 1))(*[int(s) for s in streams])
        if flags & (DVO_UPLOAD_DEVICE | DVO_UPLOAD_MAPPED):
            B = (C.c_void_p * max(n, 1))(*[int(p) for p in bgr])
            D = (C.c_void_p * max(n, 1))(*[int(p) for p in depth])
            rows, cols = self.params.rows, self.params.cols
            keep = None
        else:
            image_format, bl, depth_format, dl = _camera_arrays(bgr, depth, rgb, 0)
            B = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bl])
            D = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in dl])
            rows, cols = bl[0].shape[:2] if n else (0, 0)
            keep = (bl, dl)
        nr, it = len(self.levels), self.iterations
        T = np.zeros((max(n, 1), 4, 4))
        norms = np.zeros((max(n, 1), nr, it))
        upd = np.zeros((max(n, 1), nr), np.int32)
        ev = np.zeros(max(n, 1), np.int32)
        if (image_format, depth_format) == (DVO_CAM_BGR8, DVO_DEPTH_F32):
            self._chk(self.lib.dvo_photo_streams_step(self._h, n, S, B, D, rows, cols, flags, _ptr(T), _ptr(norms),
                                                      upd.ctypes.data_as(C.POINTER(C.c_int)), ev.ctypes.data_as(C.POINTER(C.c_int))))
        else:
            self._chk(self.lib.dvo_photo_streams_step_fmt(self._h, n, S, B, image_format, D, depth_format, rows, cols, flags, _ptr(T),
                                                          _ptr(norms), upd.ctypes.data_as(C.POINTER(C.c_int)),
                                                          ev.ctypes.data_as(C.POINTER(C.c_int))))
        del keep
        return dict(T=T[:n], event=ev[:n], norms=norms[:n], updates=upd[:n])

    def jacobian(self, stream: int, level: int, capacity: Optional[int] = None) -> dict:
        """J, sel_i, sel_j, A, n of the stream's current reference at `level` (as DvoContext.photo_jacobian)"""
        if capacity is None:
            capacity = min(self.params.photo.max_jacobian_size,
                           int(round(self.params.rows * 0.5 ** level)) * int(round(self.params.cols * 0.5 ** level)) + 1)
        J = np.zeros((capacity, 6), np.float64); si = np.zeros(capacity, np.int32); sj = np.zeros(capacity, np.int32)
        A = np.zeros((6, 6), np.float64); nn = C.c_int(0)
        self._chk(self.lib.dvo_photo_streams_get_jacobian(self._h, stream, level, _ptr(J), _ptr(si), _ptr(sj), capacity, _ptr(A),
                                                          C.byref(nn)))
        m = min(nn.value, capacity)
        return dict(J=J[:m].copy(), sel_i=si[:m].copy(), sel_j=sj[:m].copy(), A=A, n=nn.value)

    def stats(self) -> dict:
        v = [C.c_int() for _ in range(5)]
        self._chk(self.lib.dvo_photo_streams_get_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("launches", "syncs", "runs", "ref_events", "refused"), (x.value for x in v)))

    def context_handle(self) -> int:
        """the underlying dvo_ctx* (frame-store slot = stream)"""
        return self.lib.dvo_photo_streams_context(self._h)
