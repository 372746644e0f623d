"""Python binding of liborbx (the MI355X ORB front-end C ABI, include/orbx.h).

Mirrors the reference's operator interface for the hot path:

* ``ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)`` with
  ``__call__(image) -> (keypoints, descriptors)``, the getters
  ``GetLevels/GetScaleFactor/GetScaleFactors/...`` and ``mvImagePyramid``
  (include/ORBextractor.h:45-111).
* ``ORBmatcher.DescriptorDistance`` (include/ORBmatcher.h:44) plus the batched
  device searches.

Keypoints are numpy structured arrays laid out like cv::KeyPoint (28 bytes).
Device-batch entry points take torch tensors (torch is used only for device
memory and streams).  There is no CPU fallback: if liborbx.so is missing this
module raises on import.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ORBX_LIB: an instrumented build of the same library for profiling experiments (tools/diag)
LIB_PATH = os.environ.get("ORBX_LIB") or os.path.join(_HERE, "liborbx.so")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

OK, EMPTY, EINVAL, ENOMEM, EDEVICE, ENOSPC = 0, 1, -22, -12, -5, -28
ORBM_MAX_FEATURES = 16384   # include/orbx.h: keypoints per frame of the matcher searches
ORBV_MAX_FEATURES = 65536   # include/orbx.h: descriptors per frame of the vocabulary transform
ORBV_DB_MAX_KEYFRAMES = 65536   # include/orbx.h: KeyFrameDatabase slots between clears
TOP2, FULL_U16 = 0, 1
RESIZE_SCALAR, RESIZE_SSE2 = 0, 1              # orbx_set_cv_modes (include/orbx.h)
BLUR_SCALAR, BLUR_SSE2, BLUR_BITEXACT = 0, 1, 2

EXPORTED = [
    "orbx_create", "orbx_destroy", "orbx_get_tables", "orbx_capacity", "orbx_set_cv_modes", "orbx_extract", "orbx_get_level",
    "orbx_extract_batch_device", "orbx_extract_stage_device", "orbx_sync", "orbx_set_timing", "orbx_get_stage_times",
    "orbx_debug_pyramid", "orbx_debug_candidates", "orbx_debug_fill_workspace", "orbx_debug_launches", "orbx_debug_qt_plan", "orbm_descriptor_distance", "orbm_allpairs_device", "orbm_allpairs",
    "orbm_search_init_batch_device", "orbm_search_for_initialization_device", "orbm_search_for_initialization",
    "orbm_debug_search_init_plan",
    "orbx_compute_stereo_matches", "orbx_stereo_batch_device",
    "orbm_bow_search_device", "orbm_bow_search",
    "orbm_search_by_projection_device", "orbm_search_by_projection",
    "orbm_project_search_device", "orbm_project_search", "orbx_ingest_batch_device", "orbx_depth_batch_device",
    "orbm_search_by_sim3_device", "orbm_search_by_sim3",
    "orbx_undistort_points", "orbx_image_bounds", "orbx_undistort_batch_device", "orbx_rgbd_stereo_batch_device",
    "orbx_rgbd_stereo", "orbm_frustum_batch_device", "orbm_frustum",
    "orbm_pose_optimization_device", "orbm_pose_optimization", "orbm_pose_optimization_host",
    "orbx_po_sincos_theta3",
    "orbm_sim3_workspace_bytes", "orbm_sim3_ransac_iterations", "orbm_sim3_setup_device", "orbm_sim3_iterate_device",
    "orbm_sim3_solve", "orbm_sim3_solve_host", "orbx_fixed_atan2", "orbx_sim3_triplet",
    "orbm_optimize_sim3_device", "orbm_sim3_gather_matches_device", "orbm_optimize_sim3", "orbm_optimize_sim3_host",
    "orbx_fixed_exp",
    "orbm_init_workspace_bytes", "orbm_initialize_device", "orbm_initialize", "orbm_initialize_host", "orbx_init_sets",
    "orbx_fixed_acosf",
    "orbm_pnp_workspace_bytes", "orbm_pnp_ransac_parameters", "orbm_pnp_setup_device", "orbm_pnp_iterate_device",
    "orbm_pnp_state_bytes", "orbm_pnp_solve", "orbm_pnp_solve_host", "orbx_pnp_quad", "orbx_pnp_qr_solve",
    "orbx_pnp_svd12",
    "orbm_refresh_map_points_device", "orbm_refresh_map_points", "orbm_triangulate_device", "orbm_triangulate",
    "orbm_local_map_work_bytes", "orbm_local_map_device", "orbm_local_map",
    "orbm_connections_work_bytes", "orbm_update_connections_device", "orbm_update_connections",
    "orbm_erase_connections_device", "orbm_best_covisibles_device", "orbm_connected_mask_device",
    "orbm_covisibles_by_weight_device", "orbm_children_work_bytes", "orbm_children_device",
    "orbm_map_point_culling_device", "orbm_map_point_culling", "orbm_culling_work_bytes",
    "orbm_keyframe_culling_device", "orbm_keyframe_culling", "orbm_compact_observations_device",
    "orbm_compact_observations",
    "orbm_best2_csr_device", "orbm_best2_csr", "orbm_stereo_band", "orbm_stereo_band_device",
    "orbv_load_text", "orbv_create", "orbv_destroy", "orbv_info", "orbv_transform", "orbv_transform_batch_device",
    "orbv_score", "orbv_db_create", "orbv_db_destroy", "orbv_db_add", "orbv_db_add_batch_device", "orbv_db_erase",
    "orbv_db_clear", "orbv_db_info", "orbv_db_scores", "orbv_db_detect_loop", "orbv_db_detect_reloc",
    "orbv_db_detect_loop_device", "orbv_db_detect_reloc_device",
]
BOW_KF_F, BOW_KF_KF, TRIANGULATION = 0, 1, 2


class OrbxError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__("%s failed with status %d" % (fn, code))
        self.code = code


class BowView(C.Structure):
    """orbm_bow_view: one side of a vocabulary-node search (host or device pointers)."""
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("has_mp", C.c_void_p), ("u_right", C.c_void_p),
                ("fv_node", C.c_void_p), ("fv_ptr", C.c_void_p), ("fv_idx", C.c_void_p), ("n", C.c_int32),
                ("fv_nnodes", C.c_int32)]


class TriangParams(C.Structure):
    """orbm_triang_params (SearchForTriangulation geometry)."""
    _fields_ = [("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float), ("scale2", C.c_float * 16),
                ("sigma2_2", C.c_float * 16), ("only_stereo", C.c_int32)]


PROJ_POINT_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"),
                             ("level", "<i4"), ("flags", "<i4")])


class ProjParams(C.Structure):
    """orbm_proj_params (Frame grid bounds, th, nnratio, mvScaleFactors)."""
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
                ("th", C.c_float), ("nnratio", C.c_float), ("scale", C.c_float * 16)]


def proj_params(grid, scale, th=1.0, nnratio=0.8):
    pp = ProjParams()
    pp.min_x, pp.min_y, pp.grid_w_inv, pp.grid_h_inv = (float(g) for g in grid)
    pp.th, pp.nnratio = th, nnratio
    sc = np.zeros(16, np.float32)
    sc[:len(scale)] = scale
    pp.scale[:] = [float(x) for x in sc]
    return pp


PROJ_LAST_FRAME, PROJ_KEYFRAME, PROJ_SIM3, FUSE, FUSE_SIM3 = 0, 1, 2, 3, 4


class Grid(C.Structure):
    """orbm_grid: Frame's image bounds and grid cell inverses (src/Frame.cc:32-33, 127-128)."""
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float)]


def frame_grid(bounds):
    """bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY) -> Grid, with the inverses computed in float like
    Frame's constructor: 64.f / (mnMaxX - mnMinX), 48.f / (mnMaxY - mnMinY)."""
    b = [np.float32(v) for v in bounds]
    g = Grid()
    g.min_x, g.min_y = float(b[0]), float(b[2])
    g.grid_w_inv = float(np.float32(64) / np.float32(b[1] - b[0]))
    g.grid_h_inv = float(np.float32(48) / np.float32(b[3] - b[2]))
    return g


def debug_search_init_plan(cap, npairs):
    """What the SearchForInitialization launcher does for per-frame capacity `cap` and `npairs` pairs
    (orbm_debug_search_init_plan; host arithmetic, no launch): qsplit = k_si_build's query slices per pair,
    lds_tiers = the level-0 capacities of the LDS-form k_si_greedy launches in ascending order, global_cap = the
    device-memory form's capacity (0 = not launched), lds_max = the largest level-0 count the LDS form holds,
    rank_max = k_si_grid's rank sort / counting sort threshold, build_lds = k_si_build's LDS staging threshold, build_queries = the queries one k_si_build
    workgroup takes per sweep."""
    out = (C.c_int * 10)()
    _check("orbm_debug_search_init_plan", lib.orbm_debug_search_init_plan(cap, npairs, out))
    v = list(out)
    return {"qsplit": v[0], "lds_tiers": v[2:2 + v[1]], "global_cap": v[5], "lds_max": v[6], "rank_max": v[7],
            "build_lds": v[8], "build_queries": v[9]}


MAP_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                            ("max_dist", "<f4"), ("min_dist", "<f4"), ("angle", "<f4"), ("octave", "<i4"),
                            ("flags", "<i4"), ("pad", "<i4")])


OBSERVATION_DTYPE = np.dtype([("kf", "<i4"), ("idx", "<i4")])   # orbm_observation: KeyFrame slot, mObservations[pKF]
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
ORBM_MAX_OBSERVATIONS = 1024   # include/orbx.h: observations of one MapPoint in a refresh


class PoseParams(C.Structure):
    """orbm_pose_params (camera, image bounds, grid, scale pyramid, the search arguments)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("b", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
                ("log_scale", C.c_float), ("nlevels", C.c_int32), ("th", C.c_float), ("mono", C.c_int32),
                ("orb_dist", C.c_int32), ("check_ori", C.c_int32), ("scale", C.c_float * 16),
                ("inv_sigma2", C.c_float * 16)]


class InitOut(C.Structure):
    """orbm_init_out: the per-pair output arrays of the Initializer (host or device pointers)."""
    _fields_ = [(n, C.c_void_p) for n in ("status", "model", "reason", "scores", "H21", "F21", "inliersH", "inliersF",
                                          "R21", "t21", "p3d", "triangulated", "ngood", "parallax", "nmatches_left",
                                          "matches_out")]


def pose_params(K, bounds, scale, inv_sigma2=None, log_scale=None, bf=0.0, th=1.0, mono=False, orb_dist=100,
                check_ori=True):
    """K = (fx, fy, cx, cy); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY); scale = mvScaleFactors.
    The grid cell sizes follow Frame's constructor (64 x 48 cells over the bounds);
    log_scale defaults to (float)log(scale[1]) like Frame::mfLogScaleFactor."""
    pp = PoseParams()
    pp.fx, pp.fy, pp.cx, pp.cy = (float(v) for v in K)
    pp.bf = float(bf)
    pp.b = float(np.float32(bf) / np.float32(K[0])) if K[0] else 0.0
    pp.min_x, pp.max_x, pp.min_y, pp.max_y = (float(v) for v in bounds)
    pp.grid_w_inv = float(np.float32(64) / np.float32(np.float32(bounds[1]) - np.float32(bounds[0])))
    pp.grid_h_inv = float(np.float32(48) / np.float32(np.float32(bounds[3]) - np.float32(bounds[2])))
    sc = np.zeros(16, np.float32)
    sc[:len(scale)] = scale
    pp.scale[:] = [float(x) for x in sc]
    pp.nlevels = len(scale)
    if inv_sigma2 is None:
        inv_sigma2 = np.float32(1) / (np.asarray(scale, np.float32) * np.asarray(scale, np.float32))
    s2 = np.zeros(16, np.float32)
    s2[:len(inv_sigma2)] = inv_sigma2
    pp.inv_sigma2[:] = [float(x) for x in s2]
    pp.log_scale = float(np.float32(np.log(np.float64(np.float32(scale[1]))))) if log_scale is None else log_scale
    pp.th, pp.mono, pp.orb_dist, pp.check_ori = float(th), int(bool(mono)), int(orb_dist), int(bool(check_ori))
    return pp


class Camera(C.Structure):
    """orbx_camera: mK and mDistCoef (CV_32F), Camera.fx .. Camera.k3 of the settings file."""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


def camera(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    return Camera(fx, fy, cx, cy, k1, k2, p1, p2, k3)


class CovisGraph(C.Structure):
    """orbm_covis_graph: the covisibility graph's tables (host or device pointers)."""
    _fields_ = [("conn_kf", C.c_void_p), ("conn_w", C.c_void_p), ("nconn", C.c_void_p), ("ord_kf", C.c_void_p),
                ("ord_w", C.c_void_p), ("nord", C.c_void_p), ("parent", C.c_void_p), ("first", C.c_void_p)]


class _Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("liborbx.so not built (run `make -C orb-slam-_amd` or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P, vp = C.POINTER, C.c_void_p
    u8p, i32p, f32p = P(C.c_uint8), P(C.c_int), P(C.c_float)
    L.orbx_create.argtypes = [P(_Params), C.c_int, P(vp)]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_destroy.restype = None
    L.orbx_get_tables.argtypes = [vp, i32p, f32p, f32p, f32p, f32p, f32p, i32p]
    L.orbx_capacity.argtypes = [vp, C.c_int, C.c_int]
    L.orbx_set_cv_modes.argtypes = [vp, C.c_int, C.c_int]
    L.orbx_extract.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, u8p, i32p]
    L.orbx_get_level.argtypes = [vp, C.c_int, P(u8p), i32p, i32p, P(C.c_size_t)]
    L.orbx_extract_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp, vp,
                                            vp, C.c_int, vp]
    L.orbx_extract_stage_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp,
                                            vp, vp, C.c_int, vp]
    L.orbx_sync.argtypes = [vp, vp]
    L.orbx_set_timing.argtypes = [vp, C.c_int]
    L.orbx_get_stage_times.argtypes = [vp, f32p, C.c_int]
    L.orbx_debug_pyramid.argtypes = [vp, C.c_int, u8p, C.c_size_t]
    L.orbx_debug_candidates.argtypes = [vp, C.c_int, C.c_int, i32p, C.c_int, i32p]
    L.orbx_debug_fill_workspace.argtypes = [vp, C.c_int]
    L.orbx_debug_launches.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, C.c_int]
    L.orbx_debug_qt_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, C.c_int]
    L.orbm_descriptor_distance.argtypes = [u8p, u8p]
    L.orbm_allpairs_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_allpairs.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_int, vp, vp, vp, vp]
    L.orbm_search_init_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_float, C.c_int, vp, vp, vp]
    L.orbm_search_for_initialization_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp,
                                                        C.c_int, C.c_float, C.c_int, vp, vp, vp, vp]
    L.orbm_search_for_initialization.argtypes = [C.c_int, vp, u8p, C.c_int, vp, u8p, C.c_int, vp, f32p, C.c_int,
                                                 C.c_float, C.c_int, i32p, i32p]
    L.orbm_debug_search_init_plan.argtypes = [C.c_int, C.c_int, i32p]
    L.orbx_compute_stereo_matches.argtypes = [vp, vp, vp, u8p, C.c_int, vp, u8p, C.c_int, C.c_float, C.c_float,
                                              f32p, f32p, i32p]
    L.orbx_stereo_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_float, vp, vp,
                                           vp, vp]
    f64p = P(C.c_double)
    L.orbv_load_text.argtypes = [C.c_char_p, C.c_int, P(vp)]
    L.orbv_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, u8p, u8p, f64p, C.c_int, P(vp)]
    L.orbv_destroy.argtypes = [vp]
    L.orbv_destroy.restype = None
    L.orbv_info.argtypes = [vp, i32p, i32p, i32p, i32p, i32p, i32p]
    L.orbv_transform.argtypes = [vp, u8p, C.c_int, C.c_int, i32p, f64p, i32p, i32p, i32p, i32p, i32p]
    L.orbv_transform_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbv_score.argtypes = [C.c_int, i32p, f64p, C.c_int, i32p, f64p, C.c_int, f64p]
    L.orbv_db_create.argtypes = [vp, C.c_int, C.c_int, P(vp)]
    L.orbv_db_destroy.argtypes = [vp]
    L.orbv_db_destroy.restype = None
    L.orbv_db_add.argtypes = [vp, i32p, f64p, C.c_int, i32p]
    L.orbv_db_add_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, i32p, vp]
    L.orbv_db_erase.argtypes = [vp, C.c_int]
    L.orbv_db_clear.argtypes = [vp]
    L.orbv_db_info.argtypes = [vp, i32p, i32p, P(C.c_size_t)]
    L.orbv_db_scores.argtypes = [vp, i32p, f64p, C.c_int, i32p, C.c_int, f64p]
    L.orbv_db_detect_loop.argtypes = [vp, i32p, f64p, C.c_int, u8p, i32p, C.c_float, i32p, C.c_int, i32p, i32p,
                                      f32p]
    L.orbv_db_detect_reloc.argtypes = [vp, i32p, f64p, C.c_int, i32p, i32p, C.c_int, i32p, i32p, f32p]
    L.orbv_db_detect_loop_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_float, C.c_int, vp, vp, vp, vp,
                                             vp]
    L.orbv_db_detect_reloc_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_search_by_projection_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int,
                                                   P(ProjParams), vp, vp, vp]
    L.orbm_search_by_projection.argtypes = [C.c_int, vp, u8p, f32p, u8p, C.c_int, vp, u8p, C.c_int, P(ProjParams),
                                            i32p, i32p]
    L.orbm_project_search_device.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int,
                                             P(PoseParams), vp, vp, vp]
    L.orbm_project_search.argtypes = [C.c_int, C.c_int, vp, u8p, f32p, u8p, C.c_int, f32p, vp, u8p, C.c_int,
                                      P(PoseParams), i32p, i32p]
    L.orbm_search_by_sim3_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int,
                                             P(PoseParams), vp, vp, vp, vp, vp]
    L.orbm_search_by_sim3.argtypes = [C.c_int, vp, u8p, vp, u8p, u8p, C.c_int, f32p, vp, u8p, vp, u8p, u8p, C.c_int,
                                      f32p, C.c_float, f32p, f32p, P(PoseParams), i32p, i32p, i32p, i32p]
    L.orbx_ingest_batch_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                           vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, vp]
    L.orbx_depth_batch_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_float,
                                          vp, C.c_size_t, C.c_size_t, vp]
    L.orbx_undistort_points.argtypes = [P(Camera), f32p, C.c_int, f32p]
    L.orbx_image_bounds.argtypes = [P(Camera), C.c_int, C.c_int, f32p]
    L.orbx_undistort_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, P(Camera), vp, vp]
    L.orbx_rgbd_stereo_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t,
                                                C.c_size_t, C.c_float, vp, vp, vp]
    L.orbx_rgbd_stereo.argtypes = [C.c_int, vp, vp, C.c_int, f32p, C.c_int, C.c_int, C.c_size_t, C.c_float, f32p,
                                   f32p]
    L.orbm_frustum_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, P(PoseParams), C.c_float, vp, vp, vp]
    L.orbm_frustum.argtypes = [C.c_int, vp, C.c_int, f32p, P(PoseParams), C.c_float, vp, i32p]
    L.orbm_pose_optimization_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int,
                                                P(PoseParams), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    for fn in (L.orbm_pose_optimization, L.orbm_pose_optimization_host):
        fn.argtypes = ([C.c_int] if fn is L.orbm_pose_optimization else []) + [
            vp, vp, C.c_int, vp, vp, C.c_int, vp, P(PoseParams), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_po_sincos_theta3.argtypes = [C.c_double, C.POINTER(C.c_double)]
    L.orbx_po_sincos_theta3.restype = None
    L.orbm_sim3_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.orbm_sim3_workspace_bytes.restype = C.c_size_t
    L.orbm_sim3_ransac_iterations.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int]
    L.orbm_sim3_setup_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp,
                                         C.c_int, P(PoseParams), vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.orbm_sim3_iterate_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, P(PoseParams), C.c_int, C.c_int, C.c_int,
                                           vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for fn in (L.orbm_sim3_solve, L.orbm_sim3_solve_host):
        fn.argtypes = ([C.c_int] if fn is L.orbm_sim3_solve else []) + [
            vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, P(PoseParams), C.c_int, C.c_double,
            C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_fixed_atan2.argtypes = [C.c_double, C.c_double]
    L.orbx_fixed_atan2.restype = C.c_double
    L.orbx_sim3_triplet.argtypes = [C.c_int, i32p, i32p]
    L.orbx_sim3_triplet.restype = None
    L.orbm_optimize_sim3_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int,
                                            vp, vp, C.c_int, C.c_float, C.c_int, P(PoseParams), vp, vp, vp, vp, vp, vp,
                                            vp]
    L.orbm_sim3_gather_matches_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp,
                                                  C.c_int, vp]
    for fn in (L.orbm_optimize_sim3, L.orbm_optimize_sim3_host):
        fn.argtypes = ([C.c_int] if fn is L.orbm_optimize_sim3 else []) + [
            vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_float, C.c_int, P(PoseParams),
            vp, vp, vp, vp, vp, vp]
    L.orbx_fixed_exp.argtypes = [C.c_double]
    L.orbx_fixed_exp.restype = C.c_double
    L.orbm_init_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.orbm_init_workspace_bytes.restype = C.c_size_t
    L.orbm_initialize_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int,
                                         P(PoseParams), C.c_float, C.c_int, C.c_int, vp, C.c_size_t, P(InitOut), vp]
    for fn in (L.orbm_initialize, L.orbm_initialize_host):
        fn.argtypes = ([C.c_int] if fn is L.orbm_initialize else []) + [
            vp, C.c_int, vp, C.c_int, vp, vp, P(PoseParams), C.c_float, C.c_int, C.c_int, P(InitOut)]
    L.orbx_init_sets.argtypes = [C.c_int, vp, C.c_int, vp]
    L.orbx_init_sets.restype = None
    L.orbx_fixed_acosf.argtypes = [C.c_float]
    L.orbx_fixed_acosf.restype = C.c_float
    L.orbm_pnp_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.orbm_pnp_workspace_bytes.restype = C.c_size_t
    L.orbm_pnp_state_bytes.argtypes = [C.c_int]
    L.orbm_pnp_state_bytes.restype = C.c_size_t
    L.orbm_pnp_ransac_parameters.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, i32p, i32p]
    L.orbm_pnp_ransac_parameters.restype = None
    L.orbm_pnp_setup_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp,
                                        C.c_int, P(PoseParams), C.c_float, vp, vp, C.c_int, vp, C.c_size_t, vp, vp,
                                        vp, vp, vp]
    L.orbm_pnp_iterate_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, P(PoseParams), C.c_int, C.c_int, C.c_int,
                                          vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for fn in (L.orbm_pnp_solve, L.orbm_pnp_solve_host):
        fn.argtypes = ([C.c_int] if fn is L.orbm_pnp_solve else []) + [
            vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, P(PoseParams), C.c_float, C.c_double, C.c_int, C.c_int,
            C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp] + (
            [vp, C.c_int, vp] if fn is L.orbm_pnp_solve_host else [])
    L.orbx_pnp_quad.argtypes = [C.c_int, i32p, i32p]
    L.orbx_pnp_quad.restype = None
    L.orbx_pnp_qr_solve.argtypes = [vp, vp, vp]
    L.orbx_pnp_svd12.argtypes = [vp, vp, vp]
    L.orbx_pnp_svd12.restype = None
    L.orbm_refresh_map_points_device.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int,
                                                 C.c_int, P(PoseParams), vp, vp, vp, vp]
    L.orbm_refresh_map_points.argtypes = [C.c_int, C.c_int, vp, u8p, i32p, C.c_int, C.c_int, f32p, u8p, i32p, vp, vp,
                                          C.c_int, P(PoseParams), vp, u8p, i32p]
    L.orbm_triangulate_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int,
                                          P(PoseParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_triangulate.argtypes = [C.c_int, vp, vp, f32p, f32p, C.c_int, f32p, vp, vp, f32p, f32p, C.c_int, f32p, i32p,
                                   P(PoseParams), f32p, i32p, vp, vp, vp, i32p, i32p, u8p, u8p]
    L.orbm_local_map_work_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.orbm_local_map_work_bytes.restype = C.c_size_t
    L.orbm_local_map_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp,
                                        vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp,
                                        vp, vp, C.c_size_t, vp]
    L.orbm_local_map.argtypes = [C.c_int, i32p, i32p, u8p, i32p, i32p, i32p, i32p, i32p, C.c_int, C.c_int, vp, u8p,
                                 i32p, vp, C.c_int, C.c_int, i32p, i32p, i32p, i32p, C.c_int, i32p, i32p, i32p, vp,
                                 u8p, C.c_int, u8p, i32p]
    L.orbm_connections_work_bytes.argtypes = [C.c_int, C.c_int]
    L.orbm_connections_work_bytes.restype = C.c_size_t
    L.orbm_update_connections_device.argtypes = [P(CovisGraph), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp,
                                                 C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]
    L.orbm_update_connections.argtypes = [C.c_int, P(CovisGraph), C.c_int, C.c_int, i32p, i32p, C.c_int, i32p, vp,
                                          i32p, vp, C.c_int, i32p, C.c_int, C.c_int, C.c_int, i32p]
    L.orbm_erase_connections_device.argtypes = [P(CovisGraph), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_size_t,
                                                vp]
    L.orbm_best_covisibles_device.argtypes = [P(CovisGraph), C.c_int, C.c_int, C.c_int, vp, vp]
    L.orbm_connected_mask_device.argtypes = [P(CovisGraph), C.c_int, C.c_int, C.c_int, vp, vp]
    L.orbm_covisibles_by_weight_device.argtypes = [P(CovisGraph), C.c_int, C.c_int, C.c_int, vp, vp]
    L.orbm_children_work_bytes.argtypes = [C.c_int]
    L.orbm_children_work_bytes.restype = C.c_size_t
    L.orbm_children_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_size_t, vp]
    L.orbm_map_point_culling_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp,
                                                C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_map_point_culling.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp,
                                         vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_culling_work_bytes.argtypes = [C.c_int]
    L.orbm_culling_work_bytes.restype = C.c_size_t
    L.orbm_keyframe_culling_device.argtypes = [P(CovisGraph), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp,
                                               vp, vp, C.c_float, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                               C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.orbm_keyframe_culling.argtypes = [C.c_int, P(CovisGraph), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int,
                                        vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int,
                                        vp, vp, vp, vp, vp, vp]
    L.orbm_compact_observations_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbm_compact_observations.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    L.orbm_best2_csr_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbm_best2_csr.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, i32p, i32p, C.c_int, i32p, i32p, i32p]
    L.orbm_stereo_band.argtypes = [C.c_int, vp, u8p, C.c_int, vp, u8p, C.c_int, C.c_int, f32p, C.c_int, C.c_float,
                                   C.c_float, i32p, i32p]
    L.orbm_stereo_band_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, f32p, C.c_int, C.c_float,
                                          C.c_float, vp, vp, vp]
    L.orbm_bow_search_device.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp, C.c_int,
                                         vp, vp]
    L.orbm_bow_search.argtypes = [C.c_int, C.c_int, P(BowView), P(BowView), P(TriangParams), C.c_float, C.c_int,
                                  i32p, i32p]
    return L


lib = _load()


def _check(fn, rc):
    if rc not in (OK, EMPTY):
        raise OrbxError(fn, rc)
    return rc


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


class ORBextractor:
    """ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-111) on an MI355X."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device=0):
        self.params = _Params(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        h = C.c_void_p()
        _check("orbx_create", lib.orbx_create(C.byref(self.params), device, C.byref(h)))
        self._h = h
        n = nlevels
        self._scale = np.zeros(n, np.float32)
        self._inv = np.zeros(n, np.float32)
        self._s2 = np.zeros(n, np.float32)
        self._is2 = np.zeros(n, np.float32)
        self._nfl = np.zeros(n, np.int32)
        f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        _check("orbx_get_tables", lib.orbx_get_tables(h, None, None, f32(self._scale), f32(self._inv), f32(self._s2),
                                                      f32(self._is2), self._nfl.ctypes.data_as(C.POINTER(C.c_int))))
        self._last_shape = None
        self._modes = (RESIZE_SCALAR, BLUR_SCALAR)

    def close(self):
        if getattr(self, "_h", None):
            lib.orbx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # getters, include/ORBextractor.h:63-83
    def GetLevels(self):
        return self.params.nlevels

    def GetScaleFactor(self):
        return float(np.float32(self.params.scale_factor))

    def GetScaleFactors(self):
        return self._scale.copy()

    def GetInverseScaleFactors(self):
        return self._inv.copy()

    def GetScaleSigmaSquares(self):
        return self._s2.copy()

    def GetInverseScaleSigmaSquares(self):
        return self._is2.copy()

    def features_per_level(self):
        return self._nfl.copy()

    def set_cv_modes(self, resize=None, blur=None):
        """The OpenCV build the extractor reproduces (include/orbx.h orbx_set_cv_modes):
        resize RESIZE_SCALAR / RESIZE_SSE2, blur BLUR_SCALAR / BLUR_SSE2 / BLUR_BITEXACT (None: keep)."""
        self._modes = (self._modes[0] if resize is None else int(resize), self._modes[1] if blur is None else int(blur))
        _check("orbx_set_cv_modes", lib.orbx_set_cv_modes(self._h, self._modes[0], self._modes[1]))

    def capacity(self, rows, cols):
        c = lib.orbx_capacity(self._h, rows, cols)
        if c < 0:
            raise OrbxError("orbx_capacity", c)
        return c

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors); mask ignored like the reference."""
        img = np.asarray(image)
        # a cv::Mat ROI keeps its parent's step: rows with unit-stride pixels pass through as they are
        if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), None
        rows, cols = img.shape
        cap = self.capacity(rows, cols)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        _check("orbx_extract", lib.orbx_extract(self._h, _u8(img), rows, cols, img.strides[0], kps.ctypes.data, cap,
                                                _u8(desc), C.byref(n)))
        self._last_shape = (rows, cols)
        k = n.value
        return kps[:k].copy(), (desc[:k].copy() if k else None)

    @property
    def mvImagePyramid(self):
        out = []
        for l in range(self.params.nlevels):
            p = C.POINTER(C.c_uint8)()
            r, c, s = C.c_int(), C.c_int(), C.c_size_t()
            _check("orbx_get_level", lib.orbx_get_level(self._h, l, C.byref(p), C.byref(r), C.byref(c), C.byref(s)))
            buf = np.ctypeslib.as_array(p, shape=(r.value * s.value,))
            out.append(buf.reshape(r.value, s.value)[:, :c.value].copy())
        return out

    # ---- device batch (config 2/4 replay) ----
    def extract_batch_device(self, imgs, kps, desc, counts, stream=None):
        """imgs: uint8 cuda tensor (B, H, W) (row pitch = stride(1)); kps: int32 (B, cap, 7);
        desc: uint8 (B, cap, 32); counts: int32 (B,).  Asynchronous on `stream`."""
        B, H, W = imgs.shape
        cap = kps.shape[1]
        rc = lib.orbx_extract_batch_device(self._h, _ptr(imgs), B, H, W, imgs.stride(1), imgs.stride(0), _ptr(kps),
                                           _ptr(desc), _ptr(counts), cap, _stream(stream))
        _check("orbx_extract_batch_device", rc)

    def extract_stage_device(self, stage, imgs, kps, desc, counts, stream=None):
        """One stage (0 pyramid, 1 FAST, 2 quadtree, 3 describe) of extract_batch_device, on `stream`; the caller
        orders a batch's stages across streams (orbx_extract_stage_device)."""
        B, H, W = imgs.shape
        cap = kps.shape[1]
        rc = lib.orbx_extract_stage_device(self._h, int(stage), _ptr(imgs), B, H, W, imgs.stride(1), imgs.stride(0),
                                           _ptr(kps), _ptr(desc), _ptr(counts), cap, _stream(stream))
        _check("orbx_extract_stage_device", rc)

    def stereo_batch_device(self, kps, desc, counts, left, right, bf, fx, u_right=None, depth=None, n_good=None,
                            stream=None):
        """Frame::ComputeStereoMatches on pairs (left[p], right[p]) of the last device batch.
        Returns (u_right (P, cap) f32, depth (P, cap) f32, n_good (P,) i32) cuda tensors."""
        import torch
        npairs, cap = left.shape[0], kps.shape[1]
        if u_right is None:
            u_right = torch.empty((npairs, cap), dtype=torch.float32, device=kps.device)
        if depth is None:
            depth = torch.empty((npairs, cap), dtype=torch.float32, device=kps.device)
        if n_good is None:
            n_good = torch.empty((npairs,), dtype=torch.int32, device=kps.device)
        rc = lib.orbx_stereo_batch_device(self._h, _ptr(kps), _ptr(desc), _ptr(counts), cap, _ptr(left), _ptr(right),
                                          npairs, bf, fx, _ptr(u_right), _ptr(depth), _ptr(n_good), _stream(stream))
        _check("orbx_stereo_batch_device", rc)
        return u_right, depth, n_good

    def sync(self, stream=None):
        _check("orbx_sync", lib.orbx_sync(self._h, _stream(stream)))

    def set_timing(self, enable=True):
        _check("orbx_set_timing", lib.orbx_set_timing(self._h, 1 if enable else 0))

    def stage_times(self):
        ms = np.zeros(4, np.float32)
        _check("orbx_get_stage_times", lib.orbx_get_stage_times(self._h, ms.ctypes.data_as(C.POINTER(C.c_float)), 4))
        return ms

    def debug_pyramid(self, frame, sizes):
        total = sum(w * h for w, h in sizes)
        buf = np.zeros(total, np.uint8)
        _check("orbx_debug_pyramid", lib.orbx_debug_pyramid(self._h, frame, _u8(buf), total))
        out, o = [], 0
        for w, h in sizes:
            out.append(buf[o:o + w * h].reshape(h, w))
            o += w * h
        return out

    def debug_candidates(self, frame, level, cap=1 << 20):
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int(0)
        _check("orbx_debug_candidates", lib.orbx_debug_candidates(self._h, frame, level,
                                                                  out.ctypes.data_as(C.POINTER(C.c_int)), cap,
                                                                  C.byref(n)))
        return out[:n.value].copy()

    def debug_fill_workspace(self, value):
        """Byte-fill the pyramid workspace and the host path's staged image over their whole capacity, after the
        handle's last work, and synchronise: the next extraction of a shape the workspace already holds then
        finds `value` in every byte it does not write itself (row padding, the room past the last level)."""
        _check("orbx_debug_fill_workspace", lib.orbx_debug_fill_workspace(self._h, int(value) & 0xFF))

    def debug_launches(self, rows, cols, batch):
        """Kernel launches per stage of one batched extract: {pyramid, fast, quadtree, describe}, and
        pyramid_sources, the bit mask of the levels the pyramid launches resize from."""
        c = np.zeros(5, np.int32)
        _check("orbx_debug_launches", lib.orbx_debug_launches(self._h, rows, cols, batch,
                                                              c.ctypes.data_as(C.POINTER(C.c_int)), 5))
        return dict(zip(("pyramid", "fast", "quadtree", "describe", "pyramid_sources"), (int(v) for v in c)))

    def debug_qt_plan(self, rows, cols, batch):
        """The quadtree form of each level of one batched extract (orbx_debug_qt_plan), a dict per level: nt
        (workgroup size), kpt (keypoints per thread), glob (node arrays in global memory), wide, lcap, cellcap,
        gather_room (bytes: the owner map runs while 4 * cells + 2 * candidates fit) and launch (its index)."""
        nl = self.params.nlevels
        c = np.zeros((nl, 8), np.int32)
        _check("orbx_debug_qt_plan", lib.orbx_debug_qt_plan(self._h, rows, cols, batch,
                                                            c.ctypes.data_as(C.POINTER(C.c_int)), nl))
        names = ("nt", "kpt", "glob", "wide", "lcap", "cellcap", "gather_room", "launch")
        return [dict(zip(names, (int(v) for v in row))) for row in c]


def compute_stereo_matches(left, right, kps_l, desc_l, kps_r, desc_r, bf, fx):
    """Frame::ComputeStereoMatches (src/Frame.cc:630-872) for the host path: `left` / `right`
    are the two ORBextractor objects right after extracting the left / right image.
    Returns (mvuRight, mvDepth, n_good)."""
    kl = np.ascontiguousarray(kps_l, KEYPOINT_DTYPE)
    kr = np.ascontiguousarray(kps_r, KEYPOINT_DTYPE)
    nl, nr = len(kl), len(kr)
    dl = np.ascontiguousarray(desc_l if desc_l is not None else np.zeros((0, 32), np.uint8), np.uint8)
    dr = np.ascontiguousarray(desc_r if desc_r is not None else np.zeros((0, 32), np.uint8), np.uint8)
    ur = np.full(max(nl, 1), -1.0, np.float32)
    dp = np.full(max(nl, 1), -1.0, np.float32)
    ng = C.c_int(0)
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    _check("orbx_compute_stereo_matches",
           lib.orbx_compute_stereo_matches(left._h, right._h, kl.ctypes.data, _u8(dl), nl, kr.ctypes.data, _u8(dr), nr,
                                           bf, fx, f32(ur), f32(dp), C.byref(ng)))
    return ur[:nl].copy(), dp[:nl].copy(), ng.value


def ingest_batch_device(src, rgb=False, map_x=None, map_y=None, out=None, stream=None):
    """Tracking::GrabImage* colour conversion after the examples' cv::remap rectification, on a device
    batch.  src: uint8 tensor (B, H, W) or (B, H, W, C); map_x / map_y: float32 (nmaps, H', W') or None.
    Returns the gray (B, H', W') uint8 tensor (the layout orbx_extract_batch_device reads)."""
    import torch
    B, rows, cols = src.shape[:3]
    ch = 1 if src.dim() == 3 else src.shape[3]
    if map_x is not None:
        nmaps, drows, dcols = map_x.shape
    else:
        nmaps, drows, dcols = 1, rows, cols
    if out is None:
        out = torch.empty((B, drows, dcols), dtype=torch.uint8, device=src.device)
    _check("orbx_ingest_batch_device",
           lib.orbx_ingest_batch_device(_ptr(src), B, rows, cols, ch, int(bool(rgb)), src.stride(1), src.stride(0),
                                        _ptr(map_x) if map_x is not None else None,
                                        _ptr(map_y) if map_y is not None else None, nmaps, drows, dcols, _ptr(out),
                                        out.stride(1), out.stride(0), _stream(stream)))
    return out


def depth_batch_device(src, factor, out=None, stream=None):
    """GrabImageRGBD's imDepth.convertTo(CV_32F, mDepthMapFactor), applied under the reference's own
    condition (factor != 1 or a non-float depth map); src: (B, H, W) uint16-as-int16 or float32 tensor."""
    import torch
    B, rows, cols = src.shape
    isf = src.dtype == torch.float32
    if isf and abs(factor - 1.0) <= 1e-5:
        return src
    if out is None:
        out = torch.empty((B, rows, cols), dtype=torch.float32, device=src.device)
    esz = src.element_size()
    _check("orbx_depth_batch_device",
           lib.orbx_depth_batch_device(_ptr(src), 1 if isf else 0, B, rows, cols, src.stride(1) * esz,
                                       src.stride(0) * esz, factor, _ptr(out), out.stride(1) * 4, out.stride(0) * 4,
                                       _stream(stream)))
    return out


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def undistort_points(cam, xy):
    """cv::undistortPoints(xy, K, D, noArray(), K) (orbx_undistort_points, host code): xy (n, 2) float32."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.empty_like(xy)
    _check("orbx_undistort_points", lib.orbx_undistort_points(C.byref(cam), _f32p(xy), len(xy), _f32p(out)))
    return out


def image_bounds(cam, rows, cols):
    """Frame::ComputeImageBounds: (mnMinX, mnMaxX, mnMinY, mnMaxY) as float32 (host code)."""
    b = np.zeros(4, np.float32)
    _check("orbx_image_bounds", lib.orbx_image_bounds(C.byref(cam), rows, cols, _f32p(b)))
    return b


def undistort_batch_device(kps, counts, cam, out=None, stream=None):
    """Frame::UndistortKeyPoints over an extract batch: kps (B, cap, 7) int32, counts (B,).  out: the
    tensor to receive mvKeysUn (may be kps itself; default a new one, whose rows past the count are
    uninitialised).  Returns out."""
    import torch
    if out is None:
        out = torch.empty_like(kps)
    _check("orbx_undistort_batch_device",
           lib.orbx_undistort_batch_device(_ptr(kps), _ptr(counts), kps.shape[0], kps.shape[1], C.byref(cam),
                                           _ptr(out), _stream(stream)))
    return out


def rgbd_stereo_batch_device(kps, kps_un, counts, depth, bf, uright=None, depth_out=None, stream=None):
    """Frame::ComputeStereoFromRGBD over an extract batch: kps / kps_un (B, cap, 7) int32 (mvKeys /
    mvKeysUn), counts (B,), depth (B, H, W) float32 (depth_batch_device's output; any row / frame
    stride).  Returns (mvuRight, mvDepth), float32 (B, cap), written below each frame's count."""
    import torch
    B, cap = kps.shape[0], kps.shape[1]
    if uright is None:
        uright = torch.empty((B, cap), dtype=torch.float32, device=kps.device)
    if depth_out is None:
        depth_out = torch.empty((B, cap), dtype=torch.float32, device=kps.device)
    _check("orbx_rgbd_stereo_batch_device",
           lib.orbx_rgbd_stereo_batch_device(_ptr(kps), _ptr(kps_un), _ptr(counts), B, cap, _ptr(depth),
                                             depth.shape[1], depth.shape[2], depth.stride(1) * 4,
                                             depth.stride(0) * 4, bf, _ptr(uright), _ptr(depth_out),
                                             _stream(stream)))
    return uright, depth_out


def rgbd_stereo(kps, kps_un, depth, bf, device=0):
    """Frame::ComputeStereoFromRGBD on host arrays (one frame): returns (mvuRight, mvDepth)."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    ku = np.ascontiguousarray(kps_un, KEYPOINT_DTYPE)
    d = np.ascontiguousarray(depth, np.float32)
    n = len(k)
    ur, dp = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    _check("orbx_rgbd_stereo",
           lib.orbx_rgbd_stereo(device, k.ctypes.data, ku.ctypes.data, n, _f32p(d), d.shape[0], d.shape[1],
                                d.strides[0], bf, _f32p(ur), _f32p(dp)))
    return ur[:n].copy(), dp[:n].copy()


def frustum_batch_device(pts, npts, pose, params, viewing_cos_limit=0.5, out=None, ninview=None, stream=None):
    """Frame::isInFrustum over a batch: pts (B, pcap, 12) int32 view of MAP_POINT_DTYPE, npts (B,), pose
    (B, 12) float32 mTcw, params: PoseParams.  Returns (proj, ninview): proj (B, pcap, 6) int32 view of
    PROJ_POINT_DTYPE, the d_pts of ORBmatcher's search_by_projection device call, written below each
    frame's npts; ninview (B,) = nToMatch."""
    import torch
    B, pcap = pts.shape[0], pts.shape[1]
    if out is None:
        out = torch.empty((B, pcap, 6), dtype=torch.int32, device=pts.device)
    if ninview is None:
        ninview = torch.empty((B,), dtype=torch.int32, device=pts.device)
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_frustum_batch_device",
           lib.orbm_frustum_batch_device(_ptr(pts), _ptr(npts), B, pcap, _ptr(pose), C.byref(prm),
                                         viewing_cos_limit, _ptr(out), _ptr(ninview), _stream(stream)))
    return out, ninview


def frustum(pts, pose, params, viewing_cos_limit=0.5, device=0):
    """Frame::isInFrustum on host arrays (one frame): pts MAP_POINT_DTYPE, pose 3x4 mTcw.  Returns
    (proj PROJ_POINT_DTYPE[np], nToMatch)."""
    pp = np.ascontiguousarray(pts, MAP_POINT_DTYPE)
    ps = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1)[:12])
    out = np.zeros(max(len(pp), 1), PROJ_POINT_DTYPE)
    nv = C.c_int(0)
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_frustum", lib.orbm_frustum(device, pp.ctypes.data, len(pp), _f32p(ps), C.byref(prm),
                                            viewing_cos_limit, out.ctypes.data, C.byref(nv)))
    return out[:len(pp)].copy(), nv.value


POSE_OPT_DISCARD = 1    # orbm_pose_optimization*: flags
POSE_OPT_INVALID = 1    # status bits
POSE_OPT_TRACE_DTYPE = np.dtype([("iters", "<i4", (4,)), ("rejected", "<i4", (4,)), ("nbad", "<i4", (4,)),
                                 ("rounds", "<i4"), ("ncorr", "<i4")])


def pose_optimization_device(kps, uright, counts, frame_mp, pts, pose, params, flags=0, pose_out=None, outlier=None,
                             frame_outlier=None, ninliers=None, nmatches_map=None, trace=None, status=None,
                             stream=None):
    """Optimizer::PoseOptimization over a batch of Frames: kps (B, fcap, 7) int32 (mvKeysUn), uright (B, fcap)
    float32, counts (B,), frame_mp (B, fcap) int32 (mvpMapPoints as rows of pts, -1 none), pts (nmp, 12) int32 view
    of MAP_POINT_DTYPE, pose (B, 12) or (B, 24) float32 mTcw, params: PoseParams.  outlier (B, fcap) uint8 =
    mvbOutlier, updated for the features with a MapPoint (default: a new zeroed tensor).  trace: (B, 14) int32 view
    of POSE_OPT_TRACE_DTYPE, False for none (default: a new one).  With POSE_OPT_DISCARD frame_mp is updated and
    frame_outlier (B, fcap) int32 written.  Returns (pose_out (B, 12), outlier, frame_outlier, ninliers,
    nmatches_map, trace, status)."""
    import torch
    B, fcap = kps.shape[0], kps.shape[1]
    dev = kps.device
    if pose_out is None:
        pose_out = torch.empty((B, 12), dtype=torch.float32, device=dev)
    if outlier is None:
        outlier = torch.zeros((B, fcap), dtype=torch.uint8, device=dev)
    if frame_outlier is None and flags & POSE_OPT_DISCARD:
        frame_outlier = torch.empty((B, fcap), dtype=torch.int32, device=dev)
    if ninliers is None:
        ninliers = torch.empty((B,), dtype=torch.int32, device=dev)
    if nmatches_map is None:
        nmatches_map = torch.empty((B,), dtype=torch.int32, device=dev)
    if trace is None:
        trace = torch.empty((B, 14), dtype=torch.int32, device=dev)
    elif trace is False:
        trace = None
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=dev)
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_pose_optimization_device",
           lib.orbm_pose_optimization_device(_ptr(kps), _ptr(uright), _ptr(counts), B, fcap, _ptr(frame_mp), _ptr(pts),
                                             pts.shape[0], _ptr(pose), pose.shape[-1], C.byref(prm), flags,
                                             _ptr(pose_out), _ptr(outlier),
                                             _ptr(frame_outlier) if frame_outlier is not None else None,
                                             _ptr(ninliers), _ptr(nmatches_map),
                                             _ptr(trace) if trace is not None else None, _ptr(status),
                                             _stream(stream)))
    return pose_out, outlier, frame_outlier, ninliers, nmatches_map, trace, status


def pose_optimization(kps, uright, frame_mp, pts, pose, params, flags=0, outlier=None, device=0, on_host=False):
    """Optimizer::PoseOptimization on host arrays (one frame): kps KEYPOINT_DTYPE (mvKeysUn), uright float32,
    frame_mp int32, pts MAP_POINT_DTYPE, pose 3x4 mTcw, outlier uint8 = mvbOutlier on entry (default zeros).
    on_host=True runs the kernel's code on the CPU (orbm_pose_optimization_host).  Returns a dict: pose (12,)
    float32, outlier, frame_mp, frame_outlier, ninliers, nmatches_map, trace (POSE_OPT_TRACE_DTYPE scalar), status."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    n = len(k)
    ur = np.ascontiguousarray(uright, np.float32)
    mp = np.array(frame_mp, np.int32).reshape(-1)
    pp = np.ascontiguousarray(pts, MAP_POINT_DTYPE)
    ps = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1)[:12])
    ol = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(-1)
    assert len(ur) == n and len(mp) == n and len(ol) == n
    pad = lambda a: a if n else np.zeros(1, a.dtype)   # noqa: E731
    k, ur, mp, ol = pad(k), pad(ur), pad(mp), pad(ol)
    fo = np.full(max(n, 1), -1, np.int32)
    po = np.zeros(12, np.float32)
    tr = np.zeros(1, POSE_OPT_TRACE_DTYPE)
    ni, nm, st = C.c_int(0), C.c_int(0), C.c_int(0)
    prm = PoseParams.from_buffer_copy(params)
    args = (k.ctypes.data, ur.ctypes.data, n, mp.ctypes.data, pp.ctypes.data if len(pp) else None, len(pp),
            ps.ctypes.data, C.byref(prm), flags, po.ctypes.data, ol.ctypes.data, fo.ctypes.data,
            C.cast(C.byref(ni), C.c_void_p), C.cast(C.byref(nm), C.c_void_p), tr.ctypes.data,
            C.cast(C.byref(st), C.c_void_p))
    if on_host:
        _check("orbm_pose_optimization_host", lib.orbm_pose_optimization_host(*args))
    else:
        _check("orbm_pose_optimization", lib.orbm_pose_optimization(device, *args))
    return dict(pose=po, outlier=ol[:n], frame_mp=mp[:n], frame_outlier=fo[:n], ninliers=ni.value,
                nmatches_map=nm.value, trace=tr[0], status=st.value)


def po_sincos_theta3(theta):
    """(sin, cos, theta ** 3) as the pose optimiser's SE3 exponential evaluates them (host code)."""
    o = (C.c_double * 3)()
    lib.orbx_po_sincos_theta3(float(theta), o)
    return o[0], o[1], o[2]


SIM3_INVALID = 1    # orbm_sim3_*: status bits


def sim3_ransac_iterations(n, probability=0.99, min_inliers=20, max_iterations=300):
    """mRansacMaxIts of Sim3Solver::SetRansacParameters for N = n (src/Sim3Solver.cc:125-135)."""
    return lib.orbm_sim3_ransac_iterations(int(n), float(probability), int(min_inliers), int(max_iterations))


def fixed_atan2(y, x):
    """atan2 as the Sim3 solver evaluates it (host code)."""
    return lib.orbx_fixed_atan2(float(y), float(x))


def sim3_triplet(n, draws):
    """The three correspondences one iteration's raw rand() draws select among n (RandomInt and the removal)."""
    r = np.ascontiguousarray(draws, np.int32).reshape(3)
    o = np.zeros(3, np.int32)
    lib.orbx_sim3_triplet(int(n), r.ctypes.data_as(C.POINTER(C.c_int)), o.ctypes.data_as(C.POINTER(C.c_int)))
    return [int(v) for v in o]


def sim3_solve(kf1, kf2, T1w, T2w, pts, obs_ptr, obs, match12, rand, params, nit, obs_erased=None, fix_scale=False,
               probability=0.99, min_inliers=20, max_iterations=300, iterations=0, best_inliers=0, device=0,
               on_host=False):
    """Sim3Solver on host arrays (one pair): the constructor, SetRansacParameters and one iterate(nit) that starts
    from (iterations, best_inliers).  kf = (mvKeysUn KEYPOINT_DTYPE, GetMapPointMatches() as int32 rows of pts, -1
    none); KeyFrame 1 is slot 0 and KeyFrame 2 slot 1 in obs; T1w / T2w 3x4 Tcw; pts MAP_POINT_DTYPE; obs_ptr
    (nmp + 1,), obs OBSERVATION_DTYPE, obs_erased uint8 or None; match12 (n1,) int32 as SearchByBoW leaves it; rand:
    at least 3 * nit raw rand() values.  on_host=True runs the kernels' code on the CPU (orbm_sim3_solve_host).
    Returns a dict: status, and for a valid solver n, sim3 (13,) float32 = s12, R12, t12 (zeros without a result),
    inliers12 (n1,) uint8, already2 (n2,) uint8, ninliers, nomore, used, iterations, best_inliers."""
    k1, k2 = (np.ascontiguousarray(kf[0], KEYPOINT_DTYPE) for kf in (kf1, kf2))
    m1, m2 = (np.ascontiguousarray(kf[1], np.int32).reshape(-1) for kf in (kf1, kf2))
    n1, n2 = len(k1), len(k2)
    assert len(m1) == n1 and len(m2) == n2
    p = np.ascontiguousarray(pts, MAP_POINT_DTYPE).reshape(-1)
    op = np.ascontiguousarray(obs_ptr, np.int32).reshape(-1)
    ob = np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    er = None if obs_erased is None else np.ascontiguousarray(obs_erased, np.uint8).reshape(-1)
    assert len(op) == len(p) + 1 and (er is None or len(er) == len(ob))
    m12 = np.ascontiguousarray(match12, np.int32).reshape(-1)
    rd = np.ascontiguousarray(rand, np.int32).reshape(-1)
    assert len(m12) == n1 and len(rd) >= 3 * nit
    t1, t2 = (np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1)[:12]) for T in (T1w, T2w))
    sim3 = np.zeros(13, np.float32)
    in12, al2 = np.zeros(max(n1, 1), np.uint8), np.zeros(max(n2, 1), np.uint8)
    ints = [C.c_int(v) for v in (iterations, best_inliers, 0, 0, 0, 0, 0)]
    iv = [C.cast(C.byref(v), C.c_void_p) for v in ints]
    d = lambda a: a.ctypes.data if a is not None and len(a) else None   # noqa: E731
    prm = PoseParams.from_buffer_copy(params)
    args = (d(k1), d(m1), n1, t1.ctypes.data, d(k2), d(m2), n2, t2.ctypes.data, d(p), len(p),
            op.ctypes.data if len(p) else None, d(ob), d(er), d(m12), C.byref(prm), int(bool(fix_scale)),
            float(probability), int(min_inliers), int(max_iterations), int(nit), rd.ctypes.data, iv[0], iv[1], iv[2],
            sim3.ctypes.data, in12.ctypes.data, al2.ctypes.data, iv[3], iv[4], iv[5], iv[6])
    if on_host:
        _check("orbm_sim3_solve_host", lib.orbm_sim3_solve_host(*args))
    else:
        _check("orbm_sim3_solve", lib.orbm_sim3_solve(device, *args))
    if ints[6].value:
        return dict(status=ints[6].value)
    return dict(status=0, n=ints[2].value, sim3=sim3, inliers12=in12[:n1], already2=al2[:n2], ninliers=ints[3].value,
                nomore=ints[4].value, used=ints[5].value, iterations=ints[0].value, best_inliers=ints[1].value)


class Sim3Solver:
    """A batch of ORB_SLAM2::Sim3Solver on the device: one solver per KeyFrame pair, kept in a workspace between
    the calls.  setup() is the constructor and SetRansacParameters, iterate(nit, ...) the reference's iterate of every
    solver, find(...) an iterate over all of mRansacMaxIts.  Tensors live on the device of `kps`."""

    def __init__(self, nsolvers, cap, max_iters_per_call, params, device, probability=0.99, min_inliers=20,
                 max_iterations=300, fix_scale=False):
        import torch
        self.nsolvers, self.cap, self.max_iters = int(nsolvers), int(cap), int(max_iters_per_call)
        self.params = PoseParams.from_buffer_copy(params)
        self.min_inliers, self.max_iterations, self.fix_scale = int(min_inliers), int(max_iterations), bool(fix_scale)
        self.work_bytes = lib.orbm_sim3_workspace_bytes(self.nsolvers, self.cap, self.max_iters)
        if not self.work_bytes and self.nsolvers:
            raise OrbxError("orbm_sim3_workspace_bytes", EINVAL)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)   # noqa: E731
        self.work = torch.zeros((max(self.work_bytes, 16) + 7) // 8, dtype=torch.int64, device=device)
        table = [sim3_ransac_iterations(n, probability, min_inliers, max_iterations) for n in range(self.cap + 1)]
        self.maxits = torch.tensor(table, dtype=torch.int32, device=device)
        self.n, self.iterations, self.best_inliers, self.status = (i32(self.nsolvers) for _ in range(4))
        self.sim3 = torch.zeros((self.nsolvers, 13), dtype=torch.float32, device=device)
        self.inliers12 = torch.zeros((self.nsolvers, self.cap), dtype=torch.uint8, device=device)
        self.already2 = torch.zeros((self.nsolvers, self.cap), dtype=torch.uint8, device=device)
        self.ninliers, self.nomore, self.used = (i32(self.nsolvers) for _ in range(3))

    def setup(self, kps, counts, pose, kf_mp, pts, obs_ptr, obs, pair_a, pair_b, match12, obs_erased=None,
              stream=None):
        """kps (B, cap, 7) int32, counts (B,), pose (B, 12) float32, kf_mp (B, cap) int32, pts (nmp, 12) int32 view of
        MAP_POINT_DTYPE, obs_ptr (nmp + 1,), obs (nobs, 2) int32, pair_a / pair_b (nsolvers,), match12 (nsolvers,
        stride) int32 as bow_search leaves it.  Writes n, iterations = best_inliers = 0 and status."""
        assert kps.shape[1] == self.cap and pair_a.shape[0] == self.nsolvers and match12.shape[0] == self.nsolvers
        _check("orbm_sim3_setup_device",
               lib.orbm_sim3_setup_device(_ptr(kps), _ptr(counts), kps.shape[0], self.cap, _ptr(pose), _ptr(kf_mp),
                                          _ptr(pts), pts.shape[0], _ptr(obs_ptr), _ptr(obs),
                                          _ptr(obs_erased) if obs_erased is not None else None, _ptr(pair_a),
                                          _ptr(pair_b), self.nsolvers, _ptr(match12), match12.shape[1],
                                          C.byref(self.params), _ptr(self.maxits), _ptr(self.work), self.work_bytes,
                                          _ptr(self.n), _ptr(self.iterations), _ptr(self.best_inliers),
                                          _ptr(self.status), _stream(stream)))
        return self.n, self.status

    def iterate(self, nit, rand, rand_off, stream=None):
        """iterate(nit) of every solver: rand int32 raw rand() values, rand_off (nsolvers,) int32 where each solver's
        draws start (3 per iteration).  Returns (sim3, inliers12, already2, ninliers, nomore, used); the state
        tensors iterations / best_inliers are updated."""
        _check("orbm_sim3_iterate_device",
               lib.orbm_sim3_iterate_device(_ptr(self.work), self.work_bytes, self.nsolvers, self.cap,
                                            C.byref(self.params), int(self.fix_scale), self.min_inliers, int(nit),
                                            _ptr(rand), _ptr(rand_off), _ptr(self.iterations),
                                            _ptr(self.best_inliers), _ptr(self.sim3), _ptr(self.inliers12),
                                            _ptr(self.already2), _ptr(self.ninliers), _ptr(self.nomore),
                                            _ptr(self.used), _stream(stream)))
        return self.sim3, self.inliers12, self.already2, self.ninliers, self.nomore, self.used

    def find(self, rand, rand_off, stream=None):
        """Sim3Solver::find: iterate(mRansacMaxIts); needs max_iters_per_call >= max_iterations."""
        return self.iterate(self.max_iterations, rand, rand_off, stream)


OPT_SIM3_INVALID = 1    # orbm_optimize_sim3*: status bits
OPT_SIM3_TRACE_DTYPE = np.dtype([("iters", "<i4", (2,)), ("rejected", "<i4", (2,)), ("nbad", "<i4"), ("ncorr", "<i4"),
                                 ("rounds", "<i4")])


def fixed_exp(x):
    """exp as the Sim3 optimiser evaluates it (host code)."""
    return lib.orbx_fixed_exp(float(x))


def optimize_sim3_device(kps, counts, pose, kf_mp, pts, obs_ptr, obs, pair_a, pair_b, sim3_in, matches1, params,
                         th2=10.0, fix_scale=False, obs_erased=None, sim3_out=None, sim3f_out=None, scw=None, nin=None,
                         trace=None, status=None, stream=None):
    """Optimizer::OptimizeSim3 over a batch of KeyFrame pairs.  Tables as Sim3Solver.setup: kps (B, cap, 7) int32,
    counts (B,), pose (B, 12) float32, kf_mp (B, cap) int32, pts (nmp, 12) int32 view of MAP_POINT_DTYPE, obs_ptr
    (nmp + 1,), obs (nobs, 2) int32, pair_a / pair_b (npairs,).  sim3_in (npairs, 13) float32 = s12, R12, t12;
    matches1 (npairs, stride) int32 = vpMatches1 as rows of pts, updated in place.  sim3f_out, scw and trace: a
    tensor, False for none, None for a new one ((npairs, 13) / (npairs, 12) float32, (npairs, 7) int32 view of
    OPT_SIM3_TRACE_DTYPE); new Sim3 outputs start as zeros and are written only for the pairs that reach the end.
    Returns (sim3_out (npairs, 8) float64, sim3f_out, scw, nin, trace, status)."""
    import torch
    npairs, cap, dev = pair_a.shape[0], kps.shape[1], kps.device
    new = lambda cur, shape, dt: torch.zeros(shape, dtype=dt, device=dev) if cur is None else cur   # noqa: E731
    opt = lambda cur, shape, dt: None if cur is False else new(cur, shape, dt)   # noqa: E731
    sim3_out = new(sim3_out, (npairs, 8), torch.float64)
    sim3f_out = opt(sim3f_out, (npairs, 13), torch.float32)
    scw = opt(scw, (npairs, 12), torch.float32)
    trace = opt(trace, (npairs, 7), torch.int32)
    nin = new(nin, (npairs,), torch.int32)
    status = new(status, (npairs,), torch.int32)
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_optimize_sim3_device",
           lib.orbm_optimize_sim3_device(_ptr(kps), _ptr(counts), kps.shape[0], cap, _ptr(pose), _ptr(kf_mp), _ptr(pts),
                                         pts.shape[0], _ptr(obs_ptr), _ptr(obs), _ptr(obs_erased), _ptr(pair_a),
                                         _ptr(pair_b), npairs, _ptr(sim3_in), _ptr(matches1), matches1.shape[1],
                                         float(th2), int(bool(fix_scale)), C.byref(prm), _ptr(sim3_out),
                                         _ptr(sim3f_out), _ptr(scw), _ptr(nin), _ptr(trace), _ptr(status),
                                         _stream(stream)))
    return sim3_out, sim3f_out, scw, nin, trace, status


def sim3_gather_matches_device(kf_mp, counts, pair_a, pair_b, inliers12, bow_match12, sbs_match12, matches1=None,
                               stream=None):
    """vpMapPointMatches of LoopClosing::ComputeSim3 after SearchBySim3: kf_mp (B, cap) int32, inliers12 (npairs,
    cap) uint8 of Sim3Solver.iterate, bow_match12 (npairs, stride) int32 as given to Sim3Solver.setup, sbs_match12
    (npairs, cap) int32 of search_by_sim3_batch_device.  Returns matches1 (npairs, cap) int32, rows of pts or -1."""
    import torch
    npairs, cap = pair_a.shape[0], kf_mp.shape[1]
    if matches1 is None:
        matches1 = torch.empty((npairs, cap), dtype=torch.int32, device=kf_mp.device)
    _check("orbm_sim3_gather_matches_device",
           lib.orbm_sim3_gather_matches_device(_ptr(kf_mp), _ptr(counts), kf_mp.shape[0], cap, _ptr(pair_a),
                                               _ptr(pair_b), npairs, _ptr(inliers12), _ptr(bow_match12),
                                               bow_match12.shape[1], _ptr(sbs_match12), _ptr(matches1),
                                               matches1.shape[1], _stream(stream)))
    return matches1


def optimize_sim3(kf1, kf2, T1w, T2w, pts, obs_ptr, obs, sim3_in, matches1, params, th2=10.0, fix_scale=False,
                  obs_erased=None, device=0, on_host=False):
    """Optimizer::OptimizeSim3 on host arrays (one pair).  kf1 = (mvKeysUn KEYPOINT_DTYPE, GetMapPointMatches() as
    int32 rows of pts, -1 none), kf2 = (mvKeysUn,); KeyFrame 1 is slot 0 and KeyFrame 2 slot 1 in obs; sim3_in (13,)
    float32 = s12, R12, t12; matches1 (n1,) int32 = vpMatches1 as rows of pts.  on_host=True runs the kernel's code on
    the CPU (orbm_optimize_sim3_host).  Returns a dict: status, and for a valid pair nin, matches1, trace
    (OPT_SIM3_TRACE_DTYPE scalar), written (the reference reached the end) and sim3 (8,) float64 = qx, qy, qz, qw, t,
    s, sim3f (13,), scw (12,), which are NaN unless written."""
    k1, k2 = np.ascontiguousarray(kf1[0], KEYPOINT_DTYPE), np.ascontiguousarray(kf2[0], KEYPOINT_DTYPE)
    m1 = np.ascontiguousarray(kf1[1], np.int32).reshape(-1)
    n1, n2 = len(k1), len(k2)
    p = np.ascontiguousarray(pts, MAP_POINT_DTYPE).reshape(-1)
    op = np.ascontiguousarray(obs_ptr, np.int32).reshape(-1)
    ob = np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    er = None if obs_erased is None else np.ascontiguousarray(obs_erased, np.uint8).reshape(-1)
    mm = np.array(matches1, np.int32).reshape(-1)
    assert len(m1) == n1 and len(mm) == n1 and len(op) == len(p) + 1 and (er is None or len(er) == len(ob))
    t1, t2 = (np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1)[:12]) for T in (T1w, T2w))
    si = np.ascontiguousarray(np.asarray(sim3_in, np.float32).reshape(13))
    so, sf, sc = np.full(8, np.nan), np.full(13, np.nan, np.float32), np.full(12, np.nan, np.float32)
    tr = np.zeros(1, OPT_SIM3_TRACE_DTYPE)
    ni, st = C.c_int(0), C.c_int(0)
    d = lambda a: a.ctypes.data if a is not None and len(a) else None   # noqa: E731
    prm = PoseParams.from_buffer_copy(params)
    args = (d(k1), d(m1), n1, t1.ctypes.data, d(k2), n2, t2.ctypes.data, d(p), len(p),
            op.ctypes.data if len(p) else None, d(ob), d(er), si.ctypes.data, d(mm), float(th2), int(bool(fix_scale)),
            C.byref(prm), so.ctypes.data, sf.ctypes.data, sc.ctypes.data, C.cast(C.byref(ni), C.c_void_p),
            tr.ctypes.data, C.cast(C.byref(st), C.c_void_p))
    if on_host:
        _check("orbm_optimize_sim3_host", lib.orbm_optimize_sim3_host(*args))
    else:
        _check("orbm_optimize_sim3", lib.orbm_optimize_sim3(device, *args))
    if st.value:
        return dict(status=st.value)
    return dict(status=0, nin=ni.value, matches1=mm, trace=tr[0], written=int(tr[0]["rounds"]) == 2, sim3=so,
                sim3f=sf, scw=sc)


PNP_INVALID = 1    # orbm_pnp_*: status bits
# Tracking::Relocalization's SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
PNP_TRACKING = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)
PNP_TRACE_DTYPE = np.dtype([(k, np.int32) for k in ("refine", "N", "b_neg", "b1_neg", "sign_flip", "det_flip",
                                                     "qr_singular", "inliers")])


def pnp_ransac_parameters(n, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """(mRansacMinInliers, mRansacMaxIts) of PnPsolver::SetRansacParameters for N = n (src/PnPsolver.cc:129-152)."""
    a, b = C.c_int(0), C.c_int(0)
    lib.orbm_pnp_ransac_parameters(int(n), float(probability), int(min_inliers), int(max_iterations), int(min_set),
                                   float(epsilon), C.byref(a), C.byref(b))
    return a.value, b.value


def pnp_quad(n, draws):
    """The four correspondences one iteration's raw rand() draws select among n (RandomInt and the removal)."""
    r = np.ascontiguousarray(draws, np.int32).reshape(4)
    o = np.zeros(4, np.int32)
    lib.orbx_pnp_quad(int(n), r.ctypes.data_as(C.POINTER(C.c_int)), o.ctypes.data_as(C.POINTER(C.c_int)))
    return [int(v) for v in o]


def pnp_qr_solve(A, b, x0=None):
    """PnPsolver::qr_solve of a 6x4 system (host code).  Returns (x, ok): ok False where the reference returns early on
    eta == 0, and x is then x0 (zeros by default) unchanged."""
    a = np.array(A, np.float64).reshape(24)
    bb = np.array(b, np.float64).reshape(6)
    x = np.zeros(4) if x0 is None else np.array(x0, np.float64).reshape(4)
    ok = lib.orbx_pnp_qr_solve(a.ctypes.data, bb.ctypes.data, x.ctypes.data)
    return x, bool(ok)


def pnp_svd12(A):
    """cvSVD(A, D, Ut, 0, CV_SVD_MODIFY_A | CV_SVD_U_T) of a 12x12 as the PnP solver evaluates it: (Ut, w)."""
    a = np.ascontiguousarray(A, np.float64).reshape(144)
    ut, w = np.zeros(144), np.zeros(12)
    lib.orbx_pnp_svd12(a.ctypes.data, ut.ctypes.data, w.ctypes.data)
    return ut.reshape(12, 12), w


def pnp_solve(kps, kf_mp, pts, match, rand, params, nit, probability=0.99, min_inliers=10, max_iterations=300,
              min_set=4, epsilon=0.5, th2=5.991, iterations=0, best_inliers=0, state=None, device=0, on_host=False,
              trace=False):
    """PnPsolver on host arrays (one frame, one candidate KeyFrame): the constructor, SetRansacParameters and one
    iterate(nit) that starts from (iterations, best_inliers, state).  kps: the frame's mvKeysUn (KEYPOINT_DTYPE);
    kf_mp: the KeyFrame's GetMapPointMatches() as int32 rows of pts, -1 none; pts MAP_POINT_DTYPE; match (n,) int32 as
    bow_search (ORBM_BOW_KF_F) leaves it; rand: at least 4 * max(nit, max_iterations) raw rand() values.
    on_host=True runs the kernels' code on the CPU (orbm_pnp_solve_host), trace=True also returns its trace.
    Returns a dict: status, and for a valid solver n, tcw (3, 4) float32 (zeros without a pose), has_pose, inliers (n,)
    uint8, ninliers, nomore, used, frame_mp (n,) int32, iterations, best_inliers, state (pass it to the next call)."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE).reshape(-1)
    km = np.ascontiguousarray(kf_mp, np.int32).reshape(-1)
    p = np.ascontiguousarray(pts, MAP_POINT_DTYPE).reshape(-1)
    m = np.ascontiguousarray(match, np.int32).reshape(-1)
    n, nk = len(k), len(km)
    slots = max(int(nit), int(max_iterations))
    rd = np.ascontiguousarray(rand, np.int32).reshape(-1)
    assert len(m) == n and len(rd) >= 4 * slots
    nbytes = lib.orbm_pnp_state_bytes(max(n, nk, 1))
    st = np.zeros((nbytes + 7) // 8, np.int64)
    if state is not None:
        assert state.nbytes == st.nbytes
        st[:] = state
    tcw = np.zeros(12, np.float32)
    inl, fmp = np.zeros(max(n, 1), np.uint8), np.full(max(n, 1), -1, np.int32)
    ints = [C.c_int(v) for v in (iterations, best_inliers, 0, 0, 0, 0, 0, 0, 0)]
    iv = [C.cast(C.byref(v), C.c_void_p) for v in ints]
    d = lambda a: a.ctypes.data if a is not None and len(a) else None   # noqa: E731
    prm = PoseParams.from_buffer_copy(params)
    args = [d(k), n, d(km), nk, d(p), len(p), d(m), C.byref(prm), float(th2), float(probability), int(min_inliers),
            int(max_iterations), int(min_set), float(epsilon), int(nit), rd.ctypes.data, iv[0], iv[1], st.ctypes.data,
            iv[2], tcw.ctypes.data, iv[3], inl.ctypes.data, iv[4], iv[5], iv[6], fmp.ctypes.data, iv[7]]
    tr = None
    if on_host:
        tr = np.zeros(2 * slots + 2, PNP_TRACE_DTYPE)
        _check("orbm_pnp_solve_host", lib.orbm_pnp_solve_host(*args, tr.ctypes.data, len(tr), iv[8]))
        tr = tr[:ints[8].value]
    else:
        _check("orbm_pnp_solve", lib.orbm_pnp_solve(device, *args))
    if ints[7].value:
        return dict(status=ints[7].value)
    out = dict(status=0, n=ints[2].value, tcw=tcw.reshape(3, 4), has_pose=ints[3].value, inliers=inl[:n],
               ninliers=ints[4].value, nomore=ints[5].value, used=ints[6].value, frame_mp=fmp[:n],
               iterations=ints[0].value, best_inliers=ints[1].value, state=st)
    if trace:
        out["trace"] = tr
    return out


class PnPsolver:
    """A batch of ORB_SLAM2::PnPsolver on the device: one solver per (frame, candidate KeyFrame) pair, kept in a
    workspace between the calls.  setup() is the constructor and SetRansacParameters, iterate(nit, ...) the reference's
    iterate of every solver, find(...) iterate(mRansacMaxIts).  Tensors live on `device`."""

    def __init__(self, nsolvers, cap, max_iters_per_call, params, device, probability=0.99, min_inliers=10,
                 max_iterations=300, min_set=4, epsilon=0.5, th2=5.991):
        import torch
        self.nsolvers, self.cap, self.max_iters = int(nsolvers), int(cap), int(max_iters_per_call)
        self.params = PoseParams.from_buffer_copy(params)
        self.max_iterations, self.min_set, self.th2 = int(max_iterations), int(min_set), float(th2)
        self.work_bytes = lib.orbm_pnp_workspace_bytes(self.nsolvers, self.cap, self.max_iters)
        if not self.work_bytes and self.nsolvers:
            raise OrbxError("orbm_pnp_workspace_bytes", EINVAL)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)   # noqa: E731
        self.work = torch.zeros((max(self.work_bytes, 16) + 7) // 8, dtype=torch.int64, device=device)
        table = [pnp_ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon)
                 for n in range(self.cap + 1)]
        self.min_inliers = torch.tensor([t[0] for t in table], dtype=torch.int32, device=device)
        self.maxits = torch.tensor([t[1] for t in table], dtype=torch.int32, device=device)
        self.n, self.iterations, self.best_inliers, self.status = (i32(self.nsolvers) for _ in range(4))
        self.tcw = torch.zeros((self.nsolvers, 12), dtype=torch.float32, device=device)
        self.inliers = torch.zeros((self.nsolvers, self.cap), dtype=torch.uint8, device=device)
        self.frame_mp = torch.full((self.nsolvers, self.cap), -1, dtype=torch.int32, device=device)
        self.has_pose, self.ninliers, self.nomore, self.used = (i32(self.nsolvers) for _ in range(4))

    def setup(self, kps, counts, kf_mp, pts, frame_of, kf_of, match, stream=None):
        """kps (F, cap, 7) int32 view of KEYPOINT_DTYPE, counts (F,), kf_mp (K, cap) int32, pts (nmp, 12) int32 view of
        MAP_POINT_DTYPE, frame_of / kf_of (nsolvers,), match (nsolvers, stride) int32 as bow_search (ORBM_BOW_KF_F)
        leaves it.  Writes n, iterations = best_inliers = 0 and status."""
        assert kps.shape[1] == self.cap and kf_mp.shape[1] == self.cap
        assert frame_of.shape[0] == self.nsolvers and match.shape[0] == self.nsolvers
        _check("orbm_pnp_setup_device",
               lib.orbm_pnp_setup_device(_ptr(kps), _ptr(counts), kps.shape[0], self.cap, _ptr(kf_mp),
                                         kf_mp.shape[0], _ptr(pts), pts.shape[0], _ptr(frame_of), _ptr(kf_of),
                                         self.nsolvers, _ptr(match), match.shape[1], C.byref(self.params), self.th2,
                                         _ptr(self.min_inliers), _ptr(self.maxits), self.max_iterations,
                                         _ptr(self.work), self.work_bytes, _ptr(self.n), _ptr(self.iterations),
                                         _ptr(self.best_inliers), _ptr(self.status), _stream(stream)))
        return self.n, self.status

    def iterate(self, nit, rand, rand_off, stream=None):
        """iterate(nit) of every solver: rand int32 raw rand() values, rand_off (nsolvers,) int32 where each solver's
        draws start (4 per iteration, max(nit, max_iterations) iterations).  Returns (tcw, has_pose, inliers, ninliers,
        nomore, used, frame_mp); the state tensors iterations / best_inliers are updated."""
        _check("orbm_pnp_iterate_device",
               lib.orbm_pnp_iterate_device(_ptr(self.work), self.work_bytes, self.nsolvers, self.cap,
                                           C.byref(self.params), self.min_set, self.max_iterations, int(nit),
                                           _ptr(rand), int(rand.numel()), _ptr(rand_off), _ptr(self.iterations),
                                           _ptr(self.best_inliers), _ptr(self.tcw), _ptr(self.has_pose),
                                           _ptr(self.inliers), _ptr(self.ninliers), _ptr(self.nomore),
                                           _ptr(self.used), _ptr(self.frame_mp), _stream(stream)))
        return self.tcw, self.has_pose, self.inliers, self.ninliers, self.nomore, self.used, self.frame_mp

    def find(self, rand, rand_off, stream=None):
        """PnPsolver::find: iterate(mRansacMaxIts)."""
        return self.iterate(self.max_iterations, rand, rand_off, stream)


INIT_INVALID, INIT_NO_MODEL, INIT_FAILED = 1, 2, 4    # orbm_initialize*: status bits
INIT_PRUNE_MATCHES = 1                                # flag
INIT_F_AMBIGUOUS, INIT_F_PARALLAX, INIT_H_SINGULAR, INIT_H_TEST = 1, 2, 3, 4   # orbm_init_reason
# orbm_init_out: (field, dtype, entries per pair; "cap" = one per frame-1 keypoint, "stride" = the match row)
_INIT_FIELDS = (("status", np.int32, 1), ("model", np.int32, 1), ("reason", np.int32, 1), ("scores", np.float32, 2),
                ("H21", np.float32, 9), ("F21", np.float32, 9), ("inliersH", np.uint8, "cap"),
                ("inliersF", np.uint8, "cap"), ("R21", np.float32, 9), ("t21", np.float32, 3),
                ("p3d", np.float32, "cap3"), ("triangulated", np.uint8, "cap"), ("ngood", np.int32, 8),
                ("parallax", np.float32, 8), ("nmatches_left", np.int32, 1), ("matches_out", np.int32, "stride"))


def fixed_acosf(x):
    """acosf as the Initializer's parallax evaluates it (host code)."""
    return lib.orbx_fixed_acosf(float(x))


def init_sets(n, draws, iterations):
    """mvSets of Initializer::Initialize (:88-120) for n matches from 8 raw rand() values per iteration."""
    r = np.ascontiguousarray(draws, np.int32).reshape(-1)
    assert n >= 8 and len(r) >= 8 * iterations
    o = np.zeros((iterations, 8), np.int32)
    lib.orbx_init_sets(int(n), r.ctypes.data, int(iterations), o.ctypes.data)
    return o


def initialize(kps1, kps2, matches12, draws, params, sigma=1.0, max_iterations=200, prune_matches=False, device=0,
               on_host=False):
    """Initializer::Initialize on host arrays (one pair).  kps1 / kps2: mvKeysUn of the reference and the current
    frame (KEYPOINT_DTYPE); matches12 (n1,) int32 as SearchForInitialization leaves it; draws: 8 * max_iterations raw
    rand() values; params: PoseParams (fx, fy, cx, cy are read).  on_host=True runs the kernels' code on the CPU
    (orbm_initialize_host).  Returns a dict: status, and for a valid pair model, reason, scores (2,), H21, F21, R21
    (9,), t21 (3,), inliersH, inliersF, triangulated (n1,) uint8, p3d (n1, 3), ngood, parallax (8,), nmatches_left and,
    with prune_matches, matches_out (n1,)."""
    k1, k2 = (np.ascontiguousarray(k, KEYPOINT_DTYPE).reshape(-1) for k in (kps1, kps2))
    n1, n2 = len(k1), len(k2)
    m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    rd = np.ascontiguousarray(draws, np.int32).reshape(-1)
    assert len(m12) == n1 and (not 1 <= int(max_iterations) <= 4096 or len(rd) >= 8 * int(max_iterations))
    if not len(rd):
        rd = np.zeros(8, np.int32)
    size = {"cap": max(n1, 1), "cap3": 3 * max(n1, 1), "stride": max(n1, 1)}
    arr = {f: np.zeros(size.get(k, k), dt) for f, dt, k in _INIT_FIELDS}
    out = InitOut(**{f: a.ctypes.data for f, a in arr.items()})
    prm = PoseParams.from_buffer_copy(params)
    d = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
    args = (d(k1), n1, d(k2), n2, d(m12), rd.ctypes.data, C.byref(prm), float(sigma), int(max_iterations),
            INIT_PRUNE_MATCHES if prune_matches else 0, C.byref(out))
    if on_host:
        _check("orbm_initialize_host", lib.orbm_initialize_host(*args))
    else:
        _check("orbm_initialize", lib.orbm_initialize(device, *args))
    st = int(arr["status"][0])
    if st & INIT_INVALID:
        return dict(status=st)
    r = dict(status=st, model=int(arr["model"][0]), reason=int(arr["reason"][0]),
             nmatches_left=int(arr["nmatches_left"][0]), p3d=arr["p3d"][:3 * n1].reshape(n1, 3))
    for f in ("scores", "H21", "F21", "R21", "t21", "ngood", "parallax"):
        r[f] = arr[f]
    for f in ("inliersH", "inliersF", "triangulated"):
        r[f] = arr[f][:n1]
    if prune_matches:
        r["matches_out"] = arr["matches_out"][:n1]
    return r


class Initializer:
    """A batch of ORB_SLAM2::Initializer::Initialize calls on the device, one per frame pair: owns the workspace and
    the output tensors (the fields of orbm_init_out, one row per pair).  Tensors live on `device`."""

    def __init__(self, npairs, cap, params, device, match_stride=None, sigma=1.0, max_iterations=200):
        import torch
        self.npairs, self.cap, self.max_iterations = int(npairs), int(cap), int(max_iterations)
        self.match_stride = int(match_stride) if match_stride is not None else self.cap
        self.sigma = float(sigma)
        self.params = PoseParams.from_buffer_copy(params)
        self.work_bytes = lib.orbm_init_workspace_bytes(self.npairs, self.cap, self.max_iterations)
        if not self.work_bytes and self.npairs:
            raise OrbxError("orbm_init_workspace_bytes", EINVAL)
        self.work = torch.zeros((max(self.work_bytes, 16) + 7) // 8, dtype=torch.int64, device=device)
        size = {"cap": self.cap, "cap3": 3 * self.cap, "stride": self.match_stride}
        tdt = {np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}
        for f, dt, k in _INIT_FIELDS:
            setattr(self, f, torch.zeros((self.npairs, size.get(k, k)), dtype=tdt[dt], device=device))
        self.p3d = self.p3d.view(self.npairs, self.cap, 3)
        self.out = InitOut(**{f: getattr(self, f).data_ptr() for f, _, _ in _INIT_FIELDS})

    def initialize(self, kps, counts, pair_a, pair_b, matches12, draws, max_iterations=None, prune_matches=False,
                   stream=None):
        """kps (B, cap, 7) int32 = mvKeysUn, counts (B,), pair_a / pair_b (npairs,) int32 (reference, current frame),
        matches12 (npairs, match_stride) int32 as search_for_initialization_batch leaves it, draws (npairs, >= 8 *
        max_iterations) int32 raw rand() values.  max_iterations at most the constructor's.  Writes the output
        tensors and returns self."""
        it = self.max_iterations if max_iterations is None else int(max_iterations)
        assert kps.shape[1] == self.cap and pair_a.shape[0] == self.npairs and matches12.shape[0] == self.npairs
        assert matches12.shape[1] == self.match_stride and draws.shape[0] == self.npairs
        _check("orbm_initialize_device",
               lib.orbm_initialize_device(_ptr(kps), _ptr(counts), kps.shape[0], self.cap, _ptr(pair_a), _ptr(pair_b),
                                          self.npairs, _ptr(matches12), self.match_stride, _ptr(draws),
                                          draws.shape[1], C.byref(self.params), self.sigma, it,
                                          INIT_PRUNE_MATCHES if prune_matches else 0, _ptr(self.work),
                                          self.work_bytes, C.byref(self.out), _stream(stream)))
        return self


def refresh_map_points_device(what, kps, desc, counts, pose, kf_bad, obs_ptr, obs, ref, max_obs, params, pts, pdesc,
                              best=None, stream=None):
    """MapPoint::ComputeDistinctiveDescriptors (what & REFRESH_DESCRIPTOR) and UpdateNormalAndDepth (what &
    REFRESH_NORMAL_DEPTH) over device tensors, in place.  KeyFrame table as for search_by_sim3_batch_device: kps
    (B, cap, 7) int32, desc (B, cap, 32) uint8, counts (B,), pose (B, 12) float32 Tcw; kf_bad (B,) uint8 = isBad().
    obs_ptr (np + 1,) int32 and obs (nobs, 2) int32 = each MapPoint's (KeyFrame slot, feature index) list in the
    order of its std::map; ref (np, 2) int32 = (mpRefKF's slot, its feature index); max_obs >= the longest list.
    pts (np, 12) int32 view of MAP_POINT_DTYPE and pdesc (np, 32) uint8 are updated.  Returns best (np,) int32:
    the winner's position in the list, -1 nothing chosen, -2 invalid input (include/orbx.h)."""
    import torch
    n = obs_ptr.shape[0] - 1
    if best is None:
        best = torch.empty((max(n, 1),), dtype=torch.int32, device=pts.device)[:n]
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_refresh_map_points_device",
           lib.orbm_refresh_map_points_device(int(what), _ptr(kps), _ptr(desc), _ptr(counts), kps.shape[0],
                                              kps.shape[1], _ptr(pose), _ptr(kf_bad), _ptr(obs_ptr), _ptr(obs),
                                              _ptr(ref), n, int(max_obs), C.byref(prm), _ptr(pts), _ptr(pdesc),
                                              _ptr(best), _stream(stream)))
    return best


def refresh_map_points(what, kps, desc, counts, pose, kf_bad, obs_ptr, obs, ref, params, pts, pdesc, device=0):
    """The same on host arrays: kps (B, cap) KEYPOINT_DTYPE, desc (B, cap, 32), counts (B,), pose (B, 12) or
    (B, 3, 4), kf_bad (B,), obs_ptr (np + 1,), obs / ref OBSERVATION_DTYPE, pts MAP_POINT_DTYPE, pdesc (np, 32).
    Returns (pts, pdesc, best): refreshed copies and the winners' positions."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    B, cap = (k.shape[0], k.shape[1]) if k.ndim == 2 else (0, 1)
    d = np.ascontiguousarray(desc, np.uint8)
    cn = np.ascontiguousarray(counts, np.int32)
    po = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1))
    bad = np.ascontiguousarray(kf_bad, np.uint8)
    op = np.ascontiguousarray(obs_ptr, np.int32)
    ob = np.ascontiguousarray(obs, OBSERVATION_DTYPE)
    rf = np.ascontiguousarray(ref, OBSERVATION_DTYPE)
    n = len(op) - 1
    p = np.array(pts, MAP_POINT_DTYPE, ndmin=1)
    pd = np.array(pdesc, np.uint8).reshape(-1, 32)
    if not (len(cn) == len(bad) == B and len(po) == 12 * B and d.size == 32 * k.size and len(rf) == len(p) ==
            len(pd) == n and (n == 0 or len(ob) >= op[-1])):
        raise ValueError("refresh_map_points: array sizes disagree")
    best = np.full(max(n, 1), -1, np.int32)
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_refresh_map_points",
           lib.orbm_refresh_map_points(device, int(what), k.ctypes.data, _u8(d), _i32p(cn), B, cap, _f32p(po),
                                       _u8(bad), _i32p(op), ob.ctypes.data, rf.ctypes.data, n, C.byref(prm),
                                       p.ctypes.data, _u8(pd), _i32p(best)))
    return p, pd, best[:n].copy()


# orbm_triang_status (include/orbx.h): what the match loop of CreateNewMapPoints did with a (pair, idx1) entry
(TRI_NO_MATCH, TRI_CREATED_SVD, TRI_CREATED_STEREO1, TRI_CREATED_STEREO2, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_Z1, TRI_Z2,
 TRI_REPROJ1, TRI_REPROJ2, TRI_ZERO_DIST, TRI_SCALE, TRI_INVALID) = range(13)


def triangulate_device(kps, counts, pose, pair_a, pair_b, match, params, kps_raw=None, uright=None, depth=None,
                       kf_rank=None, mark=None, out=None, stream=None):
    """The match loop of LocalMapping::CreateNewMapPoints over device tensors.  KeyFrame table as for
    refresh_map_points_device: kps (B, cap, 7) int32 (mvKeysUn), counts (B,), pose (B, 12) float32 Tcw; kps_raw =
    mvKeys (None = kps), uright / depth (B, cap) float32 (both None = monocular), kf_rank (B,) int32 = the caller's
    std::map order of the KeyFrames (None = slot order).  pair_a / pair_b (npairs,) int32; match (npairs, stride)
    int32 = the output of bow_search_batch_device(TRIANGULATION).  mark: (B, cap) uint8 the views' has_mp point
    into, or None.  out: a dict of preallocated outputs (any subset).  Returns a dict of tensors: x3d (npairs,
    stride, 3) float32 (written for created points only), status (npairs, stride) int32 (TRI_*), and per pair,
    compacted in idx1 order, new_pts (npairs, stride, 12) int32 view of MAP_POINT_DTYPE, new_obs (npairs, stride, 2,
    2), new_ref (npairs, stride, 2), new_idx1 (npairs, stride), nnew (npairs,).  new_pts[p], new_obs[p].view(-1, 2)
    and new_ref[p] are the pts, obs and ref of refresh_map_points_device with obs_ptr = 2 * arange(nnew[p] + 1)."""
    import torch
    B, cap = kps.shape[0], kps.shape[1]
    npairs, stride = match.shape[0], match.shape[1]
    out = dict(out or {})
    dev = kps.device
    shapes = dict(x3d=((npairs, stride, 3), torch.float32), status=((npairs, stride), torch.int32),
                  new_pts=((npairs, stride, 12), torch.int32), new_obs=((npairs, stride, 2, 2), torch.int32),
                  new_ref=((npairs, stride, 2), torch.int32), new_idx1=((npairs, stride), torch.int32),
                  nnew=((npairs,), torch.int32))
    for k, (shape, dt) in shapes.items():
        if out.get(k) is None:
            out[k] = torch.zeros(shape, dtype=dt, device=dev)
        elif tuple(out[k].shape) != shape or out[k].dtype != dt or not out[k].is_contiguous():
            raise ValueError("triangulate_device: out[%r] must be a contiguous %s tensor of shape %s" % (k, dt, shape))
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_triangulate_device",
           lib.orbm_triangulate_device(_ptr(kps), _ptr(kps_raw), _ptr(uright), _ptr(depth), _ptr(counts), B, cap,
                                       _ptr(pose), _ptr(kf_rank), _ptr(pair_a), _ptr(pair_b), npairs, _ptr(match),
                                       stride, C.byref(prm), _ptr(out["x3d"]), _ptr(out["status"]),
                                       _ptr(out["new_pts"]), _ptr(out["new_obs"]), _ptr(out["new_ref"]),
                                       _ptr(out["new_idx1"]), _ptr(out["nnew"]), _ptr(mark), _stream(stream)))
    return out


def triangulate(kps1, pose1, kps2, pose2, match, params, kps1_raw=None, kps2_raw=None, uright1=None, depth1=None,
                uright2=None, depth2=None, mark1=None, mark2=None, x3d=None, device=0):
    """The same for one pair on host arrays: kps KEYPOINT_DTYPE, pose 3x4 Tcw, match (n1,) int32.  Returns a dict:
    x3d (n1, 3) (a copy of the x3d argument, or zeros, with the created points written), status (n1,), new_pts
    MAP_POINT_DTYPE, new_obs (nnew, 2) and new_ref (nnew,) OBSERVATION_DTYPE with KeyFrame 1 as slot 0 and KeyFrame 2
    as slot 1, new_idx1 (nnew,), nnew, and mark1 / mark2 (updated copies) when given."""
    k1, k2 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE), np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
    n1, n2 = len(k1), len(k2)
    m = np.ascontiguousarray(match, np.int32)
    if len(m) != n1:
        raise ValueError("triangulate: match must have one entry per keypoint of KeyFrame 1")
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    kp = lambda a: None if a is None else np.ascontiguousarray(a, KEYPOINT_DTYPE)
    r1, r2, u1, d1, u2, d2 = kp(kps1_raw), kp(kps2_raw), f32(uright1), f32(depth1), f32(uright2), f32(depth2)
    t1 = np.ascontiguousarray(np.asarray(pose1, np.float32).reshape(-1)[:12])
    t2 = np.ascontiguousarray(np.asarray(pose2, np.float32).reshape(-1)[:12])
    room = max(n1, 1)
    x = np.zeros((room, 3), np.float32) if x3d is None else np.array(x3d, np.float32).reshape(-1, 3)
    if len(x) < n1 or any(a is not None and len(a) != n for a, n in ((r1, n1), (u1, n1), (d1, n1), (mark1, n1),
                                                                      (r2, n2), (u2, n2), (d2, n2), (mark2, n2))):
        raise ValueError("triangulate: array sizes disagree")
    status = np.zeros(room, np.int32)
    pts = np.zeros(room, MAP_POINT_DTYPE)
    obs, ref = np.zeros((room, 2), OBSERVATION_DTYPE), np.zeros(room, OBSERVATION_DTYPE)
    idx1 = np.zeros(room, np.int32)
    nnew = C.c_int(0)
    mk1 = None if mark1 is None else np.array(mark1, np.uint8)
    mk2 = None if mark2 is None else np.array(mark2, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data
    fp = lambda a: None if a is None else _f32p(a)
    prm = PoseParams.from_buffer_copy(params)
    _check("orbm_triangulate",
           lib.orbm_triangulate(device, vp(k1), vp(r1), fp(u1), fp(d1), n1, _f32p(t1), vp(k2), vp(r2), fp(u2), fp(d2),
                                n2, _f32p(t2), _i32p(m), C.byref(prm), _f32p(x), _i32p(status), pts.ctypes.data,
                                obs.ctypes.data, ref.ctypes.data, _i32p(idx1), C.byref(nnew),
                                None if mk1 is None else _u8(mk1), None if mk2 is None else _u8(mk2)))
    k = nnew.value
    return dict(x3d=x[:n1], status=status[:n1], new_pts=pts[:k].copy(), new_obs=obs[:k].copy(), new_ref=ref[:k].copy(),
                new_idx1=idx1[:k].copy(), nnew=k, mark1=mk1, mark2=mk2)


# d_status bits of orbm_local_map_device (include/orbx.h) and the KeyFrame count up to which votes are counted in LDS
LOCAL_MAP_KF_TRUNCATED, LOCAL_MAP_POINTS_TRUNCATED, LOCAL_MAP_INVALID = 1, 2, 4
LOCAL_MAP_LDS_KEYFRAMES = 8192


def local_map_work_bytes(nkf, nmp, nframes, kfcap):
    """orbm_local_map_work_bytes: the scratch one local_map_device call is handed (0 for sizes the call refuses)."""
    return int(lib.orbm_local_map_work_bytes(int(nkf), int(nmp), int(nframes), int(kfcap)))


def local_map_work(nkf, nmp, nframes, kfcap, device):
    """A zeroed scratch tensor for local_map_device; every call leaves it zeroed, so it is made once."""
    import torch
    nbytes = local_map_work_bytes(nkf, nmp, nframes, kfcap)
    if nbytes == 0:
        raise ValueError("local_map_work: sizes out of range")
    return torch.zeros(((nbytes + 3) // 4,), dtype=torch.int32, device=device)


def local_map_device(counts, kf_mp, kf_bad, covis, child_ptr, child, parent, pts, pdesc, obs_ptr, obs, fcounts,
                     frame_mp, local_kf, nlocal_kf, ref_kf, pcap, work, kf_rank=None, frame_outlier=None, out=None,
                     stream=None):
    """Tracking::UpdateLocalMap and the first loop of SearchLocalPoints over device tensors (include/orbx.h).
    KeyFrame table: counts (nkf,), kf_mp (nkf, cap) int32 MapPoint indices or -1, kf_bad (nkf,) uint8, covis
    (nkf, 10) int32 padded with -1, child_ptr (nkf + 1,) / child int32, parent (nkf,) int32, kf_rank (nkf,) int32 or
    None = slot order.  MapPoint table: pts (nmp, 12) int32 view of MAP_POINT_DTYPE, pdesc (nmp, 32) uint8, obs_ptr
    (nmp + 1,), obs (nobs, 2) int32.  Frames: fcounts (B,), frame_mp (B, fcap) int32 (bad MapPoints are nulled in
    place), frame_outlier (B, fcap) int32 or None.  local_kf (B, kfcap) int32, nlocal_kf (B,) and ref_kf (B,) hold
    the previous list and reference KeyFrame and are updated in place.  work: local_map_work(...).  out: a dict of
    preallocated outputs (any subset).  Returns a dict of tensors: local_mp (B, pcap), nlocal (B,), out_pts
    (B, pcap, 12) and out_pdesc (B, pcap, 32) -- the pts / npts of frustum_batch_device and the pdesc of the
    projection search -- claimed (B, fcap) uint8 and status (B,) (LOCAL_MAP_* bits, 0 = faithful)."""
    import torch
    nkf, cap = kf_mp.shape[0], kf_mp.shape[1]
    nmp = obs_ptr.shape[0] - 1
    B, fcap = frame_mp.shape[0], frame_mp.shape[1]
    kfcap = local_kf.shape[1]
    out = dict(out or {})
    dev = frame_mp.device
    shapes = dict(local_mp=((B, pcap), torch.int32), nlocal=((B,), torch.int32),
                  out_pts=((B, pcap, 12), torch.int32), out_pdesc=((B, pcap, 32), torch.uint8),
                  claimed=((B, fcap), torch.uint8), status=((B,), torch.int32))
    for k, (shape, dt) in shapes.items():
        if out.get(k) is None:
            out[k] = torch.zeros(shape, dtype=dt, device=dev)
        elif tuple(out[k].shape) != shape or out[k].dtype != dt or not out[k].is_contiguous():
            raise ValueError("local_map_device: out[%r] must be a contiguous %s tensor of shape %s" % (k, dt, shape))
    _check("orbm_local_map_device",
           lib.orbm_local_map_device(_ptr(counts), _ptr(kf_mp), _ptr(kf_bad), _ptr(kf_rank), _ptr(covis),
                                     _ptr(child_ptr), _ptr(child), _ptr(parent), nkf, cap, _ptr(pts), _ptr(pdesc),
                                     _ptr(obs_ptr), _ptr(obs), nmp, _ptr(fcounts), _ptr(frame_mp),
                                     _ptr(frame_outlier), B, fcap, _ptr(local_kf), _ptr(nlocal_kf), kfcap,
                                     _ptr(ref_kf), _ptr(out["local_mp"]), _ptr(out["nlocal"]), _ptr(out["out_pts"]),
                                     _ptr(out["out_pdesc"]), int(pcap), _ptr(out["claimed"]), _ptr(out["status"]),
                                     _ptr(work), work.numel() * work.element_size(), _stream(stream)))
    return out


def local_map(counts, kf_mp, kf_bad, covis, child_ptr, child, parent, pts, pdesc, obs_ptr, obs, frame_mp, local_kf,
              ref_kf, kfcap, pcap, kf_rank=None, frame_outlier=None, out=None, device=0):
    """The same for one frame on host arrays: frame_mp (n,) int32, local_kf the previous list (any length <= kfcap),
    ref_kf the previous reference KeyFrame.  out: optional dict of local_kf (kfcap,), local_mp (pcap,), out_pts
    (pcap,) MAP_POINT_DTYPE, out_pdesc (pcap, 32) and claimed (n,) whose contents stand where the call writes
    nothing.  Returns a dict: frame_mp (the cleaned copy), local_kf (kfcap,), nlocal_kf, ref_kf, local_mp, nlocal,
    out_pts, out_pdesc, claimed, status."""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    cn, km, bad = i32(counts), i32(kf_mp), np.ascontiguousarray(kf_bad, np.uint8)
    nkf, cap = (km.shape[0], km.shape[1]) if km.ndim == 2 else (0, 1)
    cv, cp, ch, pa = i32(covis).reshape(-1), i32(child_ptr), i32(child).reshape(-1), i32(parent)
    p = np.ascontiguousarray(pts, MAP_POINT_DTYPE).reshape(-1)
    pd = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
    op, ob = i32(obs_ptr), np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    nmp = len(op) - 1
    fm = np.array(frame_mp, np.int32).reshape(-1)
    n = len(fm)
    rk = None if kf_rank is None else i32(kf_rank)
    fo = None if frame_outlier is None else i32(frame_outlier).reshape(-1)
    prev = i32(local_kf).reshape(-1)
    if not (len(cn) == len(bad) == len(pa) == nkf and len(cv) == 10 * nkf and len(cp) == nkf + 1 and
            len(p) == len(pd) == nmp and (rk is None or len(rk) == nkf) and (fo is None or len(fo) == n) and
            len(prev) <= kfcap):
        raise ValueError("local_map: array sizes disagree")
    out = dict(out or {})
    lk = np.array(out["local_kf"], np.int32) if out.get("local_kf") is not None else np.zeros(kfcap, np.int32)
    lk[:len(prev)] = prev
    lm = np.array(out["local_mp"], np.int32) if out.get("local_mp") is not None else np.zeros(pcap, np.int32)
    opt = (np.array(out["out_pts"], MAP_POINT_DTYPE) if out.get("out_pts") is not None
           else np.zeros(pcap, MAP_POINT_DTYPE))
    opd = (np.array(out["out_pdesc"], np.uint8).reshape(-1, 32) if out.get("out_pdesc") is not None
           else np.zeros((pcap, 32), np.uint8))
    cl = np.array(out["claimed"], np.uint8) if out.get("claimed") is not None else np.zeros(max(n, 1), np.uint8)
    if not (len(lk) == kfcap and len(lm) == len(opt) == len(opd) == pcap and len(cl) >= n):
        raise ValueError("local_map: out array sizes disagree")
    nlk, ref, nl, st = C.c_int(len(prev)), C.c_int(int(ref_kf)), C.c_int(0), C.c_int(0)
    ip = lambda a: None if a is None or a.size == 0 else _i32p(a)
    _check("orbm_local_map",
           lib.orbm_local_map(device, ip(cn), ip(km), _u8(bad) if nkf else None, ip(rk), ip(cv), _i32p(cp), ip(ch),
                              ip(pa), nkf, cap, p.ctypes.data if nmp else None, _u8(pd) if nmp else None, _i32p(op),
                              ob.ctypes.data if ob.size else None, nmp, n, ip(fm), ip(fo), _i32p(lk), C.byref(nlk),
                              kfcap, C.byref(ref), _i32p(lm), C.byref(nl), opt.ctypes.data, _u8(opd), pcap, _u8(cl),
                              C.byref(st)))
    return dict(frame_mp=fm, local_kf=lk, nlocal_kf=nlk.value, ref_kf=ref.value, local_mp=lm, nlocal=nl.value,
                out_pts=opt, out_pdesc=opd, claimed=cl[:n], status=st.value)


# d_status values of orbm_update_connections_device / orbm_erase_connections_device (include/orbx.h) and the row limit
CONN_EMPTY, CONN_NOSPC, CONN_INVALID = 1, 2, 4
MAX_CONNECTIONS = 4096
_GRAPH_FIELDS = ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent", "first")


def covis_graph(nkf, ccap, device=None):
    """An empty covisibility graph of nkf slots at row stride ccap: a dict of conn_kf / conn_w / ord_kf / ord_w
    (nkf, ccap) int32, nconn / nord (nkf,) int32, parent (nkf,) int32 filled with -1 and first (nkf,) uint8 filled
    with 1 (mbFirstConnection).  Torch tensors on `device`, numpy arrays when device is None."""
    if device is None:
        g = {k: np.zeros((nkf, ccap), np.int32) for k in ("conn_kf", "conn_w", "ord_kf", "ord_w")}
        g.update(nconn=np.zeros(nkf, np.int32), nord=np.zeros(nkf, np.int32), parent=np.full(nkf, -1, np.int32),
                 first=np.ones(nkf, np.uint8))
        return g
    import torch
    g = {k: torch.zeros((nkf, ccap), dtype=torch.int32, device=device) for k in ("conn_kf", "conn_w", "ord_kf", "ord_w")}
    g.update(nconn=torch.zeros(nkf, dtype=torch.int32, device=device),
             nord=torch.zeros(nkf, dtype=torch.int32, device=device),
             parent=torch.full((nkf,), -1, dtype=torch.int32, device=device),
             first=torch.ones(nkf, dtype=torch.uint8, device=device))
    return g


def _graph_dims(fn, g):
    if sorted(g) != sorted(_GRAPH_FIELDS):
        raise ValueError("%s: the graph must hold exactly %s" % (fn, ", ".join(_GRAPH_FIELDS)))
    if g["conn_kf"].ndim != 2:
        raise ValueError("%s: conn_kf must be (nkf, ccap)" % fn)
    nkf, ccap = int(g["conn_kf"].shape[0]), int(g["conn_kf"].shape[1])
    for k in _GRAPH_FIELDS:
        want = (nkf, ccap) if k in ("conn_kf", "conn_w", "ord_kf", "ord_w") else (nkf,)
        if tuple(g[k].shape) != want:
            raise ValueError("%s: graph[%r] must have shape %s" % (fn, k, want))
    return nkf, ccap


def _graph_device(fn, g):
    """(CovisGraph of device pointers, nkf, ccap) of a dict of contiguous torch tensors."""
    import torch
    nkf, ccap = _graph_dims(fn, g)
    for k in _GRAPH_FIELDS:
        dt = torch.uint8 if k == "first" else torch.int32
        if g[k].dtype != dt or not g[k].is_contiguous():
            raise ValueError("%s: graph[%r] must be a contiguous %s tensor" % (fn, k, dt))
    return CovisGraph(*[g[k].data_ptr() for k in _GRAPH_FIELDS]), nkf, ccap


def connections_work_bytes(nkf, ccap):
    """orbm_connections_work_bytes: the scratch of one update / erase call (0 for sizes the calls refuse)."""
    return int(lib.orbm_connections_work_bytes(int(nkf), int(ccap)))


def connections_work(nkf, ccap, device):
    """A zeroed scratch tensor for update_connections_device / erase_connections_device; every call leaves it zeroed."""
    import torch
    nbytes = connections_work_bytes(nkf, ccap)
    if nbytes == 0:
        raise ValueError("connections_work: sizes out of range")
    return torch.zeros(((nbytes + 3) // 4,), dtype=torch.int32, device=device)


def _work_bytes(work):
    return work.numel() * work.element_size()


def update_connections_device(graph, counts, kf_mp, pts, obs_ptr, obs, targets, work, th=15, root=-1, kf_rank=None,
                              status=None, stream=None):
    """KeyFrame::UpdateConnections for targets (int32 tensor of slots, run in sequence) over device tensors
    (include/orbx.h).  graph: covis_graph(...), updated in place.  counts (nkf,), kf_mp (nkf, cap), kf_rank (nkf,) or
    None, pts (nmp, 12) int32 view of MAP_POINT_DTYPE, obs_ptr (nmp + 1,), obs (nobs, 2) as in local_map_device.
    work: connections_work(...).  Returns status (ntargets,) int32: 0, CONN_EMPTY, CONN_NOSPC or CONN_INVALID."""
    import torch
    g, nkf, ccap = _graph_device("update_connections_device", graph)
    if kf_mp.ndim != 2 or kf_mp.shape[0] != nkf:
        raise ValueError("update_connections_device: kf_mp must be (nkf, cap)")
    nt = int(targets.shape[0])
    if status is None:
        status = torch.zeros((max(nt, 1),), dtype=torch.int32, device=targets.device)[:nt]
    elif tuple(status.shape) != (nt,) or status.dtype != torch.int32 or not status.is_contiguous():
        raise ValueError("update_connections_device: status must be a contiguous int32 tensor of shape (%d,)" % nt)
    _check("orbm_update_connections_device",
           lib.orbm_update_connections_device(C.byref(g), nkf, ccap, _ptr(counts), _ptr(kf_mp), int(kf_mp.shape[1]),
                                              _ptr(kf_rank), _ptr(pts), _ptr(obs_ptr), _ptr(obs),
                                              int(obs_ptr.shape[0]) - 1, _ptr(targets), nt, int(th), int(root),
                                              _ptr(status), _ptr(work), _work_bytes(work), _stream(stream)))
    return status


def erase_connections_device(graph, targets, work, kf_rank=None, status=None, stream=None):
    """The connection part of KeyFrame::SetBadFlag for targets in sequence (include/orbx.h); graph is updated in
    place.  Returns status (ntargets,) int32: 0 or CONN_INVALID."""
    import torch
    g, nkf, ccap = _graph_device("erase_connections_device", graph)
    nt = int(targets.shape[0])
    if status is None:
        status = torch.zeros((max(nt, 1),), dtype=torch.int32, device=targets.device)[:nt]
    elif tuple(status.shape) != (nt,) or status.dtype != torch.int32 or not status.is_contiguous():
        raise ValueError("erase_connections_device: status must be a contiguous int32 tensor of shape (%d,)" % nt)
    _check("orbm_erase_connections_device",
           lib.orbm_erase_connections_device(C.byref(g), nkf, ccap, _ptr(kf_rank), _ptr(targets), nt, _ptr(status),
                                             _ptr(work), _work_bytes(work), _stream(stream)))
    return status


def _getter_out(fn, out, shape, dt, device):
    import torch
    if out is None:
        return torch.zeros(shape, dtype=dt, device=device)
    if tuple(out.shape) != shape or out.dtype != dt or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous %s tensor of shape %s" % (fn, dt, shape))
    return out


def best_covisibles_device(graph, N, out=None, stream=None):
    """GetBestCovisibilityKeyFrames(N) of every slot, (nkf, N) int32 padded with -1: with N = 10 the covis of
    local_map_device and of the KeyFrameDatabase's device detection."""
    import torch
    g, nkf, ccap = _graph_device("best_covisibles_device", graph)
    out = _getter_out("best_covisibles_device", out, (nkf, int(N)), torch.int32, graph["nord"].device)
    _check("orbm_best_covisibles_device",
           lib.orbm_best_covisibles_device(C.byref(g), nkf, ccap, int(N), _ptr(out), _stream(stream)))
    return out


def connected_mask_device(graph, t, out=None, stream=None):
    """The membership of GetConnectedKeyFrames() of slot t, (nkf,) uint8: the connected of detect_loop_device."""
    import torch
    g, nkf, ccap = _graph_device("connected_mask_device", graph)
    out = _getter_out("connected_mask_device", out, (nkf,), torch.uint8, graph["nconn"].device)
    _check("orbm_connected_mask_device",
           lib.orbm_connected_mask_device(C.byref(g), nkf, ccap, int(t), _ptr(out), _stream(stream)))
    return out


def covisibles_by_weight_device(graph, w, out=None, stream=None):
    """The length GetCovisiblesByWeight(w) returns for every slot, (nkf,) int32 (0 when every weight is >= w, as in
    the reference); the KeyFrames are graph["ord_kf"][f, :n]."""
    import torch
    g, nkf, ccap = _graph_device("covisibles_by_weight_device", graph)
    out = _getter_out("covisibles_by_weight_device", out, (nkf,), torch.int32, graph["nord"].device)
    _check("orbm_covisibles_by_weight_device",
           lib.orbm_covisibles_by_weight_device(C.byref(g), nkf, ccap, int(w), _ptr(out), _stream(stream)))
    return out


def children_work_bytes(nkf):
    """orbm_children_work_bytes: the scratch of one children_device call (0 for sizes the call refuses)."""
    return int(lib.orbm_children_work_bytes(int(nkf)))


def children_work(nkf, device):
    """A zeroed scratch tensor for children_device; every call leaves it zeroed."""
    import torch
    nbytes = children_work_bytes(nkf)
    if nbytes == 0:
        raise ValueError("children_work: sizes out of range")
    return torch.zeros(((nbytes + 3) // 4,), dtype=torch.int32, device=device)


def children_device(parent, kf_bad, work, kf_rank=None, out=None, stream=None):
    """GetChilds() of every slot as the CSR local_map_device reads.  parent (nkf,) int32, kf_bad (nkf,) uint8,
    kf_rank (nkf,) int32 or None.  out: optional dict of child_ptr (nkf + 1,), child (nkf,) and status (1,) int32.
    Returns that dict; status[0] is 0 or CONN_INVALID (then child_ptr and child are untouched)."""
    import torch
    nkf = int(parent.shape[0])
    out = dict(out or {})
    for k, n in (("child_ptr", nkf + 1), ("child", max(nkf, 1)), ("status", 1)):
        out[k] = _getter_out("children_device", out.get(k), (n,), torch.int32, parent.device)
    _check("orbm_children_device",
           lib.orbm_children_device(_ptr(parent), _ptr(kf_bad), _ptr(kf_rank), nkf, _ptr(out["child_ptr"]),
                                    _ptr(out["child"]), _ptr(out["status"]), _ptr(work), _work_bytes(work),
                                    _stream(stream)))
    return out


def update_connections(graph, counts, kf_mp, pts, obs_ptr, obs, targets, th=15, root=-1, kf_rank=None, status=None,
                       device=0):
    """The same as update_connections_device on host arrays; synchronous.  graph: a dict of contiguous numpy arrays
    as covis_graph(nkf, ccap) makes them, updated in place.  status: optional (ntargets,) int32 whose contents stand
    where the call writes nothing.  Returns status."""
    nkf, ccap = _graph_dims("update_connections", graph)
    for k in _GRAPH_FIELDS:
        dt = np.uint8 if k == "first" else np.int32
        if not isinstance(graph[k], np.ndarray) or graph[k].dtype != dt or not graph[k].flags.c_contiguous:
            raise ValueError("update_connections: graph[%r] must be a contiguous %s array" % (k, np.dtype(dt)))
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    cn, km = i32(counts), i32(kf_mp)
    p = np.ascontiguousarray(pts, MAP_POINT_DTYPE).reshape(-1)
    op, ob = i32(obs_ptr), np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    nmp = len(op) - 1
    tg = i32(targets).reshape(-1)
    rk = None if kf_rank is None else i32(kf_rank)
    if not (km.ndim == 2 and km.shape[0] == nkf and len(cn) == nkf and len(p) == nmp and
            (rk is None or len(rk) == nkf)):
        raise ValueError("update_connections: array sizes disagree")
    st = np.zeros(len(tg), np.int32) if status is None else status
    if st.dtype != np.int32 or st.shape != (len(tg),) or not st.flags.c_contiguous:
        raise ValueError("update_connections: status must be a contiguous int32 array of shape (%d,)" % len(tg))
    g = CovisGraph(*[graph[k].ctypes.data for k in _GRAPH_FIELDS])
    ip = lambda a: None if a is None or a.size == 0 else _i32p(a)
    _check("orbm_update_connections",
           lib.orbm_update_connections(device, C.byref(g), nkf, ccap, ip(cn), ip(km), int(km.shape[1]), ip(rk),
                                       p.ctypes.data if nmp else None, _i32p(op), ob.ctypes.data if ob.size else None,
                                       nmp, ip(tg), len(tg), int(th), int(root), ip(st)))
    return st


# d_verdict values of orbm_map_point_culling_device and orbm_keyframe_culling_device (include/orbx.h)
CULL_KEPT, CULL_ERASED_BAD, CULL_RATIO, CULL_OBS, CULL_DROPPED_OLD, CULL_INVALID = 0, 1, 2, 3, 4, 5
KFCULL_KEPT, KFCULL_SKIP_ROOT, KFCULL_CULLED, KFCULL_TO_BE_ERASED, KFCULL_INVALID = 0, 1, 2, 3, 4


def culling_work_bytes(nmp):
    """orbm_culling_work_bytes: the scratch of one keyframe_culling_device call (0 for sizes the call refuses)."""
    return int(lib.orbm_culling_work_bytes(int(nmp)))


def culling_work(nmp, device):
    """A zeroed scratch tensor for keyframe_culling_device; every call leaves it zeroed."""
    import torch
    nbytes = culling_work_bytes(nmp)
    if nbytes == 0:
        raise ValueError("culling_work: sizes out of range")
    return torch.zeros(((nbytes + 3) // 4,), dtype=torch.int32, device=device)


def _cull_out(fn, out, shapes, device):
    import torch
    out = dict(out or {})
    for k, shape in shapes.items():
        out[k] = _getter_out(fn, out.get(k), shape, torch.int32, device)
    return out


def map_point_culling_device(recent, cur_kfid, th_obs, counts, kf_mp, pts, obs_ptr, obs, obs_erased, nobs, found,
                             visible, first_kfid, out=None, stream=None):
    """LocalMapping::MapPointCulling over device tensors (include/orbx.h).  recent (nrecent,) int32 MapPoint indices;
    counts (nkf,), kf_mp (nkf, cap), pts (nmp, 12) int32 view of MAP_POINT_DTYPE, obs_ptr (nmp + 1,), obs (nobs, 2) as
    in local_map_device; obs_erased (nobs,) uint8; nobs, found, visible, first_kfid (nmp,) int32.  kf_mp, pts and
    obs_erased are updated in place.  out: optional dict of verdict (nrecent,), recent_out (nrecent,) and nrecent_out
    (1,) int32.  Returns that dict: verdict holds CULL_*, recent_out[:nrecent_out] the KEPT points in list order."""
    if kf_mp.ndim != 2:
        raise ValueError("map_point_culling_device: kf_mp must be (nkf, cap)")
    nr = int(recent.shape[0])
    out = _cull_out("map_point_culling_device", out, dict(verdict=(nr,), recent_out=(nr,), nrecent_out=(1,)),
                    kf_mp.device)
    _check("orbm_map_point_culling_device",
           lib.orbm_map_point_culling_device(_ptr(recent), nr, int(cur_kfid), int(th_obs), _ptr(counts), _ptr(kf_mp),
                                             int(kf_mp.shape[0]), int(kf_mp.shape[1]), _ptr(pts), _ptr(obs_ptr),
                                             _ptr(obs), _ptr(obs_erased), int(obs_ptr.shape[0]) - 1, _ptr(nobs),
                                             _ptr(found), _ptr(visible), _ptr(first_kfid), _ptr(out["verdict"]),
                                             _ptr(out["recent_out"]), _ptr(out["nrecent_out"]), _stream(stream)))
    return out


def keyframe_culling_device(graph, t, counts, kf_mp, kps, depth, th_depth, stereo, nlevels, kf_noterase, pts, obs_ptr,
                            obs, obs_erased, ref, nobs, work, root=-1, uright=None, out=None, stream=None):
    """LocalMapping::KeyFrameCulling of KeyFrame t over device tensors (include/orbx.h): the candidates are
    graph["ord_kf"][t, :graph["nord"][t]], processed as if one after another.  kps (nkf, cap, 7) int32 view of
    KEYPOINT_DTYPE, uright / depth (nkf, cap) float32 (uright None = monocular; depth may be None unless stereo),
    kf_noterase (nkf,) uint8, ref (nmp, 2) int32, the rest as in map_point_culling_device.  kf_mp, pts, obs_erased,
    ref and nobs are updated in place.  work: culling_work(nmp, ...).  out: optional dict of verdict, nmps, nred,
    culled (ccap,), nculled and ncand (1,) int32.  Returns that dict: verdict holds KFCULL_*, culled the targets of
    erase_connections_device (-1 where a candidate was not culled)."""
    g, nkf, ccap = _graph_device("keyframe_culling_device", graph)
    if kf_mp.ndim != 2 or kf_mp.shape[0] != nkf:
        raise ValueError("keyframe_culling_device: kf_mp must be (nkf, cap)")
    out = _cull_out("keyframe_culling_device", out,
                    dict(verdict=(ccap,), nmps=(ccap,), nred=(ccap,), culled=(ccap,), nculled=(1,), ncand=(1,)),
                    kf_mp.device)
    _check("orbm_keyframe_culling_device",
           lib.orbm_keyframe_culling_device(C.byref(g), nkf, ccap, int(t), int(root), _ptr(counts), _ptr(kf_mp),
                                            int(kf_mp.shape[1]), _ptr(kps), _ptr(uright), _ptr(depth),
                                            float(th_depth), int(bool(stereo)), int(nlevels), _ptr(kf_noterase),
                                            _ptr(pts), _ptr(obs_ptr), _ptr(obs), _ptr(obs_erased), _ptr(ref),
                                            _ptr(nobs), int(obs_ptr.shape[0]) - 1, _ptr(out["verdict"]),
                                            _ptr(out["nmps"]), _ptr(out["nred"]), _ptr(out["culled"]),
                                            _ptr(out["nculled"]), _ptr(out["ncand"]), _ptr(work), _work_bytes(work),
                                            _stream(stream)))
    return out


def compact_observations_device(obs_ptr, obs, obs_erased, out=None, stream=None):
    """The stable compaction of the observation CSR under the erased mask (include/orbx.h).  out: optional dict of
    obs_ptr (nmp + 1,), obs (nobs, 2) and status (1,) int32.  Returns that dict: the CSR the refresh, the local map
    and update_connections_device read next; status[0] is 0 or CONN_INVALID."""
    import torch
    out = dict(out or {})
    dev = obs_ptr.device
    out["obs_ptr"] = _getter_out("compact_observations_device", out.get("obs_ptr"), tuple(obs_ptr.shape), torch.int32,
                                 dev)
    out["obs"] = _getter_out("compact_observations_device", out.get("obs"), tuple(obs.shape), torch.int32, dev)
    out["status"] = _getter_out("compact_observations_device", out.get("status"), (1,), torch.int32, dev)
    _check("orbm_compact_observations_device",
           lib.orbm_compact_observations_device(_ptr(obs_ptr), _ptr(obs), _ptr(obs_erased), int(obs_ptr.shape[0]) - 1,
                                                _ptr(out["obs_ptr"]), _ptr(out["obs"]), _ptr(out["status"]),
                                                _stream(stream)))
    return out


def _inout(fn, name, a, dt, shape=None):
    if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or \
            (shape is not None and a.shape != shape):
        raise ValueError("%s: %s must be a contiguous %s array%s" %
                         (fn, name, np.dtype(dt), "" if shape is None else " of shape %s" % (shape,)))
    return a


def _vp(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def map_point_culling(recent, cur_kfid, th_obs, counts, kf_mp, pts, obs_ptr, obs, obs_erased, nobs, found, visible,
                      first_kfid, out=None, device=0):
    """The same as map_point_culling_device on host arrays; synchronous.  kf_mp (nkf, cap) int32, pts MAP_POINT_DTYPE
    and obs_erased uint8 must be contiguous numpy arrays and are updated in place.  out: optional dict of verdict and
    recent_out (nrecent,) int32 whose contents stand where the call writes nothing.  Returns a dict of verdict,
    recent_out and nrecent_out (an int)."""
    fn = "map_point_culling"
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    rc, cn, op = i32(recent), i32(counts), i32(obs_ptr)
    nmp = len(op) - 1
    km = _inout(fn, "kf_mp", kf_mp, np.int32)
    p = _inout(fn, "pts", pts, MAP_POINT_DTYPE, (nmp,))
    ob = np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    er = _inout(fn, "obs_erased", obs_erased, np.uint8, (len(ob),))
    no, fo, vi, fk = i32(nobs), i32(found), i32(visible), i32(first_kfid)
    if not (km.ndim == 2 and len(cn) == km.shape[0] and len(no) == len(fo) == len(vi) == len(fk) == nmp):
        raise ValueError("map_point_culling: array sizes disagree")
    out = dict(out or {})
    for k in ("verdict", "recent_out"):
        out[k] = np.zeros(len(rc), np.int32) if out.get(k) is None else _inout(fn, k, out[k], np.int32, (len(rc),))
    n = C.c_int(0)
    _check("orbm_map_point_culling",
           lib.orbm_map_point_culling(device, _vp(rc), len(rc), int(cur_kfid), int(th_obs), _vp(cn), _vp(km),
                                      km.shape[0], km.shape[1], _vp(p), _vp(op), _vp(ob), _vp(er), nmp, _vp(no),
                                      _vp(fo), _vp(vi), _vp(fk), _vp(out["verdict"]), _vp(out["recent_out"]),
                                      C.addressof(n)))
    out["nrecent_out"] = n.value
    return out


def keyframe_culling(graph, t, counts, kf_mp, kps, depth, th_depth, stereo, nlevels, kf_noterase, pts, obs_ptr, obs,
                     obs_erased, ref, nobs, root=-1, uright=None, out=None, device=0):
    """The same as keyframe_culling_device on host arrays; synchronous.  graph: a dict of numpy arrays as
    covis_graph(nkf, ccap) makes them (ord_kf and nord are read).  kf_mp, pts, obs_erased, ref (OBSERVATION_DTYPE)
    and nobs (int32) must be contiguous numpy arrays and are updated in place.  out: optional dict of verdict, nmps,
    nred, culled (ccap,) int32 whose contents stand where the call writes nothing.  Returns a dict of those and of
    nculled and ncand (ints)."""
    fn = "keyframe_culling"
    nkf, ccap = int(graph["ord_kf"].shape[0]), int(graph["ord_kf"].shape[1])
    ok = _inout(fn, "graph['ord_kf']", graph["ord_kf"], np.int32)
    on = _inout(fn, "graph['nord']", graph["nord"], np.int32, (nkf,))
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    cn, op = i32(counts), i32(obs_ptr)
    nmp = len(op) - 1
    km = _inout(fn, "kf_mp", kf_mp, np.int32)
    kp = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    ur, de = f32(uright), f32(depth)
    ne = np.ascontiguousarray(kf_noterase, np.uint8)
    p = _inout(fn, "pts", pts, MAP_POINT_DTYPE, (nmp,))
    ob = np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    er = _inout(fn, "obs_erased", obs_erased, np.uint8, (len(ob),))
    rf = _inout(fn, "ref", ref, OBSERVATION_DTYPE, (nmp,))
    no = _inout(fn, "nobs", nobs, np.int32, (nmp,))
    if not (km.ndim == 2 and km.shape[0] == nkf == len(cn) == len(ne) and kp.shape == km.shape and
            (ur is None or ur.shape == km.shape) and (de is None or de.shape == km.shape)):
        raise ValueError("keyframe_culling: array sizes disagree")
    out = dict(out or {})
    for k in ("verdict", "nmps", "nred", "culled"):
        out[k] = np.zeros(ccap, np.int32) if out.get(k) is None else _inout(fn, k, out[k], np.int32, (ccap,))
    g = CovisGraph()
    g.ord_kf, g.nord = ok.ctypes.data, on.ctypes.data
    ncul, ncand = C.c_int(0), C.c_int(0)
    _check("orbm_keyframe_culling",
           lib.orbm_keyframe_culling(device, C.byref(g), nkf, ccap, int(t), int(root), _vp(cn), _vp(km), km.shape[1],
                                     _vp(kp), _vp(ur), _vp(de), float(th_depth), int(bool(stereo)), int(nlevels),
                                     _vp(ne), _vp(p), _vp(op), _vp(ob), _vp(er), _vp(rf), _vp(no), nmp,
                                     _vp(out["verdict"]), _vp(out["nmps"]), _vp(out["nred"]), _vp(out["culled"]),
                                     C.addressof(ncul), C.addressof(ncand)))
    out["nculled"], out["ncand"] = ncul.value, ncand.value
    return out


def compact_observations(obs_ptr, obs, obs_erased, out=None, device=0):
    """The same as compact_observations_device on host arrays; synchronous.  out: optional dict of obs_ptr (nmp + 1,)
    int32 and obs (nobs,) OBSERVATION_DTYPE whose contents stand where the call writes nothing.  Returns a dict of
    obs_ptr, obs and status (an int)."""
    fn = "compact_observations"
    op = np.ascontiguousarray(obs_ptr, np.int32).reshape(-1)
    ob = np.ascontiguousarray(obs, OBSERVATION_DTYPE).reshape(-1)
    er = np.ascontiguousarray(obs_erased, np.uint8).reshape(-1)
    if len(er) != len(ob):
        raise ValueError("compact_observations: array sizes disagree")
    out = dict(out or {})
    out["obs_ptr"] = (np.zeros(len(op), np.int32) if out.get("obs_ptr") is None
                      else _inout(fn, "obs_ptr", out["obs_ptr"], np.int32, (len(op),)))
    out["obs"] = (np.zeros(len(ob), OBSERVATION_DTYPE) if out.get("obs") is None
                  else _inout(fn, "obs", out["obs"], OBSERVATION_DTYPE, (len(ob),)))
    st = C.c_int(0)
    _check("orbm_compact_observations",
           lib.orbm_compact_observations(device, _vp(op), _vp(ob), _vp(er), len(op) - 1, _vp(out["obs_ptr"]),
                                         _vp(out["obs"]), C.addressof(st)))
    out["status"] = st.value
    return out


TIE_FIRST, TIE_LAST = 0, 1


def best2_csr(q, t, cand_ptr, cand_idx, tie_mode=TIE_FIRST, device=0):
    """orbm_best2_csr on host arrays: per query (best target index, best distance, second distance)
    over its candidate list, in the list's order."""
    q = np.ascontiguousarray(q, np.uint8)
    nt = len(t)
    t = np.ascontiguousarray(t if nt else np.zeros((1, 32), np.uint8), np.uint8)
    ptr = np.ascontiguousarray(cand_ptr, np.int32)
    idx = np.ascontiguousarray(cand_idx if len(cand_idx) else np.zeros(1, np.int32), np.int32)
    nq = len(q)
    out = [np.zeros(max(nq, 1), np.int32) for _ in range(3)]
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _check("orbm_best2_csr", lib.orbm_best2_csr(device, _u8(q), nq, _u8(t), nt, i32(ptr), i32(idx), tie_mode,
                                                i32(out[0]), i32(out[1]), i32(out[2])))
    return tuple(o[:nq].copy() for o in out)


def stereo_band(kps_l, desc_l, kps_r, desc_r, rows, scale, min_d, max_d, device=0):
    """orbm_stereo_band on host arrays, the coarse stage of ComputeStereoMatches (src/Frame.cc:645-757):
    per left keypoint (best right index or -1, best distance or 100)."""
    kl = np.ascontiguousarray(kps_l, KEYPOINT_DTYPE)
    kr = np.ascontiguousarray(kps_r, KEYPOINT_DTYPE)
    nl, nr = len(kl), len(kr)
    dl = np.ascontiguousarray(desc_l if nl else np.zeros((1, 32), np.uint8), np.uint8)
    dr = np.ascontiguousarray(desc_r if nr else np.zeros((1, 32), np.uint8), np.uint8)
    sc = np.ascontiguousarray(scale, np.float32)
    bi, bd = np.zeros(max(nl, 1), np.int32), np.zeros(max(nl, 1), np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _check("orbm_stereo_band",
           lib.orbm_stereo_band(device, kl.ctypes.data, _u8(dl), nl, kr.ctypes.data, _u8(dr), nr, rows,
                                sc.ctypes.data_as(C.POINTER(C.c_float)), len(sc), min_d, max_d, i32(bi), i32(bd)))
    return bi[:nl].copy(), bd[:nl].copy()


def stereo_band_batch_device(kps, desc, counts, left, right, rows, scale, min_d, max_d, stream=None):
    """orbm_stereo_band_device over pairs (left[p], right[p]) of a device batch (kps int32 (F, cap, 7),
    desc uint8 (F, cap, 32), counts int32 (F,)).  Returns (best_idx, best_dist), int32 (npairs, cap)."""
    import torch
    cap = kps.shape[1]
    left = torch.as_tensor(left, dtype=torch.int32, device=kps.device).contiguous()
    right = torch.as_tensor(right, dtype=torch.int32, device=kps.device).contiguous()
    npairs = left.numel()
    bi = torch.empty((npairs, cap), dtype=torch.int32, device=kps.device)
    bd = torch.empty((npairs, cap), dtype=torch.int32, device=kps.device)
    sc = np.ascontiguousarray(scale, np.float32)
    _check("orbm_stereo_band_device",
           lib.orbm_stereo_band_device(_ptr(kps), _ptr(desc), _ptr(counts), cap, _ptr(left), _ptr(right), npairs, rows,
                                       sc.ctypes.data_as(C.POINTER(C.c_float)), len(sc), min_d, max_d, _ptr(bi),
                                       _ptr(bd), _stream(stream)))
    return bi, bd


def keypoints_from_device(kps_i32, counts):
    """(B, cap, 7) int32 torch tensor + counts -> list of structured numpy arrays."""
    arr = kps_i32.cpu().numpy()
    cnt = counts.cpu().numpy()
    return [arr[f, :cnt[f]].copy().view(KEYPOINT_DTYPE).reshape(-1) for f in range(arr.shape[0])]


class ORBmatcher:
    """ORBmatcher Hamming searches (include/ORBmatcher.h:37-102).

    SearchByBoW(KF, F) / SearchByBoW(KF1, KF2) / SearchForTriangulation take the
    per-side arrays the reference reads from its KeyFrame/Frame objects:
    (keypoints, descriptors, FeatureVector CSR (node, ptr, idx), MapPoint flags
    and, for triangulation, mvuRight)."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib.orbm_descriptor_distance(_u8(a), _u8(b))

    def SearchByBoW_KF_F(self, kf, f, device=0):
        """kf = (kps, desc, fv, has_mp), f = (kps, desc, fv).  Returns (nmatches, match_f)."""
        v1 = _host_view(kf[0], kf[1], kf[2], has_mp=kf[3])
        v2 = _host_view(f[0], f[1], f[2])
        return bow_search(BOW_KF_F, v1, v2, None, self.mfNNratio, self.mbCheckOrientation, device)

    def SearchByBoW_KF_KF(self, kf1, kf2, device=0):
        """kf = (kps, desc, fv, has_mp).  Returns (nmatches, match12)."""
        v1 = _host_view(kf1[0], kf1[1], kf1[2], has_mp=kf1[3])
        v2 = _host_view(kf2[0], kf2[1], kf2[2], has_mp=kf2[3])
        return bow_search(BOW_KF_KF, v1, v2, None, self.mfNNratio, self.mbCheckOrientation, device)

    def SearchForTriangulation(self, kf1, kf2, F12, ex, ey, scale2, sigma2_2, bOnlyStereo=False, device=0):
        """kf = (kps, desc, fv, has_mp, u_right).  Returns (nmatches, match12)."""
        v1 = _host_view(kf1[0], kf1[1], kf1[2], has_mp=kf1[3], u_right=kf1[4])
        v2 = _host_view(kf2[0], kf2[1], kf2[2], has_mp=kf2[3], u_right=kf2[4])
        tp = triang_params(F12, ex, ey, scale2, sigma2_2, bOnlyStereo)
        return bow_search(TRIANGULATION, v1, v2, tp, self.mfNNratio, self.mbCheckOrientation, device)

    def SearchByProjection(self, kps, desc, uright, claimed, grid, scale, pts, pdesc, th=1.0, device=0):
        """SearchByProjection(Frame& F, vector<MapPoint*>, th) (src/ORBmatcher.cc:45-129).
        kps = F.mvKeysUn, uright = F.mvuRight, claimed[i] = F.mvpMapPoints[i] && Observations() > 0,
        grid = (mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv), scale = mvScaleFactors,
        pts: PROJ_POINT_DTYPE per MapPoint, pdesc its descriptors.  Returns (nmatches, match[n])."""
        k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8)
        ur = np.ascontiguousarray(uright, np.float32)
        cl = np.ascontiguousarray(claimed, np.uint8)
        pp = np.ascontiguousarray(pts, PROJ_POINT_DTYPE)
        pd = np.ascontiguousarray(pdesc, np.uint8)
        n = len(k)
        out = np.full(max(n, 1), -1, np.int32)
        nm = C.c_int(0)
        prm = proj_params(grid, scale, th, self.mfNNratio)
        _check("orbm_search_by_projection",
               lib.orbm_search_by_projection(device, k.ctypes.data, _u8(d), ur.ctypes.data_as(C.POINTER(C.c_float)),
                                             _u8(cl), n, pp.ctypes.data, _u8(pd), len(pp), C.byref(prm),
                                             out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nm)))
        return nm.value, out[:n].copy()

    def project_search(self, mode, kps, desc, uright, claimed, pose, pts, pdesc, params, device=0):
        """The pose-projection searches (include/orbx.h ORBM_PROJ_* / ORBM_FUSE*) on host arrays.
        pose: Tcw (Scw for the Sim3 modes) 3x4 [+ LastFrame Tcw 3x4]; pts: MAP_POINT_DTYPE;
        params: PoseParams (check_ori is taken from this matcher).  Returns (n, match)."""
        k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8)
        ur = np.ascontiguousarray(uright, np.float32)
        cl = np.ascontiguousarray(claimed if claimed is not None else np.zeros(len(k), np.uint8), np.uint8)
        ps = np.zeros(24, np.float32)
        pz = np.asarray(pose, np.float32).ravel()
        ps[:len(pz)] = pz
        pp = np.ascontiguousarray(pts, MAP_POINT_DTYPE)
        pd = np.ascontiguousarray(pdesc, np.uint8)
        nout = len(k) if mode <= PROJ_SIM3 else len(pp)
        out = np.full(max(nout, 1), -1, np.int32)
        nm = C.c_int(0)
        prm = PoseParams.from_buffer_copy(params)
        prm.check_ori = int(self.mbCheckOrientation)
        f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        _check("orbm_project_search",
               lib.orbm_project_search(device, mode, k.ctypes.data, _u8(d), f32(ur), _u8(cl), len(k), f32(ps),
                                       pp.ctypes.data, _u8(pd), len(pp), C.byref(prm),
                                       out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nm)))
        return nm.value, out[:nout].copy()

    def project_search_batch_device(self, mode, kps, desc, uright, claimed, counts, pose, pts, pdesc, npts, params,
                                    match=None, nmatches=None, stream=None):
        """Batched device form of project_search: kps (B, cap, 7) int32, desc (B, cap, 32) uint8, uright
        (B, cap) float32, claimed (B, cap) uint8, counts (B,), pose (B, 24) float32, pts (B, pcap, 12)
        int32 view of MAP_POINT_DTYPE, pdesc (B, pcap, 32), npts (B,).  Returns (match, nmatches)."""
        import torch
        B, cap = kps.shape[0], kps.shape[1]
        pcap = pts.shape[1]
        nout = cap if mode <= PROJ_SIM3 else pcap
        if match is None:
            match = torch.empty((B, nout), dtype=torch.int32, device=kps.device)
        if nmatches is None:
            nmatches = torch.empty((B,), dtype=torch.int32, device=kps.device)
        prm = PoseParams.from_buffer_copy(params)
        prm.check_ori = int(self.mbCheckOrientation)
        _check("orbm_project_search_device",
               lib.orbm_project_search_device(mode, _ptr(kps), _ptr(desc), _ptr(uright), _ptr(claimed), _ptr(counts),
                                              B, cap, _ptr(pose), _ptr(pts), _ptr(pdesc), _ptr(npts), pcap,
                                              C.byref(prm), _ptr(match), _ptr(nmatches), _stream(stream)))
        return match, nmatches

    def SearchByProjectionLastFrame(self, cur, last_pts, last_pdesc, Tcw, Tlw, params, th, bMono, device=0):
        """SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (src/ORBmatcher.cc:1396-1538).
        cur = (mvKeysUn, mDescriptors, mvuRight, taken) with taken[i] = mvpMapPoints[i] && Observations() > 0."""
        prm = PoseParams.from_buffer_copy(params)
        prm.th, prm.mono = float(th), int(bool(bMono))
        pose = np.concatenate([np.asarray(Tcw, np.float32).reshape(-1)[:12], np.asarray(Tlw, np.float32).reshape(-1)[:12]])
        return self.project_search(PROJ_LAST_FRAME, cur[0], cur[1], cur[2], cur[3], pose, last_pts, last_pdesc, prm,
                                   device)

    def SearchByProjectionKeyFrame(self, cur, kf_pts, kf_pdesc, Tcw, params, th, ORBdist, device=0):
        """SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (:1540-1667).
        taken[i] = CurrentFrame.mvpMapPoints[i] != NULL."""
        prm = PoseParams.from_buffer_copy(params)
        prm.th, prm.orb_dist = float(th), int(ORBdist)
        return self.project_search(PROJ_KEYFRAME, cur[0], cur[1], cur[2], cur[3], Tcw, kf_pts, kf_pdesc, prm, device)

    def SearchByProjectionSim3(self, kf, pts, pdesc, Scw, params, th, device=0):
        """SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (:290-403); taken[i] = vpMatched[i]."""
        prm = PoseParams.from_buffer_copy(params)
        prm.th = float(int(th))
        return self.project_search(PROJ_SIM3, kf[0], kf[1], kf[2], kf[3], Scw, pts, pdesc, prm, device)

    def Fuse(self, kf, pts, pdesc, Tcw, params, th=3.0, device=0):
        """Fuse(KeyFrame*, vpMapPoints, th) (:893-1043): per MapPoint the KeyFrame feature it fuses into."""
        prm = PoseParams.from_buffer_copy(params)
        prm.th = float(th)
        return self.project_search(FUSE, kf[0], kf[1], kf[2], None, Tcw, pts, pdesc, prm, device)

    def FuseSim3(self, kf, pts, pdesc, Scw, params, th, device=0):
        """Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:1045-1168)."""
        prm = PoseParams.from_buffer_copy(params)
        prm.th = float(th)
        return self.project_search(FUSE_SIM3, kf[0], kf[1], kf[2], None, Scw, pts, pdesc, prm, device)

    def search_by_sim3(self, kf1, kf2, already1, already2, T1w, T2w, s12, R12, t12, params, device=0):
        """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1170-1394) on host arrays.
        kf = (mvKeysUn, mDescriptors, mps, mpdesc): mps is MAP_POINT_DTYPE per feature (GetMapPointMatches():
        x, y, z, max_dist, min_dist, flags bit 0 = pMP && !isBad()), mpdesc each MapPoint's GetDescriptor().
        already1[i1] = vpMatches12[i1] != NULL, already2 = vbAlreadyMatched2 (:1200-1210); params: PoseParams
        with th set.  Returns (nFound, match12, vnMatch1, vnMatch2): vpMatches12[i1] = vpMapPoints2[match12[i1]]
        where match12[i1] >= 0."""
        f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        side = []
        for kf, al in ((kf1, already1), (kf2, already2)):
            k = np.ascontiguousarray(kf[0], KEYPOINT_DTYPE)
            side.append((k, np.ascontiguousarray(kf[1], np.uint8), np.ascontiguousarray(kf[2], MAP_POINT_DTYPE),
                         np.ascontiguousarray(kf[3], np.uint8),
                         np.ascontiguousarray(al if al is not None else np.zeros(len(k), np.uint8), np.uint8)))
        T = [np.ascontiguousarray(np.asarray(t, np.float32).reshape(-1)[:12]) for t in (T1w, T2w)]
        R = np.ascontiguousarray(np.asarray(R12, np.float32).reshape(-1)[:9])
        t = np.ascontiguousarray(np.asarray(t12, np.float32).reshape(-1)[:3])
        n1, n2 = len(side[0][0]), len(side[1][0])
        m12, m1 = np.full(max(n1, 1), -1, np.int32), np.full(max(n1, 1), -1, np.int32)
        m2 = np.full(max(n2, 1), -1, np.int32)
        nf = C.c_int(0)
        prm = PoseParams.from_buffer_copy(params)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        args = []
        for (k, d, mp, md, al), Tw in zip(side, T):
            args += [k.ctypes.data, _u8(d), mp.ctypes.data, _u8(md), _u8(al), len(k), f32(Tw)]
        _check("orbm_search_by_sim3",
               lib.orbm_search_by_sim3(device, *args, float(s12), f32(R), f32(t), C.byref(prm), i32(m12), C.byref(nf),
                                       i32(m1), i32(m2)))
        return nf.value, m12[:n1].copy(), m1[:n1].copy(), m2[:n2].copy()

    def search_by_sim3_batch_device(self, kps, desc, mps, mpdesc, counts, pose, pair_a, pair_b, sim3, already1,
                                    already2, params, match12=None, nfound=None, match1=None, match2=None,
                                    stream=None):
        """Batched device form of search_by_sim3 over KeyFrame pairs: kps (B, cap, 7) int32, desc (B, cap, 32)
        uint8, mps (B, cap, 12) int32 view of MAP_POINT_DTYPE, mpdesc (B, cap, 32), counts (B,), pose (B, 12)
        float32 Tcw, pair_a / pair_b (npairs,) int32, sim3 (npairs, 13) float32 = s12, R12, t12, already1 /
        already2 (npairs, cap) uint8.  match1 / match2: tensors to receive vnMatch1 / vnMatch2, or None.
        Returns (match12, nfound)."""
        import torch
        B, cap = kps.shape[0], kps.shape[1]
        npairs = pair_a.shape[0]
        if match12 is None:
            match12 = torch.empty((npairs, cap), dtype=torch.int32, device=kps.device)
        if nfound is None:
            nfound = torch.empty((npairs,), dtype=torch.int32, device=kps.device)
        prm = PoseParams.from_buffer_copy(params)
        _check("orbm_search_by_sim3_device",
               lib.orbm_search_by_sim3_device(_ptr(kps), _ptr(desc), _ptr(mps), _ptr(mpdesc), _ptr(counts), B, cap,
                                              _ptr(pose), _ptr(pair_a), _ptr(pair_b), _ptr(sim3), _ptr(already1),
                                              _ptr(already2), npairs, C.byref(prm), _ptr(match12), _ptr(nfound),
                                              _ptr(match1), _ptr(match2), _stream(stream)))
        return match12, nfound

    def search_for_initialization_batch(self, kps, desc, counts, pair_a, pair_b, rows, cols, window=100,
                                        matches12=None, nmatches=None, stream=None, bounds=None, prev_matched=None):
        """SearchForInitialization over device frame pairs; returns (matches12, nmatches) tensors.
        bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY) (default 0..cols x 0..rows); prev_matched: float32
        (npairs, cap, 2) cuda tensor holding each pair's vbPrevMatched, updated in place (default: F1's
        keypoints, not written)."""
        import torch
        npairs = pair_a.shape[0]
        cap = kps.shape[1]
        if matches12 is None:
            matches12 = torch.empty((npairs, cap), dtype=torch.int32, device=kps.device)
        if nmatches is None:
            nmatches = torch.empty((npairs,), dtype=torch.int32, device=kps.device)
        ori = 1 if self.mbCheckOrientation else 0
        if bounds is None and prev_matched is None:
            rc = lib.orbm_search_init_batch_device(_ptr(kps), _ptr(desc), _ptr(counts), kps.shape[0], cap,
                                                   _ptr(pair_a), _ptr(pair_b), npairs, rows, cols, window,
                                                   self.mfNNratio, ori, _ptr(matches12), _ptr(nmatches),
                                                   _stream(stream))
            _check("orbm_search_init_batch_device", rc)
            return matches12, nmatches
        g = frame_grid(bounds if bounds is not None else (0.0, cols, 0.0, rows))
        if prev_matched is not None:
            assert prev_matched.dtype == torch.float32 and tuple(prev_matched.shape) == (npairs, cap, 2)
            assert prev_matched.is_contiguous()
        rc = lib.orbm_search_for_initialization_device(_ptr(kps), _ptr(desc), _ptr(counts), kps.shape[0], cap,
                                                       _ptr(pair_a), _ptr(pair_b), npairs, C.byref(g), window,
                                                       self.mfNNratio, ori, _ptr(prev_matched), _ptr(matches12),
                                                       _ptr(nmatches), _stream(stream))
        _check("orbm_search_for_initialization_device", rc)
        return matches12, nmatches

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=100, bounds=None, device=0):
        """ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
        (src/ORBmatcher.cc:417-588) on host arrays: F = (mvKeysUn, mDescriptors[, (cols, rows)]);
        bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY) (default 0..cols x 0..rows from F2).  vbPrevMatched is
        a float32 (n1, 2) numpy array, updated in place like the reference's.  Returns (nmatches, vnMatches12)."""
        k1 = np.ascontiguousarray(F1[0], KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(F2[0], KEYPOINT_DTYPE)
        n1, n2 = len(k1), len(k2)
        d1 = np.ascontiguousarray(F1[1] if n1 else np.zeros((1, 32), np.uint8), np.uint8)
        d2 = np.ascontiguousarray(F2[1] if n2 else np.zeros((1, 32), np.uint8), np.uint8)
        if bounds is None:
            cols, rows = F2[2]
            bounds = (0.0, cols, 0.0, rows)
        assert isinstance(vbPrevMatched, np.ndarray) and vbPrevMatched.dtype == np.float32
        assert vbPrevMatched.shape == (n1, 2) and vbPrevMatched.flags.c_contiguous
        g = frame_grid(bounds)
        m12 = np.full(max(n1, 1), -1, np.int32)
        nm = C.c_int(0)
        pv = vbPrevMatched if n1 else np.zeros((1, 2), np.float32)
        _check("orbm_search_for_initialization",
               lib.orbm_search_for_initialization(device, k1.ctypes.data, _u8(d1), n1, k2.ctypes.data, _u8(d2), n2,
                                                  C.byref(g), pv.ctypes.data_as(C.POINTER(C.c_float)), windowSize,
                                                  self.mfNNratio, 1 if self.mbCheckOrientation else 0,
                                                  m12.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nm)))
        return nm.value, m12[:n1].copy()


def _host_view(kps, desc, fv, has_mp=None, u_right=None):
    keep = [np.ascontiguousarray(kps, KEYPOINT_DTYPE), np.ascontiguousarray(desc, np.uint8)]
    node, ptr, idx = (np.ascontiguousarray(a, np.int32) for a in fv)
    keep += [node, ptr, idx]
    mp = ur = None
    if has_mp is not None:
        mp = np.ascontiguousarray(has_mp, np.uint8)
        keep.append(mp)
    if u_right is not None:
        ur = np.ascontiguousarray(u_right, np.float32)
        keep.append(ur)
    v = BowView(keep[0].ctypes.data, keep[1].ctypes.data, mp.ctypes.data if mp is not None else None,
                ur.ctypes.data if ur is not None else None, node.ctypes.data, ptr.ctypes.data, idx.ctypes.data,
                len(keep[0]), len(node))
    v._keep = keep
    return v


def triang_params(F12, ex, ey, scale2, sigma2_2, only_stereo=False):
    tp = TriangParams()
    tp.F12[:] = [float(x) for x in np.asarray(F12, np.float32).reshape(9)]
    tp.ex, tp.ey = ex, ey
    s2 = np.zeros(16, np.float32)
    g2 = np.zeros(16, np.float32)
    s2[:len(scale2)] = scale2
    g2[:len(sigma2_2)] = sigma2_2
    tp.scale2[:] = [float(x) for x in s2]
    tp.sigma2_2[:] = [float(x) for x in g2]
    tp.only_stereo = 1 if only_stereo else 0
    return tp


def bow_search(mode, view1, view2, tp=None, nnratio=0.6, check_ori=True, device=0):
    """Host path of the vocabulary-node searches; view1/view2 from _host_view.  Returns (nmatches, match)."""
    nout = view2.n if mode == BOW_KF_F else view1.n
    out = np.full(max(nout, 1), -1, np.int32)
    nm = C.c_int(0)
    _check("orbm_bow_search", lib.orbm_bow_search(device, mode, C.byref(view1), C.byref(view2),
                                                  C.byref(tp) if tp is not None else None, nnratio,
                                                  1 if check_ori else 0, out.ctypes.data_as(C.POINTER(C.c_int)),
                                                  C.byref(nm)))
    return nm.value, out[:nout].copy()


def allpairs(q, t, mode=TOP2, stream=None):
    """Config-5 brute force: q (nq,32), t (nt,32) uint8 cuda tensors."""
    import torch
    nq, nt = q.shape[0], t.shape[0]
    if mode == TOP2:
        bi = torch.empty(nq, dtype=torch.int32, device=q.device)
        b1 = torch.empty_like(bi)
        b2 = torch.empty_like(bi)
        _check("orbm_allpairs_device", lib.orbm_allpairs_device(_ptr(q), nq, _ptr(t), nt, TOP2, _ptr(bi), _ptr(b1),
                                                                _ptr(b2), None, _stream(stream)))
        return bi, b1, b2
    full = torch.empty((nq, nt), dtype=torch.int16, device=q.device)
    _check("orbm_allpairs_device", lib.orbm_allpairs_device(_ptr(q), nq, _ptr(t), nt, FULL_U16, None, None, None,
                                                            _ptr(full), _stream(stream)))
    return full


class ORBVocabulary:
    """DBoW2 TemplatedVocabulary<FORB> on the device (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h):
    loadFromTextFile, transform(features, BowVector, FeatureVector, levelsup)."""

    def __init__(self, handle):
        self._h = handle
        k, L, sc, wt, nn, nw = (C.c_int() for _ in range(6))
        _check("orbv_info", lib.orbv_info(self._h, C.byref(k), C.byref(L), C.byref(sc), C.byref(wt), C.byref(nn),
                                          C.byref(nw)))
        self.k, self.L, self.scoring, self.weighting = k.value, L.value, sc.value, wt.value
        self.nnodes, self.nwords = nn.value, nw.value

    @staticmethod
    def loadFromTextFile(path, device=0):
        h = C.c_void_p()
        _check("orbv_load_text", lib.orbv_load_text(str(path).encode(), device, C.byref(h)))
        return ORBVocabulary(h)

    @staticmethod
    def from_arrays(k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0, device=0):
        par = np.ascontiguousarray(parent, np.int32)
        leaf = np.ascontiguousarray(is_leaf, np.uint8)
        d = np.ascontiguousarray(desc, np.uint8)
        w = np.ascontiguousarray(weight, np.float64)
        h = C.c_void_p()
        _check("orbv_create", lib.orbv_create(k, L, scoring, weighting, len(par),
                                              par.ctypes.data_as(C.POINTER(C.c_int)), _u8(leaf), _u8(d),
                                              w.ctypes.data_as(C.POINTER(C.c_double)), device, C.byref(h)))
        return ORBVocabulary(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.orbv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, desc, levelsup=4):
        """Returns (bow_word, bow_weight, (fv_node, fv_ptr, fv_idx))."""
        d = np.ascontiguousarray(desc if desc is not None else np.zeros((0, 32), np.uint8), np.uint8)
        n = len(d)
        bw = np.zeros(n + 1, np.int32)
        bv = np.zeros(n + 1, np.float64)
        fn = np.zeros(n + 1, np.int32)
        fp = np.zeros(n + 2, np.int32)
        fi = np.zeros(n + 1, np.int32)
        nb, nn = C.c_int(0), C.c_int(0)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _check("orbv_transform", lib.orbv_transform(self._h, _u8(d), n, levelsup, i32(bw),
                                                    bv.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nb), i32(fn),
                                                    i32(fp), i32(fi), C.byref(nn)))
        k, m = nb.value, nn.value
        return bw[:k].copy(), bv[:k].copy(), (fn[:m].copy(), fp[:m + 1].copy(), fi[:fp[m]].copy())

    def transform_batch_device(self, desc, counts, levelsup=4, stream=None):
        """desc: (B, cap, 32) uint8 cuda tensor, counts (B,) int32.  Returns device tensors
        (bow_word, bow_weight, bow_n, fv_node, fv_ptr, fv_idx, fv_nnodes)."""
        import torch
        B, cap = desc.shape[0], desc.shape[1]
        dev = desc.device
        bw = torch.empty((B, cap), dtype=torch.int32, device=dev)
        bv = torch.empty((B, cap), dtype=torch.float64, device=dev)
        bn = torch.empty((B,), dtype=torch.int32, device=dev)
        fn = torch.empty((B, cap), dtype=torch.int32, device=dev)
        fp = torch.empty((B, cap + 1), dtype=torch.int32, device=dev)
        fi = torch.empty((B, cap), dtype=torch.int32, device=dev)
        fnn = torch.empty((B,), dtype=torch.int32, device=dev)
        _check("orbv_transform_batch_device",
               lib.orbv_transform_batch_device(self._h, _ptr(desc), _ptr(counts), B, cap, levelsup, _ptr(bw),
                                               _ptr(bv), _ptr(bn), _ptr(fn), _ptr(fp), _ptr(fi), _ptr(fnn),
                                               _stream(stream)))
        return bw, bv, bn, fn, fp, fi, fnn

    @staticmethod
    def score(b1, b2, scoring=0):
        """TemplatedVocabulary::score(v1, v2) of two BowVectors, each a (words, weights) pair (L1_NORM only)."""
        w1, v1 = _bow(b1)
        w2, v2 = _bow(b2)
        out = C.c_double(0.0)
        _check("orbv_score", lib.orbv_score(scoring, _i32p(w1), _f64p(v1), len(w1), _i32p(w2), _f64p(v2), len(w2),
                                            C.byref(out)))
        return out.value


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _bow(b):
    w = np.ascontiguousarray(b[0], np.int32).reshape(-1)
    v = np.ascontiguousarray(b[1], np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("a BowVector's words and weights differ in length")
    return w, v


class KeyFrameDatabase:
    """KeyFrameDatabase (src/KeyFrameDatabase.cc) on the vocabulary's device.  Keyframes are slots: add() returns
    0, 1, ... in add order and every query speaks of keyframes by slot.  BowVectors are (words, weights) pairs as
    ORBVocabulary.transform returns them."""

    def __init__(self, voc, reserve_keyframes=0, reserve_words=0):
        self._h = None
        h = C.c_void_p()
        _check("orbv_db_create", lib.orbv_db_create(voc._h, reserve_keyframes, reserve_words, C.byref(h)))
        self._h = h
        self._voc = voc   # the database reads the vocabulary's device

    def close(self):
        if getattr(self, "_h", None):
            lib.orbv_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, bow):
        w, v = _bow(bow)
        slot = C.c_int(-1)
        _check("orbv_db_add", lib.orbv_db_add(self._h, _i32p(w), _f64p(v), len(w), C.byref(slot)))
        return slot.value

    def add_batch_device(self, bow_word, bow_weight, bow_n, nframes=None, stream=None):
        """Frames 0..nframes-1 of a transform_batch_device result (device tensors); returns their slots."""
        B = bow_word.shape[0] if nframes is None else int(nframes)
        slots = np.zeros(max(B, 1), np.int32)
        _check("orbv_db_add_batch_device",
               lib.orbv_db_add_batch_device(self._h, _ptr(bow_word), _ptr(bow_weight), _ptr(bow_n), B,
                                            bow_word.shape[1], _i32p(slots), _stream(stream)))
        return slots[:B].copy()

    def erase(self, slot):
        _check("orbv_db_erase", lib.orbv_db_erase(self._h, int(slot)))

    def clear(self):
        _check("orbv_db_clear", lib.orbv_db_clear(self._h))

    def info(self):
        """(nslots, nlive, words_stored)"""
        ns, nl, ws = C.c_int(0), C.c_int(0), C.c_size_t(0)
        _check("orbv_db_info", lib.orbv_db_info(self._h, C.byref(ns), C.byref(nl), C.byref(ws)))
        return ns.value, nl.value, ws.value

    def scores(self, bow, slots):
        """score(bow, slot) as float64 per listed slot (LoopClosing::DetectLoop's reference-score loop)."""
        w, v = _bow(bow)
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros(len(sl), np.float64)
        _check("orbv_db_scores", lib.orbv_db_scores(self._h, _i32p(w), _f64p(v), len(w), _i32p(sl), len(sl),
                                                    _f64p(out)))
        return out

    def _covis(self, covis, ns):
        if covis is None:
            return None
        c = np.ascontiguousarray(covis, np.int32)
        if c.shape != (ns, 10):
            raise ValueError("covis must be (nslots, 10)")
        return c

    def _detect(self, loop, bow, connected, covis, min_score, cap, want_state=True):
        w, v = _bow(bow)
        ns = self.info()[0]
        cv = self._covis(covis, ns)
        cn = None
        if connected is not None:
            cn = np.ascontiguousarray(connected, np.uint8).reshape(-1)
            if len(cn) != ns:
                raise ValueError("connected must have nslots entries")
        cap = ns if cap is None else int(cap)
        cand = np.zeros(max(cap, 1), np.int32)
        words = np.zeros(max(ns, 1), np.int32)
        sc = np.zeros(max(ns, 1), np.float32)
        nc = C.c_int(0)
        f32 = sc.ctypes.data_as(C.POINTER(C.c_float)) if want_state else None
        wp = _i32p(words) if want_state else None
        cvp = _i32p(cv) if cv is not None else None
        if loop:
            rc = lib.orbv_db_detect_loop(self._h, _i32p(w), _f64p(v), len(w), _u8(cn) if cn is not None else None,
                                         cvp, float(min_score), _i32p(cand), cap, C.byref(nc), wp, f32)
        else:
            rc = lib.orbv_db_detect_reloc(self._h, _i32p(w), _f64p(v), len(w), cvp, _i32p(cand), cap, C.byref(nc),
                                          wp, f32)
        if rc == ENOSPC:
            err = OrbxError("orbv_db_detect_loop" if loop else "orbv_db_detect_reloc", rc)
            err.ncand = nc.value
            raise err
        _check("orbv_db_detect_loop" if loop else "orbv_db_detect_reloc", rc)
        if not want_state:
            return cand[:nc.value].copy(), None, None
        return cand[:nc.value].copy(), words[:ns].copy(), sc[:ns].copy()

    def DetectLoopCandidates(self, bow, minScore, connected=None, covis=None, cap=None, want_state=True):
        """Returns (vpLoopCandidates as slots, mnLoopWords per slot, mLoopScore per slot).  cap: room for the
        candidates (default: every slot).  want_state=False skips the two per-slot arrays (None, None): the
        form for a caller that does not know the slot count, e.g. while another thread adds keyframes."""
        return self._detect(True, bow, connected, covis, minScore, cap, want_state)

    def DetectRelocalizationCandidates(self, bow, covis=None, cap=None, want_state=True):
        """Returns (vpRelocCandidates as slots, mnRelocWords per slot, mRelocScore per slot)."""
        return self._detect(False, bow, None, covis, 0.0, cap, want_state)

    def _detect_device(self, loop, q_word, q_weight, q_n, connected, covis, min_score, stream):
        import torch
        ns = self.info()[0]
        dev = q_word.device
        cand = torch.empty((max(ns, 1),), dtype=torch.int32, device=dev)
        nc = torch.empty((1,), dtype=torch.int32, device=dev)
        words = torch.empty((max(ns, 1),), dtype=torch.int32, device=dev)
        sc = torch.empty((max(ns, 1),), dtype=torch.float32, device=dev)
        q_cap = q_word.shape[-1]
        if loop:
            _check("orbv_db_detect_loop_device",
                   lib.orbv_db_detect_loop_device(self._h, _ptr(q_word), _ptr(q_weight), _ptr(q_n), q_cap,
                                                  _ptr(connected), _ptr(covis), float(min_score), ns, _ptr(cand),
                                                  _ptr(nc), _ptr(words), _ptr(sc), _stream(stream)))
        else:
            _check("orbv_db_detect_reloc_device",
                   lib.orbv_db_detect_reloc_device(self._h, _ptr(q_word), _ptr(q_weight), _ptr(q_n), q_cap,
                                                   _ptr(covis), ns, _ptr(cand), _ptr(nc), _ptr(words), _ptr(sc),
                                                   _stream(stream)))
        return cand, nc, words[:ns], sc[:ns]

    def DetectLoopCandidates_device(self, q_word, q_weight, q_n, minScore, connected=None, covis=None, stream=None):
        """The query is one frame of a transform batch: q_word / q_weight its (cap,) rows, q_n a 1-element int32
        tensor; connected (nslots,) uint8 and covis (nslots, 10) int32 device tensors or None.  Returns device
        tensors (cand[nslots], ncand[1], words[nslots], scores[nslots]); asynchronous on the stream."""
        return self._detect_device(True, q_word, q_weight, q_n, connected, covis, minScore, stream)

    def DetectRelocalizationCandidates_device(self, q_word, q_weight, q_n, covis=None, stream=None):
        return self._detect_device(False, q_word, q_weight, q_n, None, covis, 0.0, stream)


class BowBatch:
    """Device-resident batch of vocabulary-node searches (orbm_bow_search_device).

    sides1 / sides2: lists (one entry per pair) of dicts with keys kps, desc, fv=(node, ptr,
    idx) and optionally has_mp, u_right -- host numpy arrays, uploaded once; or `kps`/`desc`
    may already be cuda tensors (e.g. a slice of an extract batch), used in place.
    tps: list of TriangParams for TRIANGULATION."""

    def __init__(self, mode, sides1, sides2, tps=None, device=0):
        import torch
        self.mode = mode
        self.dev = torch.device("cuda", device)
        self._keep = []
        v1 = [self._view(s) for s in sides1]
        v2 = [self._view(s) for s in sides2]
        self.npairs = len(v1)
        self.max_nodes1 = max([v.fv_nnodes for v in v1] + [0])
        n_out = [(b.n if mode == BOW_KF_F else a.n) for a, b in zip(v1, v2)]
        self.stride = max(n_out + [1])
        self.d_v1 = self._upload_structs(v1, BowView)
        self.d_v2 = self._upload_structs(v2, BowView)
        self.d_tp = self._upload_structs(tps, TriangParams) if tps else None
        self.match = torch.empty((self.npairs, self.stride), dtype=torch.int32, device=self.dev)
        self.nmatches = torch.empty((self.npairs,), dtype=torch.int32, device=self.dev)

    def _t(self, a, dtype):
        import torch
        if isinstance(a, torch.Tensor):
            t = a.contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self._keep.append(t)
        return t.data_ptr()

    def _view(self, s):
        import torch
        kps = s["kps"]
        n = kps.shape[0] if isinstance(kps, torch.Tensor) else len(kps)
        if not isinstance(kps, torch.Tensor):
            kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).view(np.int32).reshape(-1, 7)
        node, ptr, idx = (np.ascontiguousarray(a, np.int32) for a in s["fv"])
        # has_mp / u_right may be cuda tensors too (a row of the array triangulate_device marks): used in place
        host = lambda a, dt: a if isinstance(a, torch.Tensor) else np.ascontiguousarray(a, dt)
        return BowView(self._t(kps, None), self._t(s["desc"], None),
                       self._t(host(s["has_mp"], np.uint8), None) if s.get("has_mp") is not None
                       else None,
                       self._t(host(s["u_right"], np.float32), None) if s.get("u_right") is not None
                       else None,
                       self._t(node, None), self._t(ptr, None), self._t(idx if len(idx) else np.zeros(1, np.int32),
                                                                         None),
                       n, len(node))

    def _upload_structs(self, items, cls):
        import torch
        raw = b"".join(bytes(memoryview(x)) for x in items)
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.dev)
        self._keep.append(t)
        return t

    def run(self, nnratio=0.6, check_ori=True, stream=None):
        rc = lib.orbm_bow_search_device(self.mode, _ptr(self.d_v1), _ptr(self.d_v2),
                                        _ptr(self.d_tp) if self.d_tp is not None else None, self.npairs,
                                        self.max_nodes1, nnratio, 1 if check_ori else 0, _ptr(self.match),
                                        self.stride, _ptr(self.nmatches), _stream(stream))
        _check("orbm_bow_search_device", rc)
        return self.match, self.nmatches


def allpairs_host(q, t, mode=TOP2, device=0):
    """orbm_allpairs on host arrays: TOP2 -> (best_idx, best, second); FULL_U16 -> (nq, nt) uint16."""
    q = np.ascontiguousarray(q, np.uint8)
    nq, nt = len(q), len(t)
    t = np.ascontiguousarray(t if nt else np.zeros((1, 32), np.uint8), np.uint8)
    if mode == TOP2:
        out = [np.zeros(max(nq, 1), np.int32) for _ in range(3)]
        _check("orbm_allpairs", lib.orbm_allpairs(device, _u8(q), nq, _u8(t), nt, TOP2, out[0].ctypes.data,
                                                  out[1].ctypes.data, out[2].ctypes.data, None))
        return tuple(o[:nq].copy() for o in out)
    full = np.zeros((max(nq, 1), max(nt, 1)), np.uint16)
    _check("orbm_allpairs", lib.orbm_allpairs(device, _u8(q), nq, _u8(t), nt, FULL_U16, None, None, None,
                                              full.ctypes.data))
    return full[:nq, :nt].copy()
