"""ctypes binding of the C ABI in include/orbx.h (liborbx.so).  Plumbing only: tests and bench.py
drive the library through this module; the drop-in for ORB_SLAM itself is the C++ shim in
orb_slam_amd/cpp/ (ORBextractor.h / ORBmatcher.h) which calls the same C ABI.

There is no CPU fallback anywhere in this module: if liborbx.so is missing or no GPU is usable,
calls raise OrbxError."""
import ctypes
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBX_LIB") or os.path.join(_HERE, "liborbx.so")      # ORBX_LIB: a differently built library (tuning sweeps)

ORBX_OK, ORBX_EMPTY = 0, 1
ORBX_ERR_ARG, ORBX_ERR_DEVICE, ORBX_ERR_CAPACITY, ORBX_ERR_GEOMETRY = -1, -2, -3, -4
HARRIS_SCORE, FAST_SCORE = 0, 1
BLUR_X86_SSE2, BLUR_HALF_UP = 0, 1
DBG_PLANE, DBG_BLUR, DBG_NMS, DBG_LEVEL_KPS, DBG_BANDS = 0, 1, 2, 3, 4
(ST_PYRAMID, ST_FAST_CELLS, ST_QUOTA, ST_CELL_SELECT, ST_LEVEL_SELECT, ST_BLUR, ST_DESCRIBE) = range(7)

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

# every symbol include/orbx.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "orbx_default_params", "orbx_create", "orbx_destroy", "orbx_get_levels", "orbx_get_scale_factor",
    "orbx_max_keypoints", "orbx_last_error", "orbx_build_id", "orbx_extract", "orbx_extract_batch_device", "orbx_extract_batch_device_phases", "orbx_extract_batch",
    "orbx_to_gray_device", "orbx_extract_color", "orbx_extract_batch_device_color", "orbx_extract_batch_color",
    "orbm_hamming256", "orbm_match_top2", "orbm_match_top2_device", "orbm_match_top2_batch_device", "orbm_match_top2_masked", "orbm_match_top2_masked_device",
    "orbm_count_accepted", "orbm_match_top2_segments", "orbm_match_top2_segments_device", "orbm_distinctive", "orbm_distinctive_device",
    "orbx_device_alloc", "orbx_device_free", "orbx_device_upload", "orbx_device_download",
    "orbx_stream_create", "orbx_stream_create_priority", "orbx_stream_destroy", "orbx_stream_synchronize", "orbx_event_create", "orbx_event_destroy", "orbx_event_record",
    "orbx_stream_wait_event", "orbx_device_copy_async", "orbx_host_alloc", "orbx_host_free", "orbx_device_upload_async", "orbx_device_download_async", "orbx_debug_set_stop_after", "orbx_debug_set_blur_on_demand", "orbx_debug_level_size", "orbx_debug_resize_form", "orbx_debug_fetch",
    "orbx_debug_launch_variant", "orbx_debug_variant_count", "orbx_debug_variant_name", "orbx_debug_plan",
    "orbx_debug_eval_math", "orbx_debug_eval_compass", "orbx_debug_eval_score", "orbx_debug_eval_blur_window", "orbx_debug_stage_timing", "orbx_debug_stage_time", "orbx_debug_nth_element", "orbx_debug_geometry",
    "orbm_debug_set_match_path",
    "orbm_debug_get_match_path",
]
# include/orbf.h (Frame-side steps: undistortion, search grid, window query)
EXPORTS_F = [
    "orbf_image_bounds", "orbf_undistort_grid", "orbf_undistort_grid_batch_device", "orbf_features_in_area",
    "orbf_features_in_area_device",
]
# include/orbs.h (greedy grid-window searches)
EXPORTS_S = ["orbs_lds_bytes", "orbs_debug_set_buckets", "orbs_debug_set_wide_max", "orbs_three_maxima", "orbs_window_search_batch_device", "orbs_list_search_batch_device",
             "orbs_bow_ranges_batch_device", "orbs_triangulation_search_batch_device", "orbs_epipolar_bound", "orbs_agreement_batch_device",
             "orbs_bow_rows_search_batch_device", "orbs_bow_rows_search", "orbs_tri_rows_search_batch_device", "orbs_tri_rows_search"]
PHASE_PYRAMID, PHASE_DETECT, PHASE_DESCRIBE, PHASE_ALL = 1, 2, 4, 7
RULE_MAPPOINTS, RULE_WINDOW, RULE_BEST, RULE_INIT, RULE_BOW, RULE_FREE, RULE_TRIANGULATION = 0, 1, 2, 3, 4, 5, 6
TH_HIGH, TH_LOW = 100, 50
# include/orbv.h (bag-of-words transform)
EXPORTS_V = [
    "orbv_create", "orbv_load_text", "orbv_destroy", "orbv_info", "orbv_descend", "orbv_descend_device",
    "orbv_transform", "orbv_transform_batch_device", "orbv_score",
]
# include/orbd.h (key-frame database)
EXPORTS_D = ["orbd_create", "orbd_destroy", "orbd_size", "orbd_add", "orbd_add_batch_device", "orbd_erase", "orbd_clear",
             "orbd_query_batch_device", "orbd_query"]
EXPORTS_P = ["orbp_create", "orbp_destroy", "orbp_capacity", "orbp_size", "orbp_clear", "orbp_put", "orbp_put_device", "orbp_erase", "orbp_get",
             "orbp_project_batch_device", "orbp_track_batch_device", "orbp_track", "orbp_project_source_batch_device",
             "orbp_track_source_batch_device", "orbp_track_source", "orbp_refresh_batch_device", "orbp_refresh", "orbp_fuse_batch_device",
             "orbp_fuse", "orbp_view_from_sim3", "orbp_loop_project_batch_device", "orbp_loop_search_batch_device", "orbp_loop_search",
             "orbp_sim3_from_pair", "orbp_sim3_search_batch_device", "orbp_sim3_search", "orbp_local_votes_batch_device", "orbp_local_votes",
             "orbp_local_points_batch_device", "orbp_local_points", "orbp_rows_purge_device", "orbp_cull_batch_device", "orbp_cull"]
LOCAL_MAX_PROBLEMS, LOCAL_MAX_ROWS = 64, 65535      # ORBP_LOCAL_MAX_PROBLEMS, ORBP_LOCAL_MAX_ROWS
CULL_MAX_CANDIDATES = 4096                          # ORBP_CULL_MAX_CANDIDATES
# include/orbt.h (triangulation of new map points)
EXPORTS_T = ["orbt_triangulate_batch_device", "orbt_triangulate", "orbt_new_points_rows_device", "orbt_new_points_rows"]
(T_NONE, T_ACCEPTED, T_PARALLAX, T_W_ZERO, T_DEPTH1, T_DEPTH2, T_REPROJ1, T_REPROJ2, T_ZERO_DIST, T_SCALE, T_SKIP_INDEX, T_SKIP_OCTAVE) = range(12)
# include/orbi.h (monocular initialisation)
EXPORTS_I = ["orbi_normalize", "orbi_pose_from_rt", "orbi_models_batch_device", "orbi_models", "orbi_check_rt_batch_device", "orbi_check_rt"]
INIT_MAX_PROBLEMS, INIT_MAX_MATCHES, INIT_MAX_ITERS, INIT_MAX_HYP = 32, 16384, 1024, 8      # ORBI_MAX_*
(RT_NONE, RT_GOOD, RT_COUNTED, RT_NONFINITE, RT_DEPTH1, RT_DEPTH2, RT_REPROJ1, RT_REPROJ2, RT_SKIP_INDEX) = range(9)
# include/orbe.h (the EPnP RANSAC of the relocalisation)
EXPORTS_E = ["orbe_ransac_parameters", "orbe_hypotheses_batch_device", "orbe_hypotheses", "orbe_refine_batch_device", "orbe_refine",
             "orbe_refit_batch_device", "orbe_refit", "orbe_select_batch_device", "orbe_select", "orbe_iterate", "orbe_iterate_batch"]
# include/orbh.h (the Sim3 RANSAC of loop closing)
EXPORTS_H = ["orbh_ransac_parameters", "orbh_max_errors", "orbh_hypotheses_batch_device", "orbh_hypotheses", "orbh_select_batch_device", "orbh_select",
             "orbh_iterate", "orbh_iterate_batch"]
# include/orbo.h (tracking's motion-only pose optimisation)
EXPORTS_O = ["orbo_pose_batch_device", "orbo_pose", "orbo_pose_batch"]
# include/orbb.h (the bundle adjustment of the mapping thread)
# include/orbg.h (loop closing's Sim3 refinement)
EXPORTS_G = ["orbg_sim3_batch_device", "orbg_sim3", "orbg_sim3_batch"]
EXPORTS_B = ["orbb_state_from_float", "orbb_state_to_float", "orbb_work_bytes", "orbb_optimize_device", "orbb_optimize"]
# orbp_view.mode; MODE_SIM3: orbp_sim3_dir.mode
MODE_FRAME, MODE_LAST_FRAME, MODE_KEYFRAME, MODE_FUSE, MODE_LOOP, MODE_SIM3 = 0, 1, 2, 3, 4, 5
# orbp_fused.status
(FUSE_FUSED, FUSE_SKIPPED, FUSE_DEPTH, FUSE_IMAGE, FUSE_DISTANCE, FUSE_ANGLE, FUSE_EMPTY, FUSE_FAR) = range(8)
LOOP_QUERY = 8              # orbp_loop_*: the entry passed every test and is a query
# orbp_refresh*: `what` bits and orbp_refreshed.status
REFRESH_NORMAL_DEPTH, REFRESH_DESCRIPTOR = 1, 2
(REFRESH_OK, REFRESH_SKIPPED, REFRESH_EMPTY, REFRESH_BAD_INDEX, REFRESH_BAD_OCTAVE, REFRESH_NONFINITE) = range(6)


class OrbxError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("orbx error %d %s" % (code, msg))
        self.code = code


class Params(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int32), ("scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int32),
                ("score_type", ctypes.c_int32), ("fast_th", ctypes.c_int32), ("device", ctypes.c_int32),
                ("max_batch", ctypes.c_int32), ("blur_rounding", ctypes.c_int32), ("fp_contract", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)]


class StageVariant(ctypes.Structure):
    """orbx_stage_variant: the variant of a stage's first launch (-1: none), ORBX_VF_* flags, bit mask of every variant launched"""
    _fields_ = [("id", ctypes.c_int32), ("flags", ctypes.c_uint32), ("mask", ctypes.c_uint64)]


class PlanArgs(ctypes.Structure):
    """orbx_plan_args (include/orbx.h)"""
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("nframes", ctypes.c_int32), ("gather", ctypes.c_int32),
                ("xcd_affinity", ctypes.c_int32), ("on_demand", ctypes.c_int32), ("od_min_frames", ctypes.c_int32), ("stop_after", ctypes.c_int32),
                ("row_stride", ctypes.c_int64), ("frame_stride", ctypes.c_int64), ("base_bits", ctypes.c_uint32), ("color_fmt", ctypes.c_int32),
                ("color_gather", ctypes.c_int32), ("color_bits", ctypes.c_uint32), ("one_frame", ctypes.c_int32), ("side_stream", ctypes.c_int32),
                ("one_frame_bytes", ctypes.c_int64)]


# stages of orbx_debug_launch_variant / orbx_debug_plan (ORBX_VS_*) and the flags of a stage's launch (ORBX_VF_*)
VS_COLOR, VS_INGEST, VS_PYRAMID, VS_FAST, VS_QUOTA, VS_CELL_SELECT, VS_LEVEL_SELECT, VS_BLUR, VS_DESCRIBE, VS_COUNT = range(10)
VS_NAMES = ["color", "ingest", "pyramid", "fast", "quota", "cell_select", "level_select", "blur", "describe"]
VF_LDS_OVER_64K, VF_FUSE_BLUR, VF_OVERLAP, VF_ON_DEMAND, VF_XCD_AFFINITY = 1, 2, 4, 8, 16
XCD_AFFINITY_MIN_FRAMES = 64      # launch groups of at least this many frames renumber their blocks (orbx_internal.h)
OD_MIN_FRAMES_DEFAULT = 32        # ... of at least this many may blur per keypoint window (ORBX_OD_MIN_FRAMES_DEFAULT)


class Camera(ctypes.Structure):
    """orbf_camera: mK (row-major 3x3), mDistCoef, image size"""
    _fields_ = [("K", ctypes.c_float * 9), ("dist", ctypes.c_float * 8), ("ndist", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32)]

    @classmethod
    def make(cls, fx, fy, cx, cy, dist, width, height):
        c = cls()
        for i, v in enumerate((fx, 0, cx, 0, fy, cy, 0, 0, 1)):
            c.K[i] = v
        for i, v in enumerate(dist):
            c.dist[i] = v
        c.ndist, c.width, c.height = len(dist), width, height
        return c


class Bounds(ctypes.Structure):
    """orbf_bounds: Frame::mnMinX/mnMaxX/mnMinY/mnMaxY and the inverse grid cell sizes"""
    _fields_ = [("min_x", ctypes.c_int32), ("max_x", ctypes.c_int32), ("min_y", ctypes.c_int32), ("max_y", ctypes.c_int32),
                ("inv_w", ctypes.c_float), ("inv_h", ctypes.c_float)]

    def astuple(self):
        return (self.min_x, self.max_x, self.min_y, self.max_y, self.inv_w, self.inv_h)


class SearchParams(ctypes.Structure):
    """orbs_params"""
    _fields_ = [("rule", ctypes.c_int32), ("th", ctypes.c_int32), ("ratio", ctypes.c_float), ("check_orientation", ctypes.c_int32)]


class View(ctypes.Structure):
    """orbp_view: one pose + camera + (view_cos_limit, th) of Tracking's local-map search"""
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("Ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_int32), ("max_x", ctypes.c_int32), ("min_y", ctypes.c_int32), ("max_y", ctypes.c_int32),
                ("view_cos_limit", ctypes.c_float), ("th", ctypes.c_float), ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    @classmethod
    def make(cls, Rcw, tcw, Ow, fx, fy, cx, cy, min_x, max_x, min_y, max_y, view_cos_limit=0.5, th=1.0):
        v = cls()
        v.Rcw[:] = [float(x) for x in np.asarray(Rcw, np.float32).reshape(9)]
        v.tcw[:] = [float(x) for x in np.asarray(tcw, np.float32).reshape(3)]
        v.Ow[:] = [float(x) for x in np.asarray(Ow, np.float32).reshape(3)]
        v.fx, v.fy, v.cx, v.cy = float(fx), float(fy), float(cx), float(cy)
        v.min_x, v.max_x, v.min_y, v.max_y = int(min_x), int(max_x), int(min_y), int(max_y)
        v.view_cos_limit, v.th, v.mode, v.reserved = float(view_cos_limit), float(th), 0, 0
        return v


def view_from_sim3(Scw, view):
    """orbp_view_from_sim3: Rcw, tcw and Ow of `view` (a View, or a VIEW_DTYPE array of one record) from the similarity Scw (4 x 4 or its rows
    0..2, float32); every other field stays.  Host arithmetic: needs no GPU.  Raises OrbxError(ORBX_ERR_ARG) for a zero or non-finite scale."""
    S = np.ascontiguousarray(np.asarray(Scw, dtype=np.float32).reshape(-1)[:12])
    assert S.size == 12
    if isinstance(view, np.ndarray):
        assert view.dtype == VIEW_DTYPE and view.size == 1 and view.flags.c_contiguous
        ptr = view.ctypes.data
    else:
        ptr = ctypes.addressof(view)
    rc = lib().orbp_view_from_sim3(S.ctypes.data, ptr)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbp_view_from_sim3")
    return view


def sim3_from_pair(s12, R12, t12, R1w, t1w, R2w, t2w, fx, fy, cx, cy, bounds, th):
    """orbp_sim3_from_pair: SearchBySim3's arguments and the two key frames' poses -> SIM3_DIR_DTYPE[2], direction 1 -> 2 (R1w, t1w, sR21, t21) and
    direction 2 -> 1 (R2w, t2w, sR12, t12).  Host arithmetic: needs no GPU.  Raises OrbxError(ORBX_ERR_ARG) for a zero or non-finite scale."""
    a = lambda x, n: np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(n))
    R12, t12, R1w, t1w, R2w, t2w = a(R12, 9), a(t12, 3), a(R1w, 9), a(t1w, 3), a(R2w, 9), a(t2w, 3)
    dirs = np.zeros(2, SIM3_DIR_DTYPE)
    rc = lib().orbp_sim3_from_pair(float(s12), R12.ctypes.data, t12.ctypes.data, R1w.ctypes.data, t1w.ctypes.data, R2w.ctypes.data, t2w.ctypes.data,
                                   float(fx), float(fy), float(cx), float(cy), ctypes.addressof(bounds), float(th), dirs.ctypes.data)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbp_sim3_from_pair")
    return dirs


class TriCamera(ctypes.Structure):
    """orbt_camera: one key frame's pose and camera"""
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("Ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float)]


class TriPair(ctypes.Structure):
    """orbt_pair: (mpCurrentKeyFrame, pKF2) and mfScaleFactor of the first"""
    _fields_ = [("kf1", TriCamera), ("kf2", TriCamera), ("scale_factor", ctypes.c_float), ("reserved", ctypes.c_int32)]


TRI_CAMERA_DTYPE = np.dtype([("Rcw", np.float32, 9), ("tcw", np.float32, 3), ("Ow", np.float32, 3), ("fx", np.float32), ("fy", np.float32),
                             ("cx", np.float32), ("cy", np.float32)])
# orbt_pair as a numpy record (arrays of pairs are uploaded as they are)
TRI_PAIR_DTYPE = np.dtype([("kf1", TRI_CAMERA_DTYPE), ("kf2", TRI_CAMERA_DTYPE), ("scale_factor", np.float32), ("reserved", np.int32)])
assert TRI_PAIR_DTYPE.itemsize == ctypes.sizeof(TriPair) == 160

# orbi_problem / orbi_pose as numpy records (include/orbi.h)
INIT_PROBLEM_DTYPE = np.dtype([("norm1", np.float32, 4), ("norm2", np.float32, 4), ("sigma", np.float32), ("n1", np.int32), ("n2", np.int32),
                               ("nmatches", np.int32), ("iters", np.int32), ("reserved", np.int32)])
INIT_POSE_DTYPE = np.dtype([("R", np.float32, 9), ("t", np.float32, 3), ("P2", np.float32, 12), ("O2", np.float32, 3)])
assert INIT_PROBLEM_DTYPE.itemsize == 56 and INIT_POSE_DTYPE.itemsize == 108
# orbe_problem / orbe_state / orbe_result as numpy records (include/orbe.h)
PNP_PROBLEM_DTYPE = np.dtype([("fu", np.float32), ("fv", np.float32), ("uc", np.float32), ("vc", np.float32), ("n", np.int32), ("iters", np.int32),
                              ("min_inliers", np.int32), ("max_its", np.int32)])
PNP_STATE_DTYPE = np.dtype([("iterations", np.int32), ("best_inliers", np.int32), ("refine_ok", np.int32), ("refined_inliers", np.int32),
                            ("best_tcw", np.float32, 12), ("refined_tcw", np.float32, 12)])
PNP_RESULT_DTYPE = np.dtype([("kind", np.int32), ("stop", np.int32), ("no_more", np.int32), ("ninliers", np.int32), ("tcw", np.float32, 12)])
assert PNP_PROBLEM_DTYPE.itemsize == 32 and PNP_STATE_DTYPE.itemsize == 112 and PNP_RESULT_DTYPE.itemsize == 64
PNP_KIND_NONE, PNP_KIND_BEST, PNP_KIND_REFINED = 0, 1, 2
PNP_MAX_PROBLEMS, PNP_MAX_POINTS, PNP_MAX_ITERS = 32, 8192, 1024
# orbh_problem / orbh_hyp / orbh_state / orbh_result as numpy records (include/orbh.h)
SIM3SOLVER_PROBLEM_DTYPE = np.dtype([("fx1", np.float32), ("fy1", np.float32), ("cx1", np.float32), ("cy1", np.float32), ("fx2", np.float32),
                                     ("fy2", np.float32), ("cx2", np.float32), ("cy2", np.float32), ("n", np.int32), ("iters", np.int32),
                                     ("min_inliers", np.int32), ("max_its", np.int32)])
SIM3SOLVER_HYP_DTYPE = np.dtype([("q", np.float64, 4), ("R", np.float32, 9), ("t", np.float32, 3), ("s", np.float32), ("T12", np.float32, 16),
                                 ("T21", np.float32, 16), ("count", np.int32)])
SIM3SOLVER_STATE_DTYPE = np.dtype([("iterations", np.int32), ("best_inliers", np.int32), ("best_T12", np.float32, 16), ("best_R", np.float32, 9),
                                   ("best_t", np.float32, 3), ("best_s", np.float32)])
SIM3SOLVER_RESULT_DTYPE = np.dtype([("found", np.int32), ("stop", np.int32), ("no_more", np.int32), ("ninliers", np.int32), ("T12", np.float32, 16)])
assert SIM3SOLVER_PROBLEM_DTYPE.itemsize == 48 and SIM3SOLVER_HYP_DTYPE.itemsize == 216 and SIM3SOLVER_STATE_DTYPE.itemsize == 124 and \
    SIM3SOLVER_RESULT_DTYPE.itemsize == 80
SIM3SOLVER_MAX_PROBLEMS, SIM3SOLVER_MAX_POINTS, SIM3SOLVER_MAX_ITERS, SIM3SOLVER_POINT_ROWS = 32, 8192, 1024, 12
# orbo_problem / orbo_result / orbo_step as numpy records (include/orbo.h)
POSEOPT_PROBLEM_DTYPE = np.dtype([("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("n", np.int32)])
POSEOPT_RESULT_DTYPE = np.dtype([("Tcw", np.float32, 16), ("q", np.float64, 4), ("t", np.float64, 3), ("ninitial", np.int32), ("nbad", np.int32),
                                 ("rounds", np.int32), ("iters", np.int32, 4), ("noutlier", np.int32)])
POSEOPT_STEP_DTYPE = np.dtype([("chi_in", np.float64), ("chi_out", np.float64), ("lambda", np.float64), ("trials", np.int32), ("status", np.int32)])
assert POSEOPT_PROBLEM_DTYPE.itemsize == 20 and POSEOPT_RESULT_DTYPE.itemsize == 152 and POSEOPT_STEP_DTYPE.itemsize == 32
POSEOPT_MAX_PROBLEMS, POSEOPT_MAX_EDGES, POSEOPT_EDGE_ROWS, POSEOPT_ROUNDS, POSEOPT_MAX_ITERS = 64, 8192, 6, 4, 32
POSEOPT_ROUND_SLOT = (0, 10, 20, 27)        # a round's first record of the trace
POSEOPT_OK, POSEOPT_TERMINATE, POSEOPT_NOT_RUN = 0, 1, 2
# orbg_problem / orbg_result as numpy records (include/orbg.h); the trace is POSEOPT_STEP_DTYPE[SIM3OPT_MAX_ITERS]
SIM3OPT_PROBLEM_DTYPE = np.dtype([("fx1", np.float32), ("fy1", np.float32), ("cx1", np.float32), ("cy1", np.float32), ("fx2", np.float32),
                                  ("fy2", np.float32), ("cx2", np.float32), ("cy2", np.float32), ("th2", np.float32), ("n", np.int32)])
SIM3OPT_RESULT_DTYPE = np.dtype([("q", np.float64, 4), ("t", np.float64, 3), ("s", np.float64), ("S12", np.float32, 16), ("ncorr", np.int32),
                                 ("nbad", np.int32), ("nin", np.int32), ("ret0", np.int32), ("iters", np.int32, 2)])
assert SIM3OPT_PROBLEM_DTYPE.itemsize == 40 and SIM3OPT_RESULT_DTYPE.itemsize == 152
SIM3OPT_MAX_PROBLEMS, SIM3OPT_MAX_PAIRS, SIM3OPT_PAIR_ROWS, SIM3OPT_MAX_ITERS = 64, 8192, 12, 15
SIM3OPT_PHASE_SLOT = (0, 5)                 # a phase's first record of the trace
# orbb_problem / orbb_result as numpy records (include/orbb.h); the trace is POSEOPT_STEP_DTYPE[LOCALBA_MAX_ITERS]
LOCALBA_PROBLEM_DTYPE = np.dtype([("nfree", np.int32), ("nfixed", np.int32), ("npoints", np.int32), ("nedges", np.int32)])
LOCALBA_RESULT_DTYPE = np.dtype([("chi_first", np.float64), ("chi_last", np.float64), ("lambda", np.float64), ("iters", np.int32), ("status", np.int32),
                                 ("launches", np.int32), ("syncs", np.int32)])
assert LOCALBA_PROBLEM_DTYPE.itemsize == 16 and LOCALBA_RESULT_DTYPE.itemsize == 40
LOCALBA_MAX_FREE, LOCALBA_MAX_POSES, LOCALBA_MAX_POINTS, LOCALBA_MAX_EDGES, LOCALBA_MAX_ITERS = 128, 4096, 1 << 20, 1 << 22, 64
LOCALBA_REDUCE_LANES, LOCALBA_CTL = 1024, 8
LOCALBA_RUN_OK, LOCALBA_RUN_TERMINATE, LOCALBA_RUN_NOTHING = 0, 1, 2

# orbp_view / orbp_record as numpy records (arrays of views are uploaded as they are)
VIEW_DTYPE = np.dtype([("Rcw", np.float32, 9), ("tcw", np.float32, 3), ("Ow", np.float32, 3), ("fx", np.float32), ("fy", np.float32),
                       ("cx", np.float32), ("cy", np.float32), ("min_x", np.int32), ("max_x", np.int32), ("min_y", np.int32),
                       ("max_y", np.int32), ("view_cos_limit", np.float32), ("th", np.float32), ("mode", np.int32), ("reserved", np.int32)])
RECORD_DTYPE = np.dtype([("in_view", np.uint8), ("pad", np.uint8, 3), ("u", np.float32), ("v", np.float32), ("view_cos", np.float32),
                         ("level", np.int32)])
assert VIEW_DTYPE.itemsize == ctypes.sizeof(View) == 108 and RECORD_DTYPE.itemsize == 20
# orbp_refreshed
REFRESHED_DTYPE = np.dtype([("normal", np.float32, 3), ("min_dist", np.float32), ("max_dist", np.float32), ("best_obs", np.int32),
                            ("best_median", np.int32), ("status", np.int32)])
assert REFRESHED_DTYPE.itemsize == 32
# orbp_fused
FUSED_DTYPE = np.dtype([("u", np.float32), ("v", np.float32), ("level", np.int32), ("status", np.int32)])
assert FUSED_DTYPE.itemsize == 16
# orbp_sim3_dir: one direction of one pair of orbp_sim3_search* (arrays of directions are uploaded as they are)
SIM3_DIR_DTYPE = np.dtype([("Raw", np.float32, 9), ("taw", np.float32, 3), ("S", np.float32, 9), ("t", np.float32, 3), ("fx", np.float32),
                           ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("min_x", np.int32), ("max_x", np.int32), ("min_y", np.int32),
                           ("max_y", np.int32), ("th", np.float32), ("mode", np.int32), ("reserved", np.int32, 2)])
assert SIM3_DIR_DTYPE.itemsize == 144

GRID_COLS, GRID_ROWS = 64, 48
GRID_CELLS = GRID_COLS * GRID_ROWS

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OrbxError(ORBX_ERR_DEVICE, "liborbx.so not built: run `make` / __graft_entry__.build()")
        # One HIP runtime per process: PyTorch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  If torch
        # is imported first, liborbx binds to that copy and torch streams / device pointers are directly usable;
        # the other order loads a second runtime next to torch's and torch then sees no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
        pd = ctypes.c_ssize_t
        L.orbx_default_params.argtypes = [ctypes.POINTER(Params)]
        L.orbx_default_params.restype = None
        L.orbx_create.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(vp)]
        L.orbx_destroy.argtypes = [vp]
        L.orbx_destroy.restype = None
        L.orbx_get_levels.argtypes = [vp]
        L.orbx_get_scale_factor.argtypes = [vp]
        L.orbx_get_scale_factor.restype = cf
        L.orbx_max_keypoints.argtypes = [vp]
        L.orbx_last_error.argtypes = [vp]
        L.orbx_last_error.restype = ctypes.c_char_p
        L.orbx_build_id.argtypes = []
        L.orbx_build_id.restype = ctypes.c_char_p
        L.orbx_extract.argtypes = [vp, vp, ci, ci, pd, vp, vp, ci, ctypes.POINTER(ci)]
        L.orbx_extract_batch_device.argtypes = [vp, vp, ci, ci, ci, pd, pd, vp, vp, vp, ci, vp, vp]
        L.orbx_extract_batch_device_phases.argtypes = [vp, vp, ci, ci, ci, pd, pd, vp, vp, vp, ci, vp, vp, ci]
        L.orbx_extract_batch.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp]
        L.orbx_to_gray_device.argtypes = [vp, ci, ci, ci, pd, pd, ci, vp, pd, pd, vp]
        L.orbx_extract_color.argtypes = [vp, vp, ci, ci, pd, ci, vp, vp, ci, ctypes.POINTER(ci), vp]
        L.orbx_extract_batch_device_color.argtypes = [vp, vp, ci, ci, ci, pd, pd, ci, vp, vp, vp, ci, vp, vp, pd, pd, vp]
        L.orbx_extract_batch_color.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp]
        L.orbm_hamming256.argtypes = [vp, vp]
        L.orbm_match_top2.argtypes = [vp, ci, vp, ci, vp, vp, vp, ci]
        L.orbm_match_top2_device.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp]
        L.orbm_match_top2_batch_device.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
        L.orbm_match_top2_masked.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, ci]
        L.orbm_match_top2_masked_device.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp]
        L.orbm_count_accepted.argtypes = [vp, vp, ci, ci, cf]
        L.orbm_debug_set_match_path.argtypes = [ci]
        L.orbm_debug_get_match_path.argtypes = []
        L.orbs_debug_set_buckets.argtypes = [ci]
        L.orbs_debug_set_wide_max.argtypes = [ci]
        L.orbm_match_top2_segments.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp, ci]
        L.orbm_match_top2_segments_device.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp]
        L.orbx_device_alloc.argtypes = [ci, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.orbx_device_free.argtypes = [ci, vp]
        L.orbx_device_upload.argtypes = [ci, vp, vp, ctypes.c_size_t]
        L.orbx_device_download.argtypes = [ci, vp, vp, ctypes.c_size_t]
        L.orbm_distinctive.argtypes = [vp, vp, ci, vp, vp, ci]
        L.orbm_distinctive_device.argtypes = [vp, vp, ci, vp, vp, vp]
        L.orbx_debug_set_stop_after.argtypes = [vp, ci]
        L.orbx_debug_set_blur_on_demand.argtypes = [vp, ci]
        L.orbx_debug_level_size.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        if hasattr(L, "orbx_debug_resize_form"):       # (an older library through ORBX_LIB, for an A/B, lacks it)
            L.orbx_debug_resize_form.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        if hasattr(L, "orbx_debug_launch_variant"):    # (likewise)
            L.orbx_debug_launch_variant.argtypes = [vp, ci, ctypes.POINTER(StageVariant), ctypes.c_char_p, ci]
            L.orbx_debug_variant_count.argtypes = [ci]
            L.orbx_debug_variant_name.argtypes = [ci, ci]
            L.orbx_debug_variant_name.restype = ctypes.c_char_p
            L.orbx_debug_plan.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(PlanArgs), ctypes.POINTER(StageVariant)]
        L.orbx_debug_fetch.argtypes = [vp, ci, ci, ci, vp, cl]
        L.orbx_debug_fetch.restype = cl
        L.orbx_debug_eval_math.argtypes = [ci, vp, vp, vp, vp, ci, ci]
        L.orbx_debug_eval_compass.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci]
        if hasattr(L, "orbx_debug_eval_score"):        # (likewise)
            L.orbx_debug_eval_score.argtypes = [vp, vp, vp, vp, ci, ci, ci]
        L.orbx_debug_eval_blur_window.argtypes = [vp, vp, ci, ci, ci, ci]
        L.orbx_debug_nth_element.argtypes = [vp, ci, ci, vp, ci]
        L.orbx_debug_geometry.argtypes = [ctypes.POINTER(Params), ci, ci, vp, ci]
        L.orbx_debug_stage_timing.argtypes = [vp, ci]
        L.orbx_debug_stage_time.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(cl)]
        L.orbf_image_bounds.argtypes = [ctypes.POINTER(Camera), ctypes.POINTER(Bounds)]
        L.orbf_undistort_grid.argtypes = [ctypes.POINTER(Camera), ctypes.POINTER(Bounds), vp, ci, vp, vp, vp, ci]
        L.orbf_undistort_grid_batch_device.argtypes = [ctypes.POINTER(Camera), ctypes.POINTER(Bounds), vp, vp, ci, ci, vp, vp, vp, vp]
        L.orbf_features_in_area.argtypes = [ctypes.POINTER(Bounds), vp, ci, vp, vp, vp, vp, ci, vp, vp, ci, ci]
        L.orbf_features_in_area_device.argtypes = [ctypes.POINTER(Bounds), vp, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp]
        L.orbs_lds_bytes.argtypes = [ci, ci]
        L.orbs_lds_bytes.restype = ctypes.c_size_t
        L.orbs_three_maxima.argtypes = [vp, ci, vp]
        L.orbs_three_maxima.restype = None
        L.orbs_window_search_batch_device.argtypes = [ctypes.POINTER(Bounds), ctypes.POINTER(SearchParams), vp, vp, vp, vp, vp, ci, vp,
                                                      vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
        L.orbs_list_search_batch_device.argtypes = [ctypes.POINTER(SearchParams), vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci,
                                                    vp, vp, vp, vp, vp, vp]
        L.orbs_bow_ranges_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        L.orbs_triangulation_search_batch_device.argtypes = [ctypes.POINTER(SearchParams), vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp,
                                                             vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
        L.orbs_epipolar_bound.argtypes = [ctypes.c_float]
        L.orbs_epipolar_bound.restype = ctypes.c_float
        L.orbs_agreement_batch_device.argtypes = [vp, vp, ci, vp, vp, ci, ci, vp, vp, vp]
        L.orbs_bow_rows_search_batch_device.argtypes = [ctypes.POINTER(SearchParams), vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbs_bow_rows_search.argtypes = [ctypes.POINTER(SearchParams), vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbs_tri_rows_search_batch_device.argtypes = [ctypes.POINTER(SearchParams), vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp,
                                                        vp, vp]
        L.orbs_tri_rows_search.argtypes = [ctypes.POINTER(SearchParams), vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        L.orbv_create.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, ctypes.POINTER(vp)]
        L.orbv_load_text.argtypes = [ctypes.c_char_p, ci, ctypes.POINTER(vp)]
        L.orbv_destroy.argtypes = [vp]
        L.orbv_destroy.restype = None
        L.orbv_info.argtypes = [vp] + [ctypes.POINTER(ci)] * 6
        L.orbv_descend.argtypes = [vp, vp, ci, ci, vp, vp, vp]
        L.orbv_descend_device.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
        L.orbv_transform.argtypes = [vp, vp, ci, ci, vp, vp, ctypes.POINTER(ci), vp, vp, vp, ctypes.POINTER(ci)]
        L.orbv_transform_batch_device.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbv_score.argtypes = [vp, vp, vp, ci, vp, vp, ci]
        L.orbv_score.restype = ctypes.c_double
        L.orbd_create.argtypes = [vp, ci, ci, ctypes.POINTER(vp)]
        L.orbd_destroy.argtypes = [vp]
        L.orbd_destroy.restype = None
        L.orbd_size.argtypes = [vp]
        L.orbd_add.argtypes = [vp, ci, vp, vp, ci]
        L.orbd_add_batch_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp]
        L.orbd_erase.argtypes = [vp, ci]
        L.orbd_clear.argtypes = [vp]
        L.orbd_query_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
        L.orbd_query.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), vp]
        L.orbp_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
        L.orbp_destroy.argtypes = [vp]
        L.orbp_destroy.restype = None
        L.orbp_capacity.argtypes = [vp]
        L.orbp_size.argtypes = [vp]
        L.orbp_clear.argtypes = [vp]
        L.orbp_put.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
        L.orbp_put_device.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp]
        L.orbp_erase.argtypes = [vp, vp, ci]
        L.orbp_get.argtypes = [vp, ci, ctypes.POINTER(ci), vp, vp, vp, vp, vp]
        L.orbp_project_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        L.orbp_track_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, ctypes.POINTER(Bounds), cf, vp, vp, vp, vp, vp, ci, vp, ci,
                                              vp, vp, vp, vp, vp, vp]
        L.orbp_track.argtypes = [vp, ctypes.POINTER(View), vp, ci, vp, ci, vp, ctypes.POINTER(Bounds), cf, vp, vp, vp, vp, vp, ci, ci, ci,
                                 vp, vp, ctypes.POINTER(ci), ctypes.POINTER(ci), vp]
        L.orbp_refresh_batch_device.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, vp, vp]
        L.orbp_refresh.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, vp, vp]
        L.orbp_fuse_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.orbp_fuse.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
        L.orbp_view_from_sim3.argtypes = [vp, vp]
        cf = ctypes.c_float
        L.orbp_sim3_from_pair.argtypes = [cf, vp, vp, vp, vp, vp, vp, cf, cf, cf, cf, vp, cf, vp]
        L.orbp_sim3_search_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp]
        L.orbp_sim3_search.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp]
        L.orbp_loop_project_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        L.orbp_loop_search_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        L.orbp_loop_search.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, ctypes.POINTER(ci), ctypes.POINTER(ci), vp]
        L.orbp_local_votes_batch_device.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, vp, vp]
        L.orbp_local_votes.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, ci, vp, vp]
        L.orbp_local_points_batch_device.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp, ci, vp]
        L.orbp_local_points.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, vp]
        L.orbp_rows_purge_device.argtypes = [vp, vp, ci, vp, ci, ci, vp]
        L.orbp_cull_batch_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]
        L.orbp_cull.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp]
        L.orbp_project_source_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        L.orbp_track_source_batch_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, ctypes.POINTER(Bounds), ctypes.POINTER(SearchParams),
                                                     vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp]
        L.orbp_track_source.argtypes = [vp, ctypes.POINTER(View), vp, ci, vp, ci, vp, vp, vp, ci, ctypes.POINTER(Bounds), ctypes.POINTER(SearchParams),
                                        vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, ctypes.POINTER(ci), ctypes.POINTER(ci), vp]
        L.orbt_triangulate_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, ci, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                                    ci, vp, vp, vp]
        L.orbt_triangulate.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, ctypes.POINTER(ci), ci]
        L.orbt_new_points_rows_device.argtypes = [ctypes.POINTER(SearchParams), vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp,
                                                  vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        L.orbt_new_points_rows.argtypes = [ctypes.POINTER(SearchParams), vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        pnp_bind(L)
        sim3solver_bind(L)
        poseopt_bind(L)
        sim3opt_bind(L)
        localba_bind(L)
        L.orbi_normalize.argtypes = [vp, ci, vp]
        L.orbi_pose_from_rt.argtypes = [cf, cf, cf, cf, vp, vp, vp]
        L.orbi_models_batch_device.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbi_models.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci]
        L.orbi_check_rt_batch_device.argtypes = [cf, cf, cf, cf, vp, ci, ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, cf, vp, vp, vp, vp, vp, vp, vp]
        L.orbi_check_rt.argtypes = [cf, cf, cf, cf, vp, ci, vp, ci, vp, ci, vp, ci, vp, cf, vp, vp, vp, vp, vp, vp, vp, ci]
        _LIB = L
    return _LIB


FRAMES_ON_DEVICE, FRAMES_ON_HOST = 0, 1     # orbx_extract_batch's `where`


def frame_table(frames):
    """The arguments orbx_extract_batch takes for a list of 2-D uint8 frames of one size: (where, pointers, row strides, w, h, keep).
    CUDA tensors give the device form (row stride = stride(0), stride(1) must be 1); numpy arrays and CPU tensors the host form (host
    frames whose rows are not contiguous are copied first; `keep` holds what must stay alive during the call).  Needs no GPU."""
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    on_dev = [bool(getattr(f, "is_cuda", False)) for f in frames]
    if any(on_dev) and not all(on_dev):
        raise ValueError("frames mix device and host memory")
    ptrs, strides, keep, shape = [], [], [], None
    for f in frames:
        if hasattr(f, "data_ptr"):                 # torch tensor (device or host)
            import torch
            if f.dtype != torch.uint8 or f.dim() != 2:
                raise ValueError("frames must be 2-D uint8")
            if f.stride(1) != 1 or f.stride(0) < f.shape[1]:
                if f.is_cuda:
                    raise ValueError("device frame rows must be contiguous (stride(1) == 1)")
                f = f.contiguous()
            hw, p, rs = tuple(f.shape), f.data_ptr(), f.stride(0)
        else:
            a = np.asarray(f)
            if a.dtype != np.uint8 or a.ndim != 2:
                raise ValueError("frames must be 2-D uint8")
            if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
                a = np.ascontiguousarray(a)
            hw, p, rs = a.shape, a.ctypes.data, a.strides[0]
            f = a
        if shape is None:
            shape = hw
        elif hw != shape:
            raise ValueError("frames differ in size: %s vs %s" % (hw, shape))
        keep.append(f)
        ptrs.append(p)
        strides.append(rs)
    return (FRAMES_ON_DEVICE if on_dev[0] else FRAMES_ON_HOST, np.array(ptrs, dtype=np.uint64), np.array(strides, dtype=np.int64),
            shape[1], shape[0], keep)


# pixel formats of the colour entry points (include/orbx.h ORBX_PIX_*): Tracking::GrabImage's cvtColor in front of the extractor
PIX_GRAY8, PIX_RGB8, PIX_BGR8, PIX_RGBA8, PIX_BGRA8 = 0, 1, 2, 3, 4
PIX_CHANNELS = {PIX_GRAY8: 1, PIX_RGB8: 3, PIX_BGR8: 3, PIX_RGBA8: 4, PIX_BGRA8: 4}


def pix_channels(fmt):
    """bytes per pixel of an ORBX_PIX_* format; ValueError for an unknown one"""
    if fmt not in PIX_CHANNELS:
        raise ValueError("unknown pixel format %r" % (fmt,))
    return PIX_CHANNELS[fmt]


def color_layout(frame, fmt):
    """(pointer, w, h, row stride in bytes, on device, keep) of one (H, W, C) uint8 frame of format fmt (C = its channels; a GRAY8 frame may
    also be (H, W)).  Any row stride is accepted; the pixels of a row must be packed (pixel stride C, channel stride 1).  Host frames that
    are not are copied (`keep` holds what must stay alive during the call); device frames raise.  Needs no GPU."""
    ch = pix_channels(fmt)
    if hasattr(frame, "data_ptr"):                 # torch tensor (device or host)
        import torch
        if frame.dtype != torch.uint8:
            raise ValueError("frames must be uint8")
        f = frame.unsqueeze(-1) if frame.dim() == 2 and ch == 1 else frame
        if f.dim() != 3 or f.shape[2] != ch:
            raise ValueError("format %d wants (H, W, %d) frames, got %s" % (fmt, ch, tuple(frame.shape)))
        if f.stride(2) != 1 or f.stride(1) != ch or f.stride(0) < f.shape[1] * ch:
            if f.is_cuda:
                raise ValueError("device frame pixels must be packed (stride(1) == channels, stride(2) == 1)")
            f = f.contiguous()
        return f.data_ptr(), int(f.shape[1]), int(f.shape[0]), int(f.stride(0)), bool(f.is_cuda), f
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise ValueError("frames must be uint8")
    if a.ndim == 2 and ch == 1:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] != ch:
        raise ValueError("format %d wants (H, W, %d) frames, got %s" % (fmt, ch, a.shape))
    if a.strides[2] != 1 or a.strides[1] != ch or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
    return a.ctypes.data, int(a.shape[1]), int(a.shape[0]), int(a.strides[0]), False, a


def color_frame_table(frames, fmt):
    """frame_table for colour frames: (where, pointers, row strides, w, h, keep) of a list of (H, W, C) uint8 frames of one size and format
    (see color_layout).  CUDA tensors give the device form, numpy arrays and CPU tensors the host form.  Needs no GPU."""
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    lay = [color_layout(f, fmt) for f in frames]
    if len({l[4] for l in lay}) != 1:
        raise ValueError("frames mix device and host memory")
    if len({(l[1], l[2]) for l in lay}) != 1:
        raise ValueError("frames differ in size")
    return (FRAMES_ON_DEVICE if lay[0][4] else FRAMES_ON_HOST, np.array([l[0] for l in lay], dtype=np.uint64),
            np.array([l[3] for l in lay], dtype=np.int64), lay[0][1], lay[0][2], [l[5] for l in lay])


def to_gray_device(d_src, nframes, w, h, src_row_stride, src_frame_stride, fmt, d_gray, gray_row_stride, gray_frame_stride, stream=0):
    """orbx_to_gray_device on integer device addresses.  Asynchronous on `stream`."""
    pix_channels(fmt)
    rc = lib().orbx_to_gray_device(d_src, nframes, w, h, src_row_stride, src_frame_stride, fmt, d_gray, gray_row_stride, gray_frame_stride,
                                   stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_to_gray_device")


def to_gray(frames, fmt, stream=0):
    """(F, H, W, C) or (H, W, C) CUDA uint8 tensor (rows and frames at any stride, packed pixels) -> new (F, H, W) / (H, W) gray tensor"""
    import torch
    one = frames.dim() == 3
    x = frames.unsqueeze(0) if one else frames
    ch = pix_channels(fmt)
    if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != ch or x.stride(3) != 1 or x.stride(2) != ch:
        raise ValueError("to_gray wants a CUDA uint8 (F, H, W, %d) tensor with packed pixels" % ch)
    F, h, w = x.shape[:3]
    out = torch.empty((F, h, w), dtype=torch.uint8, device=x.device)
    to_gray_device(x.data_ptr(), F, w, h, x.stride(1), x.stride(0), fmt, out.data_ptr(), w, w * h, stream)
    return out[0] if one else out


class ORBextractor:
    """Same constructor arguments as the reference ORBextractor(nfeatures, scaleFactor, nlevels, scoreType, fastTh)
    (include/ORBextractor.h:38) plus device placement; __call__(image) is operator()."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=FAST_SCORE, fastTh=20,
                 device=0, max_batch=1, blur_rounding=BLUR_X86_SSE2, fp_contract=None):
        L = lib()
        p = Params()
        L.orbx_default_params(ctypes.byref(p))
        p.nfeatures, p.scale_factor, p.nlevels, p.score_type, p.fast_th = nfeatures, scaleFactor, nlevels, scoreType, fastTh
        p.device, p.max_batch, p.blur_rounding = device, max_batch, blur_rounding
        if fp_contract is not None:                      # None: orbx_default_params' choice (ORBX_FP_CONTRACT in the environment, else ISO)
            p.fp_contract = 1 if fp_contract else 0
        h = ctypes.c_void_p()
        rc = L.orbx_create(ctypes.byref(p), ctypes.byref(h))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbx_create (is a gfx950 GPU visible?)")
        self.h = h
        self.L = L
        self.max_keypoints = L.orbx_max_keypoints(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.orbx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def GetLevels(self):
        return self.L.orbx_get_levels(self.h)

    def GetScaleFactor(self):
        return self.L.orbx_get_scale_factor(self.h)

    def _err(self, rc):
        return OrbxError(rc, self.L.orbx_last_error(self.h).decode())

    def __call__(self, image):
        """image: 2-D uint8 array.  Returns (keypoints[N] (KP_DTYPE), descriptors[N,32] uint8)."""
        img = np.asarray(image)
        if img.size == 0:
            return None   # reference: silent return, outputs untouched
        assert img.dtype == np.uint8 and img.ndim == 2
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        hh, w = img.shape
        cap = self.max_keypoints
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), dtype=np.uint8)
        n = ctypes.c_int(0)
        rc = self.L.orbx_extract(self.h, img.ctypes.data, w, hh, img.strides[0], kps.ctypes.data, desc.ctypes.data, cap, ctypes.byref(n))
        if rc != ORBX_OK:
            raise self._err(rc)
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch_device(self, d_imgs, nframes, w, h, row_stride, frame_stride, d_kps, d_desc, d_n, cap, d_status=0, stream=0, phases=PHASE_ALL):
        """All pointer arguments are integer device addresses (e.g. torch tensor.data_ptr()).  Asynchronous.
        phases: PHASE_* bit mask (orbx_extract_batch_device_phases); the parts of one batch go to one stream, in order."""
        rc = self.L.orbx_extract_batch_device_phases(self.h, d_imgs, nframes, w, h, row_stride, frame_stride, d_kps, d_desc, d_n, cap,
                                                     d_status or None, stream or None, phases)
        if rc != ORBX_OK:
            raise self._err(rc)

    def extract_batch(self, frames, d_kps, d_desc, d_n, cap, d_status=0, stream=0):
        """orbx_extract_batch: frames is a list of 2-D uint8 frames of one size (see frame_table: CUDA tensors = device form, numpy arrays
        or CPU tensors = host form); outputs are integer device addresses, frame f's results at slot f.  Asynchronous on `stream` (the
        host form returns once the frames have been read)."""
        where, ptrs, strides, w, h, keep = frame_table(frames)
        rc = self.L.orbx_extract_batch(self.h, ptrs.ctypes.data, strides.ctypes.data, len(ptrs), w, h, where, d_kps, d_desc, d_n, cap,
                                       d_status or None, stream or None)
        del keep
        if rc != ORBX_OK:
            raise self._err(rc)

    def extract_color(self, image, fmt, want_gray=False):
        """orbx_extract_color: image (H, W, C) uint8 of format fmt (PIX_*), any row stride.  Returns (keypoints, descriptors), plus the
        gray image (Frame::im) when want_gray."""
        ptr, w, hh, rs, on_dev, keep = color_layout(image, fmt)
        if on_dev:
            raise ValueError("extract_color takes a host frame")
        if w == 0 or hh == 0:
            return None   # reference: silent return, outputs untouched
        cap = self.max_keypoints
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), dtype=np.uint8)
        gray = np.empty((hh, w), dtype=np.uint8) if want_gray else None
        n = ctypes.c_int(0)
        rc = self.L.orbx_extract_color(self.h, ptr, w, hh, rs, fmt, kps.ctypes.data, desc.ctypes.data, cap, ctypes.byref(n),
                                       gray.ctypes.data if want_gray else None)
        del keep
        if rc != ORBX_OK:
            raise self._err(rc)
        res = (kps[:n.value].copy(), desc[:n.value].copy())
        return res + (gray,) if want_gray else res

    def extract_batch_device_color(self, d_imgs, nframes, w, h, row_stride, frame_stride, fmt, d_kps, d_desc, d_n, cap, d_status=0, d_gray=0,
                                   gray_row_stride=0, gray_frame_stride=0, stream=0):
        """orbx_extract_batch_device_color on integer device addresses (d_gray = 0: the handle's gray ring).  Asynchronous."""
        pix_channels(fmt)
        rc = self.L.orbx_extract_batch_device_color(self.h, d_imgs, nframes, w, h, row_stride, frame_stride, fmt, d_kps, d_desc, d_n, cap,
                                                    d_status or None, d_gray or None, gray_row_stride, gray_frame_stride, stream or None)
        if rc != ORBX_OK:
            raise self._err(rc)

    def extract_batch_color(self, frames, fmt, d_kps, d_desc, d_n, cap, d_status=0, stream=0):
        """orbx_extract_batch_color: frames is a list of (H, W, C) uint8 frames of one size (see color_frame_table: CUDA tensors = device
        form, numpy arrays or CPU tensors = host form); outputs as in extract_batch."""
        where, ptrs, strides, w, h, keep = color_frame_table(frames, fmt)
        rc = self.L.orbx_extract_batch_color(self.h, ptrs.ctypes.data, strides.ctypes.data, len(ptrs), w, h, where, fmt, d_kps, d_desc, d_n,
                                             cap, d_status or None, stream or None)
        del keep
        if rc != ORBX_OK:
            raise self._err(rc)

    # diagnostics
    def set_stop_after(self, stage):
        self.L.orbx_debug_set_stop_after(self.h, stage)

    def set_blur_on_demand(self, mode):
        """1: the blur per keypoint window inside the description kernel (full launch groups); 0: blur kernels + blurred plane"""
        rc = self.L.orbx_debug_set_blur_on_demand(self.h, int(mode))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbx_debug_set_blur_on_demand")

    STAGE_NAMES = ["pyramid", "fast_cells", "quota", "cell_select", "level_select", "blur", "describe"]

    def stage_timing(self, enable):
        """0 off, 1 on, 2 on + reset"""
        self.L.orbx_debug_stage_timing(self.h, enable)

    def stage_times(self):
        """-> {stage: (total_ms, launch_groups)} measured with HIP events on the launch stream"""
        res = {}
        for i, name in enumerate(self.STAGE_NAMES):
            ms, n = ctypes.c_double(), ctypes.c_long()
            self.L.orbx_debug_stage_time(self.h, i, ctypes.byref(ms), ctypes.byref(n))
            res[name] = (ms.value, n.value)
        return res

    def level_size(self, level):
        w, hh = ctypes.c_int(), ctypes.c_int()
        rc = self.L.orbx_debug_level_size(self.h, level, ctypes.byref(w), ctypes.byref(hh))
        if rc != ORBX_OK:
            raise self._err(rc)
        return w.value, hh.value

    def resize_form(self, level):
        """(form, rows_out) of pyramid level `level` in the last launch group: RZ_FORM_TILED / RZ_FORM_STRIP / RZ_FORM_FUSED"""
        form, rows = ctypes.c_int(), ctypes.c_int()
        rc = self.L.orbx_debug_resize_form(self.h, level, ctypes.byref(form), ctypes.byref(rows))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbx_debug_resize_form")
        return form.value, rows.value

    def launch_variant(self, stage):
        """(id, flags, mask, name) of stage VS_* in the last launch group: the variant of its first launch (-1 and "" when the stage launched
        nothing), VF_* flags, the bit mask of every variant it launched, the kernel's name with its template arguments"""
        v, name = StageVariant(), ctypes.create_string_buffer(96)
        rc = self.L.orbx_debug_launch_variant(self.h, stage, ctypes.byref(v), name, len(name))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbx_debug_launch_variant")
        return v.id, v.flags, v.mask, name.value.decode()

    def fetch_plane(self, what, level, frame=0):
        w, hh = self.level_size(level)
        out = np.empty((hh, w), dtype=np.uint8)
        rc = self.L.orbx_debug_fetch(self.h, what, frame, level, out.ctypes.data, out.nbytes)
        if rc < 0:
            raise self._err(rc)
        return out

    def fetch_bands(self, level, frame=0):
        """the FAST work items of a level after a run: int32 rows (x0, x1, y0, y1, n_all, n_hi, n_lo, list threshold)"""
        out = np.zeros((16384, 8), dtype=np.int32)
        rc = self.L.orbx_debug_fetch(self.h, DBG_BANDS, frame, level, out.ctypes.data, out.nbytes)
        if rc < 0:
            raise self._err(rc)
        return out[:rc // 32].copy()

    def fetch_level_keypoints(self, level, frame=0):
        out = np.zeros((4 * self.max_keypoints + 64, 3), dtype=np.int32)
        rc = self.L.orbx_debug_fetch(self.h, DBG_LEVEL_KPS, frame, level, out.ctypes.data, out.nbytes)
        if rc < 0:
            raise self._err(rc)
        n = rc // 12
        xy = out[:n, :2].copy()
        resp = out[:n, 2].copy().view(np.float32)
        return xy, resp


def hamming256(a, b):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    assert a.size == 32 and b.size == 32
    return lib().orbm_hamming256(a.ctypes.data, b.ctypes.data)


def match_top2(Q, T, device=0):
    """Host arrays [nq,32], [nt,32] uint8 -> (best_idx, best, second) int32 arrays (GPU computed)."""
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 32)
    nq, nt = len(Q), len(T)
    idx = np.empty(nq, np.int32)
    best = np.empty(nq, np.int32)
    sec = np.empty(nq, np.int32)
    rc = lib().orbm_match_top2(Q.ctypes.data, nq, T.ctypes.data, nt, idx.ctypes.data, best.ctypes.data, sec.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_match_top2")
    return idx, best, sec


def match_top2_masked(Q, T, t_valid, device=0):
    """dense top-2 over the train descriptors with t_valid != 0 only (src/ORBmatcher.cc:205-206); indices refer to T"""
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 32)
    v = np.ascontiguousarray(t_valid, dtype=np.uint8)
    nq, nt = len(Q), len(T)
    assert len(v) == nt
    idx = np.empty(nq, np.int32); best = np.empty(nq, np.int32); sec = np.empty(nq, np.int32)
    rc = lib().orbm_match_top2_masked(Q.ctypes.data, nq, T.ctypes.data, nt, v.ctypes.data if nt else None, idx.ctypes.data, best.ctypes.data, sec.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_match_top2_masked")
    return idx, best, sec


def match_top2_segments(Q, T, seg_off, cand, device=0):
    """per-query candidate lists (CSR): query q scans T[cand[seg_off[q]:seg_off[q+1]]] in list order"""
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 32)
    seg = np.ascontiguousarray(seg_off, dtype=np.int32)
    cd = np.ascontiguousarray(cand, dtype=np.int32)
    nq = len(Q)
    assert len(seg) == nq + 1
    idx = np.empty(nq, np.int32); best = np.empty(nq, np.int32); sec = np.empty(nq, np.int32)
    rc = lib().orbm_match_top2_segments(Q.ctypes.data, nq, T.ctypes.data, len(T), seg.ctypes.data, cd.ctypes.data if len(cd) else None,
                                        idx.ctypes.data, best.ctypes.data, sec.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_match_top2_segments")
    return idx, best, sec


def build_id():
    """hash of the kernel sources the loaded library was built from (Makefile -> orbx_build_id)"""
    return lib().orbx_build_id().decode()


def match_top2_device(dQ, nq, dT, nt, d_idx, d_best, d_second, stream=0):
    rc = lib().orbm_match_top2_device(dQ, nq, dT, nt, d_idx, d_best, d_second, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_match_top2_device")


def match_top2_batch_device(dQ, d_nq, dT, d_nt, nbatch, cap, d_idx, d_best, d_second, stream=0):
    rc = lib().orbm_match_top2_batch_device(dQ, d_nq, dT, d_nt, nbatch, cap, d_idx, d_best, d_second, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_match_top2_batch_device")


def get_match_path():
    """the dense top-2 kernels in effect: 0 xor + popcount, 1 int8 MFMA, 2 FP4 MFMA"""
    return int(lib().orbm_debug_get_match_path())


def set_match_path(path):
    """test hook: -1 process default (ORBX_MATCH_MFMA = 0 / 8 / 4), 0 xor + popcount kernels, 1 int8 MFMA kernels, 2 FP4 MFMA kernels"""
    rc = lib().orbm_debug_set_match_path(path)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_debug_set_match_path")


def set_search_buckets(mode):
    """test hook: -1 process default (ORBS_BUCKETS), 0 plain CSR scan, 1 bucketed index where it fits"""
    rc = lib().orbs_debug_set_buckets(mode)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_debug_set_buckets")


def set_search_wide_max(nproblems):
    """test hook: launches of up to `nproblems` problems take the 1024-thread (latency) form of the search kernel; -2 = process default (64), 0 = never"""
    rc = lib().orbs_debug_set_wide_max(nproblems)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_debug_set_wide_max")


def count_accepted(best, second, th=50, ratio=0.6):
    best = np.ascontiguousarray(best, dtype=np.int32)
    second = np.ascontiguousarray(second, dtype=np.int32)
    return lib().orbm_count_accepted(best.ctypes.data, second.ctypes.data, len(best), th, ratio)


def geometry(w, h, nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=FAST_SCORE, fastTh=20):
    """host-side geometry (no GPU needed): list of dicts per level, or raises OrbxError"""
    L = lib()
    p = Params()
    L.orbx_default_params(ctypes.byref(p))
    p.nfeatures, p.scale_factor, p.nlevels, p.score_type, p.fast_th = nfeatures, scaleFactor, nlevels, scoreType, fastTh
    out = np.zeros((16, 8), np.int32)
    rc = L.orbx_debug_geometry(ctypes.byref(p), w, h, out.ctypes.data, 16)
    if rc < 0:
        raise OrbxError(rc, "orbx_debug_geometry")
    keys = ("w", "h", "quota", "grid_cols", "grid_rows", "cell_w", "cell_h", "n_bands")
    return [dict(zip(keys, map(int, out[l]))) for l in range(rc)]


def variant_count(stage):
    """number of kernel variants of stage VS_* (no GPU needed)"""
    return lib().orbx_debug_variant_count(stage)


def variant_name(stage, vid):
    """the kernel with its template arguments behind variant `vid` of stage VS_*"""
    return lib().orbx_debug_variant_name(stage, vid).decode()


def plan(w, h, nframes, row_stride=None, frame_stride=None, base_bits=0, gather=False, xcd_affinity=None, on_demand=1, od_min_frames=OD_MIN_FRAMES_DEFAULT,
         stop_after=-1, color_fmt=-1, color_gather=False, color_bits=0, one_frame=False, one_frame_bytes=0, side_stream=True,
         nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=FAST_SCORE, fastTh=20, fp_contract=False):
    """orbx_debug_plan (no GPU needed): the variants a launch group of nframes w x h frames would take, a list of (id, flags, mask) per stage
    VS_*, or raises OrbxError.  Defaults: packed rows and frames, an aligned base, the affinity a handle gives a group of that size."""
    L = lib()
    p = Params()
    L.orbx_default_params(ctypes.byref(p))
    p.nfeatures, p.scale_factor, p.nlevels, p.score_type, p.fast_th, p.fp_contract = nfeatures, scaleFactor, nlevels, scoreType, fastTh, 1 if fp_contract else 0
    a = PlanArgs()
    a.w, a.h, a.nframes, a.gather = w, h, nframes, 1 if gather else 0
    a.xcd_affinity = (1 if nframes >= XCD_AFFINITY_MIN_FRAMES else 0) if xcd_affinity is None else int(xcd_affinity)
    a.on_demand, a.od_min_frames, a.stop_after = int(on_demand), od_min_frames, stop_after
    a.row_stride = w if row_stride is None else row_stride
    a.frame_stride = a.row_stride * h if frame_stride is None else frame_stride
    a.base_bits, a.color_fmt, a.color_gather, a.color_bits = base_bits, color_fmt, 1 if color_gather else 0, color_bits
    a.one_frame, a.side_stream, a.one_frame_bytes = 1 if one_frame else 0, 1 if side_stream else 0, one_frame_bytes
    out = (StageVariant * VS_COUNT)()
    rc = L.orbx_debug_plan(ctypes.byref(p), ctypes.byref(a), out)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_plan")
    return [(v.id, v.flags, v.mask) for v in out]


def nth_element_perm(resp, nth, device=0):
    """permutation produced by the device's wave-parallel std::nth_element(greater by response)"""
    r = np.ascontiguousarray(resp, dtype=np.float32)
    out = np.empty(len(r), np.int32)
    rc = lib().orbx_debug_nth_element(r.ctypes.data, len(r), nth, out.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_nth_element")
    return out


def eval_math(kind, in0, in1=None, device=0):
    in0 = np.ascontiguousarray(in0, dtype=np.float32)
    in1 = np.ascontiguousarray(in1 if in1 is not None else in0, dtype=np.float32)
    out0 = np.empty_like(in0)
    out1 = np.empty_like(in0)
    rc = lib().orbx_debug_eval_math(kind, in0.ctypes.data, in1.ctypes.data, out0.ctypes.data, out1.ctypes.data, in0.size, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_eval_math")
    return out0, out1


def eval_compass(c, e, w, n, s, t, device=0):
    """the device's FAST compass pre-test (k_fast_cells phase A1) on dword quintuples at threshold t: the flag of pixel j is bit 8 j + 7"""
    arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (c, e, w, n, s)]
    assert all(a.shape == arrs[0].shape for a in arrs)
    out = np.empty_like(arrs[0])
    rc = lib().orbx_debug_eval_compass(*[a.ctypes.data for a in arrs], out.ctypes.data, arrs[0].size, int(t), device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_eval_compass")
    return out


def eval_score(centre, ring16, tmin, device=0):
    """the FAST kernels' exact score (phase B, packed halves) and opposite-pair pre-test (phase A2) on rings: centre (n,) uint8, ring16 (n, 16)
    uint8 in ring order from (0, +3) -> (score, pair): the corner score or 0 below tmin, and 1 where the pair test passes the pixel on"""
    centre = np.ascontiguousarray(centre, dtype=np.uint8)
    ring16 = np.ascontiguousarray(ring16, dtype=np.uint8)
    assert centre.ndim == 1 and ring16.shape == (centre.size, 16)
    score = np.empty_like(centre)
    pair = np.empty_like(centre)
    rc = lib().orbx_debug_eval_score(centre.ctypes.data, ring16.ctypes.data, score.ctypes.data, pair.ctypes.data, centre.size, int(tmin), device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_eval_score")
    return score, pair


def eval_blur_window(windows, blur_rounding=BLUR_X86_SSE2, general=False, device=0):
    """k_describe_od's per-key-point blur on (n, 43, 48) uint8 windows -> the (n, 37, 40) blurred regions the taps read (window rows 3 .. 39,
    columns 4 .. 43), every column in the one rounding mode; general: through the per-lane epilogue of edge windows"""
    win = np.ascontiguousarray(windows, dtype=np.uint8)
    assert win.ndim == 3 and win.shape[1:] == (43, 48)
    out = np.empty((win.shape[0], 37, 40), np.uint8)
    rc = lib().orbx_debug_eval_blur_window(win.ctypes.data, out.ctypes.data, win.shape[0], int(blur_rounding), int(bool(general)), device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_eval_blur_window")
    return out


class ORBVocabulary:
    """Mirror of ORB_SLAM::ORBVocabulary (reference include/ORBVocabulary.h:31-32 = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>)
    for the per-frame transform: construct from a node table (`from_nodes`) or the reference's text file (`loadFromTextFile`)."""

    def __init__(self):
        self.h = ctypes.c_void_p()

    @classmethod
    def from_nodes(cls, k, L, scoring, weighting, parent, is_leaf, desc, weight, device=0):
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        is_leaf = np.ascontiguousarray(is_leaf, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        n = len(parent)
        assert len(is_leaf) == n and len(desc) == n and len(weight) == n
        v = cls()
        rc = lib().orbv_create(k, L, scoring, weighting, n, parent.ctypes.data, is_leaf.ctypes.data, desc.ctypes.data, weight.ctypes.data,
                               device, ctypes.byref(v.h))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbv_create")
        return v

    @classmethod
    def loadFromTextFile(cls, path, device=0):
        v = cls()
        rc = lib().orbv_load_text(os.fsencode(path), device, ctypes.byref(v.h))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbv_load_text")
        return v

    def close(self):
        if getattr(self, "h", None):
            lib().orbv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except TypeError:           # interpreter shutdown: module globals are already gone
            pass

    def info(self):
        vals = [ctypes.c_int() for _ in range(6)]
        lib().orbv_info(self.h, *[ctypes.byref(x) for x in vals])
        return dict(zip(("k", "L", "scoring", "weighting", "n_words", "n_nodes"), [x.value for x in vals]))

    def size(self):
        return self.info()["n_words"]

    def descend(self, desc, levelsup=4):
        """per-descriptor (word id, weight, node id at level L-levelsup)"""
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        n = len(desc)
        word = np.empty(n, np.uint32); weight = np.empty(n, np.float64); node = np.empty(n, np.uint32)
        rc = lib().orbv_descend(self.h, desc.ctypes.data, n, levelsup, word.ctypes.data, weight.ctypes.data, node.ctypes.data)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbv_descend")
        return word, weight, node

    def transform(self, desc, levelsup=4):
        """Frame::ComputeBoW: -> (bow_ids, bow_vals, fv_nodes, fv_off, fv_feat); BowVector / FeatureVector in map order"""
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        bid = np.empty(m, np.uint32); bval = np.empty(m, np.float64)
        fnode = np.empty(m, np.uint32); foff = np.zeros(m + 1, np.int32); ffeat = np.empty(m, np.uint32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        rc = lib().orbv_transform(self.h, desc.ctypes.data, n, levelsup, bid.ctypes.data, bval.ctypes.data, ctypes.byref(nb),
                                  fnode.ctypes.data, foff.ctypes.data, ffeat.ctypes.data, ctypes.byref(nf))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbv_transform")
        return bid[:nb.value], bval[:nb.value], fnode[:nf.value], foff[:nf.value + 1], ffeat[:foff[nf.value]]

    def transform_batch_device(self, d_desc, d_n, nframes, cap, levelsup, d_bow_id, d_bow_val, d_n_bow, d_fv_node, d_fv_off, d_fv_feat,
                               d_n_fv, stream=0):
        rc = lib().orbv_transform_batch_device(self.h, d_desc, d_n, nframes, cap, levelsup, d_bow_id, d_bow_val, d_n_bow, d_fv_node,
                                               d_fv_off, d_fv_feat, d_n_fv, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbv_transform_batch_device")

    def score(self, ids1, vals1, ids2, vals2):
        a = np.ascontiguousarray(ids1, dtype=np.uint32); av = np.ascontiguousarray(vals1, dtype=np.float64)
        b = np.ascontiguousarray(ids2, dtype=np.uint32); bv = np.ascontiguousarray(vals2, dtype=np.float64)
        return lib().orbv_score(self.h, a.ctypes.data, av.ctypes.data, len(a), b.ctypes.data, bv.ctypes.data, len(b))


def image_bounds(cam):
    """Frame::ComputeImageBounds + the inverse grid cell sizes (host side, once per camera)"""
    b = Bounds()
    rc = lib().orbf_image_bounds(ctypes.byref(cam), ctypes.byref(b))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbf_image_bounds")
    return b


def undistort_grid(cam, bounds, kps, device=0):
    """Frame::UndistortKeyPoints + the mGrid fill for one frame: -> (kps_un, cell_off[3073], cell_feat)"""
    kps = np.ascontiguousarray(kps, dtype=KP_DTYPE)
    n = len(kps)
    un = np.zeros(n, dtype=KP_DTYPE)
    off = np.zeros(GRID_CELLS + 1, np.int32)
    feat = np.zeros(max(n, 1), np.int32)
    rc = lib().orbf_undistort_grid(ctypes.byref(cam), ctypes.byref(bounds), kps.ctypes.data if n else None, n, un.ctypes.data if n else None,
                                   off.ctypes.data, feat.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbf_undistort_grid")
    return un, off, feat[:off[GRID_CELLS]]


def undistort_grid_batch_device(cam, bounds, d_kps, d_n, nframes, cap, d_kps_un, d_cell_off, d_cell_feat, stream=0):
    rc = lib().orbf_undistort_grid_batch_device(ctypes.byref(cam), ctypes.byref(bounds), d_kps, d_n, nframes, cap, d_kps_un, d_cell_off, d_cell_feat,
                                                stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbf_undistort_grid_batch_device")


def features_in_area(bounds, kps_un, cell_off, cell_feat, qxyr, qlev, cand_cap=None, device=0):
    """Frame::GetFeaturesInArea for many (x, y, r, minLevel, maxLevel) queries: -> (seg_off, cand) CSR"""
    kps_un = np.ascontiguousarray(kps_un, dtype=KP_DTYPE)
    cell_off = np.ascontiguousarray(cell_off, dtype=np.int32)
    cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32)
    qxyr = np.ascontiguousarray(qxyr, dtype=np.float32).reshape(-1, 3)
    qlev = np.ascontiguousarray(qlev, dtype=np.int32).reshape(-1, 2)
    nq = len(qxyr)
    assert len(qlev) == nq and len(cell_off) == GRID_CELLS + 1
    cap = cand_cap if cand_cap is not None else max(1, nq * 64)
    while True:
        seg = np.zeros(nq + 1, np.int32)
        cand = np.zeros(max(cap, 1), np.int32)
        rc = lib().orbf_features_in_area(ctypes.byref(bounds), kps_un.ctypes.data, len(kps_un), cell_off.ctypes.data, cell_feat.ctypes.data,
                                         qxyr.ctypes.data, qlev.ctypes.data, nq, seg.ctypes.data, cand.ctypes.data, cap, device)
        if rc == ORBX_ERR_CAPACITY and cand_cap is None:
            cap = int(seg[nq])
            continue
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbf_features_in_area")
        return seg, cand[:seg[nq]]


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima on bin sizes (host)"""
    sz = np.ascontiguousarray(sizes, dtype=np.int32)
    out = np.zeros(3, np.int32)
    lib().orbs_three_maxima(sz.ctypes.data, len(sz), out.ctypes.data)
    return tuple(int(v) for v in out)


def window_search_batch_device(bounds, rule, th, ratio, check_orientation, d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed,
                               d_qxyr, d_qlev, d_qdesc, d_qangle, d_qvalid, d_nq, qcap, nproblems, d_q2t, d_t2q, d_best, d_second, d_nmatches,
                               stream=0):
    """the greedy grid-window searches of ORBmatcher (include/orbs.h), device pointers as ints (0 = NULL)"""
    prm = SearchParams(rule, th, ratio, 1 if check_orientation else 0)
    rc = lib().orbs_window_search_batch_device(ctypes.byref(bounds), ctypes.byref(prm), d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap,
                                               d_claimed or None, d_qxyr, d_qlev, d_qdesc, d_qangle or None, d_qvalid or None, d_nq, qcap,
                                               nproblems, d_q2t, d_t2q, d_best or None, d_second or None, d_nmatches, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_window_search_batch_device")


def distinctive(desc, seg_off, device=0):
    """MapPoint::ComputeDistinctiveDescriptors for many map points (CSR of observed descriptors): -> (best_idx, best_median)"""
    desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
    seg = np.ascontiguousarray(seg_off, dtype=np.int32)
    M = len(seg) - 1
    idx = np.empty(max(M, 1), np.int32); med = np.empty(max(M, 1), np.int32)
    rc = lib().orbm_distinctive(desc.ctypes.data if len(desc) else None, seg.ctypes.data, M, idx.ctypes.data, med.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbm_distinctive")
    return idx[:M], med[:M]


def list_search_batch_device(rule, th, ratio, check_orientation, d_kps, d_desc, d_list, d_nlist, d_nt, cap, d_claimed, d_qrange, d_qindex, d_qdesc,
                             d_qangle, d_qvalid, d_nq, qcap, nproblems, d_q2t, d_t2q, d_best, d_second, d_nmatches, stream=0):
    """the in-order search over explicit candidate lists (SearchByBoW with the FeatureVector CSR as the list)"""
    prm = SearchParams(rule, th, ratio, 1 if check_orientation else 0)
    rc = lib().orbs_list_search_batch_device(ctypes.byref(prm), d_kps, d_desc, d_list, d_nlist, d_nt, cap, d_claimed or None, d_qrange, d_qindex or None,
                                             d_qdesc, d_qangle or None, d_qvalid or None, d_nq, qcap, nproblems, d_q2t, d_t2q, d_best or None,
                                             d_second or None, d_nmatches, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_list_search_batch_device")


def triangulation_search_batch_device(th, check_orientation, d_F12, level_sigma2, d_kps2, d_desc2, d_list, d_nlist, d_nt, cap, d_claimed, d_qrange,
                                      d_qindex, d_kps1, d_qdesc, d_qvalid, d_nq, qcap, nproblems, d_q2t, d_t2q, d_best, d_second, d_nmatches, stream=0):
    """ORBmatcher::SearchForTriangulation over FeatureVector lists (level_sigma2: host float array = mvLevelSigma2 of pKF2)"""
    prm = SearchParams(RULE_TRIANGULATION, th, 0.0, 1 if check_orientation else 0)
    s2 = np.ascontiguousarray(level_sigma2, dtype=np.float32)
    rc = lib().orbs_triangulation_search_batch_device(ctypes.byref(prm), d_F12, s2.ctypes.data, len(s2), d_kps2, d_desc2, d_list, d_nlist, d_nt, cap,
                                                      d_claimed or None, d_qrange, d_qindex or None, d_kps1, d_qdesc, d_qvalid or None, d_nq, qcap,
                                                      nproblems, d_q2t, d_t2q, d_best or None, d_second or None, d_nmatches, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_triangulation_search_batch_device")


def _level_tables(factors1, sigma2_1, factors2, sigma2_2):
    t = [np.ascontiguousarray(x, dtype=np.float32) for x in (factors1, sigma2_1, factors2, sigma2_2)]
    if len({len(x) for x in t}) != 1:
        raise ValueError("the four level tables must have one length")
    return t


def triangulate_batch_device(d_pairs, npairs, factors1, sigma2_1, factors2, sigma2_2, d_kps1, d_n1, cap1, stride1, d_kps2, d_n2, cap2, d_q2t, d_qindex,
                             d_nq, qcap, d_status, d_x3d, d_v, d_match12, d_acc_idx, d_acc_x3d, d_count, d_overflow, ocap, d_qvalid=0, d_claimed=0,
                             stream=0):
    """the match loop of LocalMapping::CreateNewMapPoints over the matches the triangulation search left on the device (include/orbt.h);
    device pointers as ints (0 = NULL), the level tables host float arrays (mvScaleFactors / mvLevelSigma2 of KF1 and KF2)"""
    f1, s1, f2, s2 = _level_tables(factors1, sigma2_1, factors2, sigma2_2)
    rc = lib().orbt_triangulate_batch_device(d_pairs, npairs, f1.ctypes.data, s1.ctypes.data, f2.ctypes.data, s2.ctypes.data, len(f1), d_kps1, d_n1, cap1,
                                             stride1, d_kps2, d_n2, cap2, d_q2t, d_qindex or None, d_nq, qcap, d_status, d_x3d, d_v or None, d_match12,
                                             d_acc_idx, d_acc_x3d, d_count, d_overflow, ocap, d_qvalid or None, d_claimed or None, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbt_triangulate_batch_device")


def triangulate(pair, factors1, sigma2_1, factors2, sigma2_2, kps1, kps2, match12, ocap=None, want_v=True, device=0):
    """one pair, host arrays, synchronous: pair = a TRI_PAIR_DTYPE record, match12 = vMatches12.
    -> (status[n1], x3d[n1, 3], v[n1, 4] or None, acc_idx[count, 2], acc_x3d[count, 3]); OrbxError(ORBX_ERR_CAPACITY) when more than ocap are accepted"""
    f1, s1, f2, s2 = _level_tables(factors1, sigma2_1, factors2, sigma2_2)
    pr = np.ascontiguousarray(pair, dtype=TRI_PAIR_DTYPE).reshape(1)
    k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE); k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
    m12 = np.ascontiguousarray(match12, dtype=np.int32)
    n1, n2 = len(k1), len(k2)
    if len(m12) != n1:
        raise ValueError("match12 must have one entry per feature of KF1")
    ocap = max(n1, 1) if ocap is None else ocap
    status = np.zeros(max(n1, 1), np.uint8); x3d = np.zeros((max(n1, 1), 3), np.float32)
    v = np.zeros((max(n1, 1), 4), np.float32) if want_v else None
    acc_idx = np.zeros((max(ocap, 1), 2), np.int32); acc_x3d = np.zeros((max(ocap, 1), 3), np.float32)
    count = ctypes.c_int(0)
    rc = lib().orbt_triangulate(pr.ctypes.data, f1.ctypes.data, s1.ctypes.data, f2.ctypes.data, s2.ctypes.data, len(f1), k1.ctypes.data if n1 else None, n1,
                                k2.ctypes.data if n2 else None, n2, m12.ctypes.data if n1 else None, status.ctypes.data, x3d.ctypes.data,
                                v.ctypes.data if want_v else None, acc_idx.ctypes.data, acc_x3d.ctypes.data, ocap, ctypes.byref(count), device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbt_triangulate (accepted: %d)" % count.value)
    return status[:n1], x3d[:n1], (v[:n1] if want_v else None), acc_idx[:count.value], acc_x3d[:count.value]


def sim3solver_bind(L):
    """the argument types of the orbh_* entry points (include/orbh.h); tools/libsim3solver_host.so exports the host forms with the same types"""
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.orbh_ransac_parameters.argtypes = [ci, cd, ci, ci, vp]
    L.orbh_max_errors.argtypes = [ci, vp, vp]
    L.orbh_hypotheses.argtypes = [vp] * 10 + [ci]
    L.orbh_select.argtypes = [vp] * 7 + [ci]
    L.orbh_iterate.argtypes = [vp] * 14 + [ci]
    L.orbh_iterate_batch.argtypes = [vp, ci] + [vp] * 13 + [ci]
    if hasattr(L, "orbh_hypotheses_batch_device"):
        L.orbh_hypotheses_batch_device.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp]
        L.orbh_select_batch_device.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    return L


def sim3solver_words(n):
    """flag words of n correspondences (ORBH_WORDS)"""
    return (int(n) + 63) // 64


def sim3solver_unpack(words, n):
    """packed flag words [..., W] -> uint8 flags [..., n] (bit i % 64 of word i // 64)"""
    w = np.ascontiguousarray(words, dtype="<u8")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n]


def sim3solver_ransac_parameters(n, probability=0.99, min_inliers=6, max_iterations=300, L=None):
    """Sim3Solver::SetRansacParameters (include/orbh.h; needs no GPU; the defaults are the reference's) -> mRansacMaxIts"""
    mx = ctypes.c_int32(0)
    rc = (L or lib()).orbh_ransac_parameters(int(n), float(probability), int(min_inliers), int(max_iterations), ctypes.addressof(mx))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_ransac_parameters")
    return mx.value


def sim3solver_max_errors(sigma2, L=None):
    """mvnMaxError1/2 as the comparisons see them: (float)(size_t)(9.210*sigma2) (include/orbh.h; needs no GPU)"""
    s2 = np.ascontiguousarray(sigma2, dtype=np.float32).reshape(-1)
    out = np.zeros(len(s2), np.float32)
    rc = (L or lib()).orbh_max_errors(len(s2), s2.ctypes.data if len(s2) else None, out.ctypes.data if len(s2) else None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_max_errors")
    return out


def sim3solver_problem(cam1, cam2, n, iters, min_inliers, max_its):
    """a SIM3SOLVER_PROBLEM_DTYPE record; cam = (fx, fy, cx, cy)"""
    q = np.zeros(1, SIM3SOLVER_PROBLEM_DTYPE)
    q["fx1"], q["fy1"], q["cx1"], q["cy1"] = cam1
    q["fx2"], q["fy2"], q["cx2"], q["cy2"] = cam2
    q["n"] = n; q["iters"] = iters; q["min_inliers"] = min_inliers; q["max_its"] = max_its
    return q[0]


def sim3solver_state(n):
    """a fresh solver state -> (SIM3SOLVER_STATE_DTYPE[1], best_flags[W])"""
    return np.zeros(1, SIM3SOLVER_STATE_DTYPE), np.zeros(sim3solver_words(n), np.uint64)


def _sim3solver_points(n, pts):
    """pts = (x3dc1[n, 3], x3dc2[n, 3], p1im1[n, 2], p2im2[n, 2], maxerr1[n], maxerr2[n]) as contiguous float arrays"""
    a = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in pts]
    if len(a) != 6 or [x.size for x in a] != [n * 3, n * 3, n * 2, n * 2, n, n]:
        raise ValueError("the arrays do not have the problem's count")
    return a


def sim3solver_point_table(pts, ncap=None):
    """the struct-of-arrays point table of one problem (include/orbh.h): float32[12, ncap]"""
    n = len(np.asarray(pts[4]).reshape(-1))
    a = _sim3solver_points(n, pts)
    t = np.zeros((SIM3SOLVER_POINT_ROWS, ncap or n), np.float32)
    t[0:3, :n] = a[0].reshape(n, 3).T; t[3:6, :n] = a[1].reshape(n, 3).T
    t[6:8, :n] = a[2].reshape(n, 2).T; t[8:10, :n] = a[3].reshape(n, 2).T
    t[10, :n] = a[4]; t[11, :n] = a[5]
    return t


def sim3solver_hypotheses(problem, pts, sets, device=0, L=None):
    """every hypothesis of one call, host arrays, synchronous -> (SIM3SOLVER_HYP_DTYPE[I], flag words uint64[I, W]) (include/orbh.h).
    L: another library with the same ABI (tools/libsim3solver_host.so)"""
    pr = np.ascontiguousarray(problem, dtype=SIM3SOLVER_PROBLEM_DTYPE).reshape(1)
    N, I = int(pr["n"][0]), int(pr["iters"][0])
    a = _sim3solver_points(N, pts)
    st = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 3)
    if len(st) != I:
        raise ValueError("one set per iteration")
    hyp = np.zeros(max(I, 1), SIM3SOLVER_HYP_DTYPE); fl = np.zeros((max(I, 1), sim3solver_words(max(N, 1))), np.uint64)
    rc = (L or lib()).orbh_hypotheses(pr.ctypes.data, *[x.ctypes.data for x in a], st.ctypes.data, hyp.ctypes.data, fl.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_hypotheses")
    return hyp[:I], fl[:I]


def _sim3solver_check_state(N, state, best_flags):
    if state.dtype != SIM3SOLVER_STATE_DTYPE or not state.flags.c_contiguous or best_flags.dtype != np.uint64 or len(best_flags) != sim3solver_words(N):
        raise ValueError("state: SIM3SOLVER_STATE_DTYPE[1]; best_flags: uint64[W]")


def sim3solver_select(problem, hyp, flags, state, best_flags, device=0, L=None):
    """the walk of Sim3Solver::iterate over the hypotheses; state (SIM3SOLVER_STATE_DTYPE[1]) and best_flags are updated in place
    -> (SIM3SOLVER_RESULT_DTYPE record, result flag words[W])"""
    pr = np.ascontiguousarray(problem, dtype=SIM3SOLVER_PROBLEM_DTYPE).reshape(1)
    N, I = int(pr["n"][0]), int(pr["iters"][0])
    _sim3solver_check_state(N, state, best_flags)
    h = np.ascontiguousarray(hyp, dtype=SIM3SOLVER_HYP_DTYPE).reshape(-1); f = np.ascontiguousarray(flags, dtype=np.uint64).reshape(-1)
    if len(h) != I or len(f) != I * sim3solver_words(N):
        raise ValueError("one hypothesis and one flag row per iteration")
    res = np.zeros(1, SIM3SOLVER_RESULT_DTYPE); rfl = np.zeros(sim3solver_words(N), np.uint64)
    rc = (L or lib()).orbh_select(pr.ctypes.data, h.ctypes.data, f.ctypes.data, state.ctypes.data, best_flags.ctypes.data, res.ctypes.data, rfl.ctypes.data,
                                  device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_select")
    return res[0], rfl


def sim3solver_iterate(problem, pts, sets, state, best_flags, want_hyp=True, device=0, L=None):
    """calls of Sim3Solver::iterate after their draw, host arrays, synchronous; state and best_flags are updated in place
    -> (SIM3SOLVER_RESULT_DTYPE record, result flag words[W], hyp[I] or None, flag words[I, W] or None)"""
    pr = np.ascontiguousarray(problem, dtype=SIM3SOLVER_PROBLEM_DTYPE).reshape(1)
    N, I = int(pr["n"][0]), int(pr["iters"][0])
    a = _sim3solver_points(N, pts)
    st = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 3)
    if len(st) != I:
        raise ValueError("one set per iteration")
    _sim3solver_check_state(N, state, best_flags)
    W = sim3solver_words(max(N, 1))
    res = np.zeros(1, SIM3SOLVER_RESULT_DTYPE); rfl = np.zeros(W, np.uint64)
    hyp = np.zeros(max(I, 1), SIM3SOLVER_HYP_DTYPE) if want_hyp else None; fl = np.zeros((max(I, 1), W), np.uint64) if want_hyp else None
    rc = (L or lib()).orbh_iterate(pr.ctypes.data, *[x.ctypes.data for x in a], st.ctypes.data, state.ctypes.data, best_flags.ctypes.data, res.ctypes.data,
                                   rfl.ctypes.data, hyp.ctypes.data if want_hyp else None, fl.ctypes.data if want_hyp else None, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_iterate")
    return res[0], rfl, (hyp[:I] if want_hyp else None), (fl[:I] if want_hyp else None)


def sim3solver_iterate_batch(problems, pts, sets, states, best_flags, want_hyp=True, device=0, L=None):
    """the same for several solvers as ONE chain with one synchronisation (what the drop-in Sim3Solver::Prefetch calls): pts and sets are lists of
    per-solver host arrays; states (SIM3SOLVER_STATE_DTYPE[P]) and the best flag words are updated in place
    -> (SIM3SOLVER_RESULT_DTYPE[P], [result flag words], [hyp] or None, [flag words] or None)"""
    pr = np.ascontiguousarray(problems, dtype=SIM3SOLVER_PROBLEM_DTYPE).reshape(-1)
    P = len(pr)
    if not (len(pts) == len(sets) == len(best_flags) == P) or states.dtype != SIM3SOLVER_STATE_DTYPE or len(states) != P or P < 1:
        raise ValueError("one entry per solver")
    arrs = [_sim3solver_points(int(pr["n"][p]), pts[p]) for p in range(P)]
    st = [np.ascontiguousarray(x, np.int32).reshape(-1, 3) for x in sets]
    for p in range(P):
        if len(st[p]) != int(pr["iters"][p]) or best_flags[p].dtype != np.uint64 or len(best_flags[p]) != sim3solver_words(pr["n"][p]):
            raise ValueError("the arrays of solver %d do not have its counts" % p)
    res = np.zeros(P, SIM3SOLVER_RESULT_DTYPE)
    out = [np.zeros(sim3solver_words(n), np.uint64) for n in pr["n"]]
    hyp = [np.zeros(int(i), SIM3SOLVER_HYP_DTYPE) for i in pr["iters"]]
    fl = [np.zeros((int(i), sim3solver_words(n)), np.uint64) for i, n in zip(pr["iters"], pr["n"])]
    ptrs = lambda xs: (ctypes.c_void_p * P)(*[x.ctypes.data for x in xs])
    keep = [ptrs([a[k] for a in arrs]) for k in range(6)] + [ptrs(st), ptrs(best_flags), ptrs(out), ptrs(hyp), ptrs(fl)]
    ad = [ctypes.addressof(k) for k in keep]
    rc = (L or lib()).orbh_iterate_batch(pr.ctypes.data, P, ad[0], ad[1], ad[2], ad[3], ad[4], ad[5], ad[6], states.ctypes.data, ad[7], res.ctypes.data, ad[8],
                                         ad[9] if want_hyp else None, ad[10] if want_hyp else None, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_iterate_batch")
    return res, out, (hyp if want_hyp else None), (fl if want_hyp else None)


def sim3solver_hypotheses_batch_device(problems, d_points, ncap, d_sets, icap, d_hyp, d_flags, stream=0):
    """the hypotheses of len(problems) calls (include/orbh.h); problems: host SIM3SOLVER_PROBLEM_DTYPE records, the rest device pointers as ints"""
    pr = np.ascontiguousarray(problems, dtype=SIM3SOLVER_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbh_hypotheses_batch_device(pr.ctypes.data, len(pr), d_points or None, ncap, d_sets or None, icap, d_hyp or None, d_flags or None,
                                            stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_hypotheses_batch_device")


def sim3solver_select_batch_device(problems, ncap, icap, d_hyp, d_flags, d_state, d_best_flags, d_result, d_result_flags, stream=0):
    """the walk of Sim3Solver::iterate for len(problems) solvers; their states and best flags are updated on the device (include/orbh.h)"""
    pr = np.ascontiguousarray(problems, dtype=SIM3SOLVER_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbh_select_batch_device(pr.ctypes.data, len(pr), ncap, icap, d_hyp or None, d_flags or None, d_state or None, d_best_flags or None,
                                        d_result or None, d_result_flags or None, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbh_select_batch_device")


def poseopt_bind(L):
    """the argument types of the orbo_* entry points (include/orbo.h); tools/libposeopt_host.so exports the host forms with the same types"""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbo_pose.argtypes = [vp] * 8 + [ci]
    L.orbo_pose_batch.argtypes = [vp, ci] + [vp] * 7 + [ci]
    if hasattr(L, "orbo_pose_batch_device"):
        L.orbo_pose_batch_device.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp]
    return L


def poseopt_problem(cam, n):
    """one orbo_problem record: cam = (fx, fy, cx, cy), n edges"""
    q = np.zeros((), POSEOPT_PROBLEM_DTYPE)
    q["fx"], q["fy"], q["cx"], q["cy"] = cam
    q["n"] = n
    return q


def poseopt_edge_table(xyz, uv, inv_sigma2, ncap=None):
    """a frame's edges as the device table: ORBO_EDGE_ROWS rows of ncap floats (include/orbo.h)"""
    n = len(inv_sigma2)
    ncap = max(n, 1) if ncap is None else ncap
    t = np.zeros((POSEOPT_EDGE_ROWS, ncap), np.float32)
    if n:
        t[0:3, :n] = np.asarray(xyz, np.float32).reshape(n, 3).T
        t[3:5, :n] = np.asarray(uv, np.float32).reshape(n, 2).T
        t[5, :n] = inv_sigma2
    return t


def _poseopt_arrays(n, xyz, uv, inv_sigma2, Tcw):
    a = (np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), np.ascontiguousarray(uv, np.float32).reshape(-1, 2),
         np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1))
    if not all(len(x) == n for x in a):
        raise ValueError("the edge arrays do not have the problem's n")
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12] if np.size(Tcw) == 16 else Tcw, np.float32).reshape(12)
    return a, T


def poseopt_pose(problem, xyz, uv, inv_sigma2, Tcw, want_trace=False, device=0, L=None):
    """Optimizer::PoseOptimization for one frame, host arrays, synchronous (include/orbo.h): Tcw is the 3 x 4 [R | t] (or the 4 x 4 matrix)
    -> (POSEOPT_RESULT_DTYPE record, outlier flags uint8[n], POSEOPT_STEP_DTYPE[32] or None)"""
    pr = np.ascontiguousarray(problem, dtype=POSEOPT_PROBLEM_DTYPE).reshape(1)
    n = int(pr["n"][0])
    a, T = _poseopt_arrays(n, xyz, uv, inv_sigma2, Tcw)
    res = np.zeros(1, POSEOPT_RESULT_DTYPE); words = np.zeros(max(sim3solver_words(n), 1), np.uint64)
    tr = np.zeros(POSEOPT_MAX_ITERS, POSEOPT_STEP_DTYPE) if want_trace else None
    rc = (L or lib()).orbo_pose(pr.ctypes.data, *[x.ctypes.data if n else None for x in a], T.ctypes.data, res.ctypes.data, words.ctypes.data if n else None,
                                tr.ctypes.data if want_trace else None, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbo_pose")
    return res[0], sim3solver_unpack(words, n), tr


def poseopt_pose_batch(problems, xyz, uv, inv_sigma2, Tcw, want_trace=False, device=0, L=None):
    """the same for several frames as ONE launch with one synchronisation (the relocaliser's candidates): xyz, uv, inv_sigma2 are lists of per-frame
    host arrays, Tcw is [P, 12] -> (POSEOPT_RESULT_DTYPE[P], [outlier flags uint8[n]], [POSEOPT_STEP_DTYPE[32]] or None)"""
    pr = np.ascontiguousarray(problems, dtype=POSEOPT_PROBLEM_DTYPE).reshape(-1)
    P = len(pr)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(P, 12)
    if not (len(xyz) == len(uv) == len(inv_sigma2) == P) or P < 1:
        raise ValueError("one entry per frame")
    arrs = [_poseopt_arrays(int(pr["n"][p]), xyz[p], uv[p], inv_sigma2[p], T[p])[0] for p in range(P)]
    res = np.zeros(P, POSEOPT_RESULT_DTYPE)
    words = [np.zeros(max(sim3solver_words(n), 1), np.uint64) for n in pr["n"]]
    tr = [np.zeros(POSEOPT_MAX_ITERS, POSEOPT_STEP_DTYPE) for _ in range(P)]
    ptrs = lambda xs, ns: (ctypes.c_void_p * P)(*[x.ctypes.data if n else None for x, n in zip(xs, ns)])
    keep = [ptrs([a[k] for a in arrs], pr["n"]) for k in range(3)] + [ptrs(words, pr["n"]), ptrs(tr, [1] * P)]
    ad = [ctypes.addressof(k) for k in keep]
    rc = (L or lib()).orbo_pose_batch(pr.ctypes.data, P, ad[0], ad[1], ad[2], T.ctypes.data, res.ctypes.data, ad[3], ad[4] if want_trace else None, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbo_pose_batch")
    return res, [sim3solver_unpack(w, int(n)) for w, n in zip(words, pr["n"])], (tr if want_trace else None)


def poseopt_pose_batch_device(problems, d_edges, ncap, d_Tcw, d_result, d_outlier, d_trace=0, stream=0):
    """the poses of len(problems) frames (include/orbo.h); problems: host POSEOPT_PROBLEM_DTYPE records, the rest device pointers as ints"""
    pr = np.ascontiguousarray(problems, dtype=POSEOPT_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbo_pose_batch_device(pr.ctypes.data, len(pr), d_edges or None, ncap, d_Tcw or None, d_result or None, d_outlier or None, d_trace or None,
                                      stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbo_pose_batch_device")


def sim3opt_bind(L):
    """the argument types of the orbg_* entry points (include/orbg.h); tools/libsim3opt_host.so exports the host forms with the same types"""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.orbg_sim3.argtypes = [vp] * 9 + [ci]
    L.orbg_sim3_batch.argtypes = [vp, ci] + [vp] * 8 + [ci]
    if hasattr(L, "orbg_sim3_batch_device"):
        L.orbg_sim3_batch_device.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp]
    return L


def sim3opt_problem(cam1, cam2, th2, n):
    """one orbg_problem record: cam1, cam2 = (fx, fy, cx, cy) of K1 and K2, the argument th2, n pairs"""
    q = np.zeros((), SIM3OPT_PROBLEM_DTYPE)
    q["fx1"], q["fy1"], q["cx1"], q["cy1"] = cam1
    q["fx2"], q["fy2"], q["cx2"], q["cy2"] = cam2
    q["th2"] = th2
    q["n"] = n
    return q


def sim3opt_start(R, t, s):
    """the thirteen floats of a start similarity: R row major, t, s (the arguments of g2o::Sim3(R, t, s), LoopClosing.cc:320)"""
    return np.concatenate([np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3), np.asarray([s], np.float32)])


def sim3opt_pair_table(P1c, P2c, obs1, obs2, ncap=None):
    """a candidate's pairs as the device table: ORBG_PAIR_ROWS rows of ncap floats (include/orbg.h)"""
    a = _sim3opt_arrays(None, P1c, P2c, obs1, obs2)
    n = len(a[0])
    ncap = max(n, 1) if ncap is None else ncap
    t = np.zeros((SIM3OPT_PAIR_ROWS, ncap), np.float32)
    for k in range(4):
        t[3 * k:3 * k + 3, :n] = a[k].T
    return t


def _sim3opt_arrays(n, P1c, P2c, obs1, obs2):
    a = tuple(np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (P1c, P2c, obs1, obs2))
    if not all(len(x) == (len(a[0]) if n is None else n) for x in a):
        raise ValueError("the pair arrays do not have the problem's n")
    return a


def sim3opt_sim3(problem, P1c, P2c, obs1, obs2, S12, want_trace=False, device=0, L=None):
    """Optimizer::OptimizeSim3 for one loop candidate, host arrays, synchronous (include/orbg.h): P1c, P2c are [n, 3], obs1 = (u1, v1, w1) and
    obs2 = (u2, v2, w2) are [n, 3], S12 the thirteen floats of sim3opt_start
    -> (SIM3OPT_RESULT_DTYPE record, removed flags uint8[n], POSEOPT_STEP_DTYPE[15] or None)"""
    pr = np.ascontiguousarray(problem, dtype=SIM3OPT_PROBLEM_DTYPE).reshape(1)
    n = int(pr["n"][0])
    a = _sim3opt_arrays(n, P1c, P2c, obs1, obs2)
    S = np.ascontiguousarray(S12, np.float32).reshape(13)
    res = np.zeros(1, SIM3OPT_RESULT_DTYPE); words = np.zeros(max(sim3solver_words(n), 1), np.uint64)
    tr = np.zeros(SIM3OPT_MAX_ITERS, POSEOPT_STEP_DTYPE) if want_trace else None
    rc = (L or lib()).orbg_sim3(pr.ctypes.data, *[x.ctypes.data if n else None for x in a], S.ctypes.data, res.ctypes.data,
                                words.ctypes.data if n else None, tr.ctypes.data if want_trace else None, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbg_sim3")
    return res[0], sim3solver_unpack(words, n), tr


def sim3opt_sim3_batch(problems, P1c, P2c, obs1, obs2, S12, want_trace=False, device=0, L=None):
    """the same for several candidates as ONE launch with one synchronisation: P1c, P2c, obs1, obs2 are lists of per-candidate host arrays, S12 is
    [P, 13] -> (SIM3OPT_RESULT_DTYPE[P], [removed flags uint8[n]], [POSEOPT_STEP_DTYPE[15]] or None)"""
    pr = np.ascontiguousarray(problems, dtype=SIM3OPT_PROBLEM_DTYPE).reshape(-1)
    P = len(pr)
    S = np.ascontiguousarray(S12, np.float32).reshape(P, 13)
    if not (len(P1c) == len(P2c) == len(obs1) == len(obs2) == P) or P < 1:
        raise ValueError("one entry per candidate")
    arrs = [_sim3opt_arrays(int(pr["n"][p]), P1c[p], P2c[p], obs1[p], obs2[p]) for p in range(P)]
    res = np.zeros(P, SIM3OPT_RESULT_DTYPE)
    words = [np.zeros(max(sim3solver_words(n), 1), np.uint64) for n in pr["n"]]
    tr = [np.zeros(SIM3OPT_MAX_ITERS, POSEOPT_STEP_DTYPE) for _ in range(P)]
    ptrs = lambda xs, ns: (ctypes.c_void_p * P)(*[x.ctypes.data if n else None for x, n in zip(xs, ns)])
    keep = [ptrs([a[k] for a in arrs], pr["n"]) for k in range(4)] + [ptrs(words, pr["n"]), ptrs(tr, [1] * P)]
    ad = [ctypes.addressof(k) for k in keep]
    rc = (L or lib()).orbg_sim3_batch(pr.ctypes.data, P, ad[0], ad[1], ad[2], ad[3], S.ctypes.data, res.ctypes.data, ad[4], ad[5] if want_trace else None,
                                      device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbg_sim3_batch")
    return res, [sim3solver_unpack(w, int(n)) for w, n in zip(words, pr["n"])], (tr if want_trace else None)


def sim3opt_sim3_batch_device(problems, d_pairs, ncap, d_S12, d_result, d_removed, d_trace=0, stream=0):
    """the similarities of len(problems) candidates (include/orbg.h); problems: host SIM3OPT_PROBLEM_DTYPE records, the rest device pointers as ints"""
    pr = np.ascontiguousarray(problems, dtype=SIM3OPT_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbg_sim3_batch_device(pr.ctypes.data, len(pr), d_pairs or None, ncap, d_S12 or None, d_result or None, d_removed or None, d_trace or None,
                                      stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbg_sim3_batch_device")


def localba_bind(L):
    """the argument types of the orbb_* entry points (include/orbb.h); tools/liblocalba_host.so exports the host forms with the same types"""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.orbb_state_from_float.argtypes = [vp] * 5
    L.orbb_state_to_float.argtypes = [vp] * 5
    L.orbb_work_bytes.argtypes = [vp]
    L.orbb_work_bytes.restype = ctypes.c_size_t
    L.orbb_optimize.argtypes = [vp] * 6 + [cf] + [vp] * 4 + [ci] + [vp] * 4 + [ci]
    if hasattr(L, "orbb_optimize_device"):
        L.orbb_optimize_device.argtypes = [vp] * 6 + [cf] + [vp] * 4 + [ci, vp, ctypes.c_size_t] + [vp] * 5
    return L


LOCALBA_HUBER_DELTA = float(np.float32(np.sqrt(5.991)))        # `const float thHuber = sqrt(5.991)` of both callers


def ba_problem(nfree, nfixed, npoints, nedges):
    """one orbb_problem record"""
    q = np.zeros((), LOCALBA_PROBLEM_DTYPE)
    q["nfree"], q["nfixed"], q["npoints"], q["nedges"] = nfree, nfixed, npoints, nedges
    return q


def ba_dump_fields(nfree, npoints):
    """the arrays of the first-build dump in order: (name, shape)"""
    n = 6 * nfree
    return [("Hpp", (nfree, 28)), ("Hll", (npoints, 6)), ("bl", (npoints, 3)), ("S", (n, n)), ("bs", (n,)), ("xp", (n,)), ("xl", (npoints, 3))]


def ba_work_bytes(problem, L=None):
    pr = np.ascontiguousarray(problem, dtype=LOCALBA_PROBLEM_DTYPE).reshape(1)
    return int((L or lib()).orbb_work_bytes(pr.ctypes.data))


def ba_state_from_float(problem, Tcw, world, L=None):
    """Converter::toSE3Quat of every pose ([np, 3 x 4] or [np, 4 x 4] float rows of [R | t]) and the float world positions widened
    -> (pose_qt float64[np, 7], point_xyz float64[npoints, 3])"""
    pr = np.ascontiguousarray(problem, dtype=LOCALBA_PROBLEM_DTYPE).reshape(1)
    npo, P = int(pr["nfree"][0] + pr["nfixed"][0]), int(pr["npoints"][0])
    T = np.asarray(Tcw, np.float32).reshape(npo, -1)
    T = np.ascontiguousarray(T[:, :12])
    X = np.ascontiguousarray(world, np.float32).reshape(P, 3)
    q, x = np.zeros((npo, 7)), np.zeros((P, 3))
    rc = (L or lib()).orbb_state_from_float(pr.ctypes.data, T.ctypes.data, X.ctypes.data if P else None, q.ctypes.data, x.ctypes.data if P else None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbb_state_from_float")
    return q, x


def ba_state_to_float(problem, pose_qt, point_xyz, L=None):
    """what SetPose(Converter::toCvMat(SE3quat)) and SetWorldPos store -> (Tcw float32[np, 4, 4], world float32[npoints, 3])"""
    pr = np.ascontiguousarray(problem, dtype=LOCALBA_PROBLEM_DTYPE).reshape(1)
    npo, P = int(pr["nfree"][0] + pr["nfixed"][0]), int(pr["npoints"][0])
    q = np.ascontiguousarray(pose_qt, np.float64).reshape(npo, 7)
    x = np.ascontiguousarray(point_xyz, np.float64).reshape(P, 3)
    T, X = np.zeros((npo, 4, 4), np.float32), np.zeros((P, 3), np.float32)
    rc = (L or lib()).orbb_state_to_float(pr.ctypes.data, q.ctypes.data, x.ctypes.data if P else None, T.ctypes.data, X.ctypes.data if P else None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbb_state_to_float")
    return T, X


def ba_pack_bits(bits):
    """edge bits (bool[nedges]) as the words of include/orbb.h: bit e % 64 of word e / 64"""
    b = np.asarray(bits, bool).reshape(-1)
    pad = np.zeros(max(sim3solver_words(len(b)), 1) * 64, np.uint8)
    pad[:len(b)] = b
    return np.packbits(pad, bitorder="little").view("<u8").astype(np.uint64)


def ba_optimize(problem, cam, point_first, edge_pose, edge_uv, edge_inv_sigma2, pose_qt, point_xyz, active, chi2, iters, huber_delta=LOCALBA_HUBER_DELTA,
                want_trace=False, want_dump=False, device=0, L=None):
    """g2o's optimize(iters) over host arrays, synchronous (include/orbb.h).  active: bool[nedges]; chi2: float64[nedges] or None (zeros).  The state
    arrays are not modified -> dict(result, pose_qt, point_xyz, chi2, flags uint8[nedges], trace POSEOPT_STEP_DTYPE[64] or None, dump dict or None)"""
    pr = np.ascontiguousarray(problem, dtype=LOCALBA_PROBLEM_DTYPE).reshape(1)
    nf, npo, P, E = int(pr["nfree"][0]), int(pr["nfree"][0] + pr["nfixed"][0]), int(pr["npoints"][0]), int(pr["nedges"][0])
    cam = np.ascontiguousarray(cam, np.float32).reshape(npo, 4)
    first = np.ascontiguousarray(point_first, np.int32).reshape(P + 1)
    ep = np.ascontiguousarray(edge_pose, np.int32).reshape(E)
    uv = np.ascontiguousarray(edge_uv, np.float32).reshape(E, 2)
    w = np.ascontiguousarray(edge_inv_sigma2, np.float32).reshape(E)
    q = np.array(pose_qt, np.float64).reshape(npo, 7).copy()
    x = np.array(point_xyz, np.float64).reshape(P, 3).copy()
    act = ba_pack_bits(np.asarray(active, bool).reshape(E))
    c2 = np.zeros(E) if chi2 is None else np.array(chi2, np.float64).reshape(E).copy()
    res = np.zeros(1, LOCALBA_RESULT_DTYPE)
    fl = np.zeros(max(sim3solver_words(E), 1), np.uint64)
    tr = np.zeros(LOCALBA_MAX_ITERS, POSEOPT_STEP_DTYPE) if want_trace else None
    dump = np.zeros(nf * 28 + P * 12 + 36 * nf * nf + 12 * nf) if want_dump else None
    ptr = lambda a, n=1: a.ctypes.data if (a is not None and n) else None
    rc = (L or lib()).orbb_optimize(pr.ctypes.data, cam.ctypes.data, first.ctypes.data, ptr(ep, E), ptr(uv, E), ptr(w, E), huber_delta, q.ctypes.data, ptr(x, P),
                                    ptr(act, E), ptr(c2, E), iters, res.ctypes.data, ptr(fl, E), ptr(tr), ptr(dump), device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbb_optimize")
    d = None
    if want_dump:
        d, at = {}, 0
        for name, shape in ba_dump_fields(nf, P):
            k = int(np.prod(shape))
            d[name] = dump[at:at + k].reshape(shape)
            at += k
    return dict(result=res[0], pose_qt=q, point_xyz=x, chi2=c2, flags=sim3solver_unpack(fl, E), trace=tr, dump=d)


def ba_optimize_device(problem, d_cam, d_point_first, d_edge_pose, d_edge_uv, d_edge_inv_sigma2, d_pose_qt, d_point_xyz, d_active, d_chi2, iters, d_work,
                       work_bytes, d_flags, d_trace=0, d_dump=0, huber_delta=LOCALBA_HUBER_DELTA, stream=0):
    """the same over device pointers (ints); allocates nothing and returns, synchronised, the LOCALBA_RESULT_DTYPE record"""
    pr = np.ascontiguousarray(problem, dtype=LOCALBA_PROBLEM_DTYPE).reshape(1)
    res = np.zeros(1, LOCALBA_RESULT_DTYPE)
    rc = lib().orbb_optimize_device(pr.ctypes.data, d_cam or None, d_point_first or None, d_edge_pose or None, d_edge_uv or None, d_edge_inv_sigma2 or None,
                                    huber_delta, d_pose_qt or None, d_point_xyz or None, d_active or None, d_chi2 or None, iters, d_work or None, work_bytes,
                                    res.ctypes.data, d_flags or None, d_trace or None, d_dump or None, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbb_optimize_device")
    return res[0]


def pnp_bind(L):
    """the argument types of the orbe_* entry points (include/orbe.h); tools/libpnp_host.so exports the host forms with the same types"""
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    L.orbe_ransac_parameters.argtypes = [ci, cd, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp]
    L.orbe_hypotheses.argtypes = [vp] * 12 + [ci]
    L.orbe_refine.argtypes = [vp] * 6 + [ci] + [vp] * 5 + [ci]
    L.orbe_refit.argtypes = [vp] * 11 + [ci]
    L.orbe_select.argtypes = [vp] * 15 + [ci]
    L.orbe_iterate.argtypes = [vp] * 10 + [ci]
    L.orbe_iterate_batch.argtypes = [vp, ci] + [vp] * 9 + [ci]
    if hasattr(L, "orbe_hypotheses_batch_device"):
        L.orbe_hypotheses_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbe_refine_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbe_refit_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbe_select_batch_device.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return L


def pnp_ransac_parameters(sigma2, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991, L=None):
    """PnPsolver::SetRansacParameters (include/orbe.h; needs no GPU; the defaults are the reference's) -> (min_inliers, max_its, epsilon, maxerr[N])"""
    s2 = np.ascontiguousarray(sigma2, dtype=np.float32).reshape(-1)
    mi, mx = ctypes.c_int32(0), ctypes.c_int32(0)
    eps = ctypes.c_float(0)
    maxerr = np.zeros(max(len(s2), 1), np.float32)
    rc = (L or lib()).orbe_ransac_parameters(len(s2), float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), float(th2),
                                             s2.ctypes.data if len(s2) else None, ctypes.addressof(mi), ctypes.addressof(mx), ctypes.addressof(eps),
                                             maxerr.ctypes.data)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_ransac_parameters")
    return mi.value, mx.value, np.float32(eps.value), maxerr[:len(s2)]


def pnp_problem(fu, fv, uc, vc, n, iters, min_inliers, max_its):
    """a PNP_PROBLEM_DTYPE record"""
    q = np.zeros(1, PNP_PROBLEM_DTYPE)
    q["fu"] = fu; q["fv"] = fv; q["uc"] = uc; q["vc"] = vc
    q["n"] = n; q["iters"] = iters; q["min_inliers"] = min_inliers; q["max_its"] = max_its
    return q[0]


def pnp_state(n):
    """a fresh solver state -> (PNP_STATE_DTYPE[1], best_flags[n], refined_flags[n])"""
    return np.zeros(1, PNP_STATE_DTYPE), np.zeros(n, np.uint8), np.zeros(n, np.uint8)


def _pnp_points(pr, p3d, p2d, maxerr):
    N = int(pr["n"][0])
    a3 = np.ascontiguousarray(p3d, dtype=np.float32).reshape(-1, 3); a2 = np.ascontiguousarray(p2d, dtype=np.float32).reshape(-1, 2)
    am = np.ascontiguousarray(maxerr, dtype=np.float32).reshape(-1)
    if not len(a3) == len(a2) == len(am) == N:
        raise ValueError("the arrays do not have the problem's count")
    return N, a3, a2, am


def pnp_hypotheses(problem, p3d, p2d, maxerr, sets, want_vecs=True, device=0, L=None):
    """every hypothesis of one call, host arrays, synchronous -> dict(R[I, 9], t[I, 3], err[I, 3], branch[I], vecs[I, 4, 12] or None, count[I],
    flags[I, N]) (include/orbe.h).  L: another library with the same ABI (tools/libpnp_host.so)"""
    pr = np.ascontiguousarray(problem, dtype=PNP_PROBLEM_DTYPE).reshape(1)
    N, a3, a2, am = _pnp_points(pr, p3d, p2d, maxerr)
    st = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
    I = int(pr["iters"][0])
    if len(st) != I:
        raise ValueError("one set per iteration")
    o = dict(R=np.zeros((I, 9)), t=np.zeros((I, 3)), err=np.zeros((I, 3)), branch=np.zeros(I, np.int32), vecs=np.zeros((I, 4, 12)) if want_vecs else None,
             count=np.zeros(I, np.int32), flags=np.zeros((I, N), np.uint8))
    rc = (L or lib()).orbe_hypotheses(pr.ctypes.data, a3.ctypes.data, a2.ctypes.data, am.ctypes.data, st.ctypes.data, o["R"].ctypes.data, o["t"].ctypes.data,
                                      o["err"].ctypes.data, o["branch"].ctypes.data, o["vecs"].ctypes.data if want_vecs else None, o["count"].ctypes.data,
                                      o["flags"].ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_hypotheses")
    return o


def pnp_refine(problem, p3d, p2d, maxerr, count, flags, best_in=0, poison=None, device=0, L=None):
    """Refine of every record of one call, host arrays, synchronous -> dict(R[I, 9], t[I, 3], count[I], flags[I, N], ok[I]); what is not a record keeps
    the value `poison` = (double, int32, uint8) the arrays start with (default NaN, -1, 255)"""
    pr = np.ascontiguousarray(problem, dtype=PNP_PROBLEM_DTYPE).reshape(1)
    N, a3, a2, am = _pnp_points(pr, p3d, p2d, maxerr)
    I = int(pr["iters"][0])
    cn = np.ascontiguousarray(count, dtype=np.int32).reshape(-1); fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1, N)
    if len(cn) != I or len(fl) != I:
        raise ValueError("one count and one flag array per iteration")
    pd, pi, pb = poison or (np.nan, -1, 255)
    o = dict(R=np.full((I, 9), pd), t=np.full((I, 3), pd), count=np.full(I, pi, np.int32), flags=np.full((I, N), pb, np.uint8), ok=np.full(I, pi, np.int32))
    rc = (L or lib()).orbe_refine(pr.ctypes.data, a3.ctypes.data, a2.ctypes.data, am.ctypes.data, cn.ctypes.data, fl.ctypes.data, int(best_in),
                                  o["R"].ctypes.data, o["t"].ctypes.data, o["count"].ctypes.data, o["flags"].ctypes.data, o["ok"].ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_refine")
    return o


def pnp_refit(problem, p3d, p2d, maxerr, flags_in, want_vecs=True, device=0, L=None):
    """the n-point fit over planted flag arrays (problem.iters of them), host arrays, synchronous -> dict(R, t, vecs or None, count, flags, ok)"""
    pr = np.ascontiguousarray(problem, dtype=PNP_PROBLEM_DTYPE).reshape(1)
    N, a3, a2, am = _pnp_points(pr, p3d, p2d, maxerr)
    I = int(pr["iters"][0])
    fi = np.ascontiguousarray(flags_in, dtype=np.uint8).reshape(-1, N)
    if len(fi) != I:
        raise ValueError("one flag array per slot")
    o = dict(R=np.zeros((I, 9)), t=np.zeros((I, 3)), vecs=np.zeros((I, 4, 12)) if want_vecs else None, count=np.zeros(I, np.int32),
             flags=np.zeros((I, N), np.uint8), ok=np.zeros(I, np.int32))
    rc = (L or lib()).orbe_refit(pr.ctypes.data, a3.ctypes.data, a2.ctypes.data, am.ctypes.data, fi.ctypes.data, o["R"].ctypes.data, o["t"].ctypes.data,
                                 o["vecs"].ctypes.data if want_vecs else None, o["count"].ctypes.data, o["flags"].ctypes.data, o["ok"].ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_refit")
    return o


def pnp_select(problem, hyp, ref, state, best_flags, refined_flags, device=0, L=None):
    """the walk of PnPsolver::iterate over hyp (of pnp_hypotheses) and ref (of pnp_refine); state (PNP_STATE_DTYPE[1]), best_flags and refined_flags are
    updated in place -> (PNP_RESULT_DTYPE record, result_flags[N])"""
    pr = np.ascontiguousarray(problem, dtype=PNP_PROBLEM_DTYPE).reshape(1)
    N = int(pr["n"][0])
    if state.dtype != PNP_STATE_DTYPE or not state.flags.c_contiguous or best_flags.dtype != np.uint8 or refined_flags.dtype != np.uint8 or \
            len(best_flags) != N or len(refined_flags) != N:
        raise ValueError("state: PNP_STATE_DTYPE[1]; best_flags, refined_flags: uint8[N]")
    res = np.zeros(1, PNP_RESULT_DTYPE); rfl = np.zeros(N, np.uint8)
    a = [np.ascontiguousarray(hyp["R"], np.float64), np.ascontiguousarray(hyp["t"], np.float64), np.ascontiguousarray(hyp["count"], np.int32),
         np.ascontiguousarray(hyp["flags"], np.uint8), np.ascontiguousarray(ref["R"], np.float64), np.ascontiguousarray(ref["t"], np.float64),
         np.ascontiguousarray(ref["count"], np.int32), np.ascontiguousarray(ref["flags"], np.uint8), np.ascontiguousarray(ref["ok"], np.int32)]
    rc = (L or lib()).orbe_select(pr.ctypes.data, *[x.ctypes.data for x in a], state.ctypes.data, best_flags.ctypes.data, refined_flags.ctypes.data,
                                  res.ctypes.data, rfl.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_select")
    return res[0], rfl


def pnp_iterate(problem, p3d, p2d, maxerr, sets, state, best_flags, refined_flags, device=0, L=None):
    """one call of PnPsolver::iterate after its draw, host arrays, synchronous; state, best_flags, refined_flags are updated in place
    -> (PNP_RESULT_DTYPE record, result_flags[N])"""
    pr = np.ascontiguousarray(problem, dtype=PNP_PROBLEM_DTYPE).reshape(1)
    N, a3, a2, am = _pnp_points(pr, p3d, p2d, maxerr)
    st = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
    if len(st) != int(pr["iters"][0]):
        raise ValueError("one set per iteration")
    if state.dtype != PNP_STATE_DTYPE or not state.flags.c_contiguous or best_flags.dtype != np.uint8 or refined_flags.dtype != np.uint8 or \
            len(best_flags) != N or len(refined_flags) != N:
        raise ValueError("state: PNP_STATE_DTYPE[1]; best_flags, refined_flags: uint8[N]")
    res = np.zeros(1, PNP_RESULT_DTYPE); rfl = np.zeros(N, np.uint8)
    rc = (L or lib()).orbe_iterate(pr.ctypes.data, a3.ctypes.data, a2.ctypes.data, am.ctypes.data, st.ctypes.data, state.ctypes.data, best_flags.ctypes.data,
                                   refined_flags.ctypes.data, res.ctypes.data, rfl.ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_iterate")
    return res[0], rfl


def pnp_iterate_batch(problems, p3d, p2d, maxerr, sets, states, best_flags, refined_flags, device=0, L=None):
    """the next iterate() of several solvers as ONE chain with one synchronisation (what the drop-in PnPsolver::Prefetch calls): lists of per-solver
    host arrays; states (PNP_STATE_DTYPE[P]) and the flag arrays are updated in place -> (PNP_RESULT_DTYPE[P], [result_flags])"""
    pr = np.ascontiguousarray(problems, dtype=PNP_PROBLEM_DTYPE).reshape(-1)
    P = len(pr)
    a3 = [np.ascontiguousarray(x, np.float32) for x in p3d]; a2 = [np.ascontiguousarray(x, np.float32) for x in p2d]
    am = [np.ascontiguousarray(x, np.float32) for x in maxerr]; st = [np.ascontiguousarray(x, np.int32) for x in sets]
    if not (len(a3) == len(a2) == len(am) == len(st) == len(best_flags) == len(refined_flags) == P) or states.dtype != PNP_STATE_DTYPE or len(states) != P:
        raise ValueError("one entry per solver")
    for p in range(P):
        n, it = int(pr["n"][p]), int(pr["iters"][p])
        if a3[p].size != n * 3 or a2[p].size != n * 2 or am[p].size != n or st[p].size != it * 4 or best_flags[p].dtype != np.uint8 or \
                refined_flags[p].dtype != np.uint8 or len(best_flags[p]) != n or len(refined_flags[p]) != n:
            raise ValueError("the arrays of solver %d do not have its counts" % p)
    res = np.zeros(P, PNP_RESULT_DTYPE)
    out = [np.zeros(int(n), np.uint8) for n in pr["n"]]
    ptrs = lambda arrs: (ctypes.c_void_p * P)(*[x.ctypes.data for x in arrs])
    keep = [ptrs(a3), ptrs(a2), ptrs(am), ptrs(st), ptrs(best_flags), ptrs(refined_flags), ptrs(out)]
    rc = (L or lib()).orbe_iterate_batch(pr.ctypes.data, P, ctypes.addressof(keep[0]), ctypes.addressof(keep[1]), ctypes.addressof(keep[2]),
                                         ctypes.addressof(keep[3]), states.ctypes.data, ctypes.addressof(keep[4]), ctypes.addressof(keep[5]), res.ctypes.data,
                                         ctypes.addressof(keep[6]), device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_iterate_batch")
    return res, out


def pnp_hypotheses_batch_device(problems, d_p3d, d_p2d, d_maxerr, ncap, d_sets, icap, d_R, d_t, d_err, d_branch, d_vecs, d_count, d_flags, stream=0):
    """the hypotheses of len(problems) calls (include/orbe.h); problems: host PNP_PROBLEM_DTYPE records, the rest device pointers as ints (0 = NULL)"""
    pr = np.ascontiguousarray(problems, dtype=PNP_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbe_hypotheses_batch_device(pr.ctypes.data, len(pr), d_p3d, d_p2d, d_maxerr, ncap, d_sets, icap, d_R, d_t, d_err, d_branch, d_vecs or None,
                                            d_count, d_flags, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_hypotheses_batch_device")


def pnp_refine_batch_device(problems, d_p3d, d_p2d, d_maxerr, ncap, icap, d_count, d_flags, d_state, d_rR, d_rt, d_rcount, d_rflags, d_rok, stream=0):
    """Refine of every record of len(problems) calls (include/orbe.h)"""
    pr = np.ascontiguousarray(problems, dtype=PNP_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbe_refine_batch_device(pr.ctypes.data, len(pr), d_p3d, d_p2d, d_maxerr, ncap, icap, d_count, d_flags, d_state, d_rR, d_rt, d_rcount, d_rflags,
                                        d_rok, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_refine_batch_device")


def pnp_refit_batch_device(problems, d_p3d, d_p2d, d_maxerr, ncap, icap, d_flags_in, d_rR, d_rt, d_rvecs, d_rcount, d_rflags, d_rok, stream=0):
    """the n-point fit over planted flag arrays of len(problems) problems (include/orbe.h)"""
    pr = np.ascontiguousarray(problems, dtype=PNP_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbe_refit_batch_device(pr.ctypes.data, len(pr), d_p3d, d_p2d, d_maxerr, ncap, icap, d_flags_in, d_rR, d_rt, d_rvecs or None, d_rcount, d_rflags,
                                       d_rok, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_refit_batch_device")


def pnp_select_batch_device(problems, ncap, icap, d_R, d_t, d_count, d_flags, d_rR, d_rt, d_rcount, d_rflags, d_rok, d_state, d_best_flags, d_refined_flags,
                            d_result, d_result_flags, stream=0):
    """the walk of PnPsolver::iterate for len(problems) solvers; their states and flag arrays are updated on the device (include/orbe.h)"""
    pr = np.ascontiguousarray(problems, dtype=PNP_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbe_select_batch_device(pr.ctypes.data, len(pr), ncap, icap, d_R, d_t, d_count, d_flags, d_rR, d_rt, d_rcount, d_rflags, d_rok, d_state,
                                        d_best_flags, d_refined_flags, d_result, d_result_flags, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbe_select_batch_device")


def init_normalize(kps):
    """Initializer::Normalize over all key points of one frame -> float32 {sX, sY, meanX, meanY} (include/orbi.h; needs no GPU)"""
    k = np.ascontiguousarray(kps, dtype=KP_DTYPE)
    out = np.zeros(4, np.float32)
    rc = lib().orbi_normalize(k.ctypes.data if len(k) else None, len(k), out.ctypes.data)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbi_normalize")
    return out


def init_pose_from_rt(fx, fy, cx, cy, R, t):
    """an INIT_POSE_DTYPE record {R, t, P2 = K*[R|t], O2 = -R.t()*t} in the cv::Mat evaluation order of DESIGN.md §2 (needs no GPU)"""
    R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
    pose = np.zeros(1, INIT_POSE_DTYPE)
    rc = lib().orbi_pose_from_rt(float(fx), float(fy), float(cx), float(cy), R.ctypes.data, t.ctypes.data, pose.ctypes.data)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbi_pose_from_rt")
    return pose[0]


def init_problem(kps1, kps2, nmatches, iters, sigma=1.0):
    """an INIT_PROBLEM_DTYPE record for one frame pair (Normalize of both frames included)"""
    q = np.zeros(1, INIT_PROBLEM_DTYPE)
    q["norm1"][0] = init_normalize(kps1); q["norm2"][0] = init_normalize(kps2)
    q["sigma"] = sigma; q["n1"] = len(kps1); q["n2"] = len(kps2); q["nmatches"] = nmatches; q["iters"] = iters
    return q[0]


def init_models_batch_device(problems, d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap, d_sets, icap, d_scoreH, d_scoreF, d_H21, d_H12, d_F21, d_hn,
                             d_fpre, d_best, d_S, d_inlH, d_inlF, stream=0):
    """the H / F RANSAC of Initializer::Initialize for len(problems) frame pairs (include/orbi.h); problems: host INIT_PROBLEM_DTYPE records,
    the rest device pointers as ints (0 = NULL)"""
    pr = np.ascontiguousarray(problems, dtype=INIT_PROBLEM_DTYPE).reshape(-1)
    rc = lib().orbi_models_batch_device(pr.ctypes.data, len(pr), d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap, d_sets, icap, d_scoreH, d_scoreF, d_H21,
                                        d_H12, d_F21, d_hn or None, d_fpre or None, d_best, d_S, d_inlH, d_inlF, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbi_models_batch_device")


def init_models(problem, kps1, kps2, matches, sets, device=0):
    """one frame pair, host arrays, synchronous -> dict(scoreH, scoreF, H21, H12, F21, hn, fpre, bestH, bestF, SH, SF, inlH, inlF)"""
    pr = np.ascontiguousarray(problem, dtype=INIT_PROBLEM_DTYPE).reshape(1)
    k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE); k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
    mt = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1, 2); st = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 8)
    N, I = int(pr["nmatches"][0]), int(pr["iters"][0])
    if len(mt) != N or len(st) != I or len(k1) != pr["n1"][0] or len(k2) != pr["n2"][0]:
        raise ValueError("the arrays do not have the problem's counts")
    o = dict(scoreH=np.zeros(I, np.float32), scoreF=np.zeros(I, np.float32), H21=np.zeros((I, 9), np.float32), H12=np.zeros((I, 9), np.float32),
             F21=np.zeros((I, 9), np.float32), hn=np.zeros((I, 9), np.float32), fpre=np.zeros((I, 9), np.float32), inlH=np.zeros(N, np.uint8),
             inlF=np.zeros(N, np.uint8))
    best = np.zeros(2, np.int32); S = np.zeros(2, np.float32)
    rc = lib().orbi_models(pr.ctypes.data, k1.ctypes.data, k2.ctypes.data, mt.ctypes.data, st.ctypes.data, o["scoreH"].ctypes.data, o["scoreF"].ctypes.data,
                           o["H21"].ctypes.data, o["H12"].ctypes.data, o["F21"].ctypes.data, o["hn"].ctypes.data, o["fpre"].ctypes.data, best.ctypes.data,
                           S.ctypes.data, o["inlH"].ctypes.data, o["inlF"].ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbi_models")
    o.update(bestH=int(best[0]), bestF=int(best[1]), SH=S[0], SF=S[1])
    return o


def init_check_rt_batch_device(fx, fy, cx, cy, d_poses, nhyp, n1, n2, nmatches, d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap, d_flags, th2, d_status,
                               d_x3d, d_cos, d_good, d_v, d_ngood, stream=0):
    """Initializer::CheckRT for nhyp poses of len(nmatches) frame pairs (include/orbi.h); n1, n2, nmatches host int arrays, the rest device
    pointers as ints (0 = NULL)"""
    a, b, c = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in (n1, n2, nmatches))
    if not len(a) == len(b) == len(c):
        raise ValueError("n1, n2 and nmatches must have one length")
    rc = lib().orbi_check_rt_batch_device(float(fx), float(fy), float(cx), float(cy), d_poses, nhyp, len(c), a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                          d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap, d_flags, float(th2), d_status, d_x3d, d_cos, d_good, d_v or None,
                                          d_ngood, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbi_check_rt_batch_device")


def init_check_rt(fx, fy, cx, cy, poses, kps1, kps2, matches, flags, th2, device=0):
    """one frame pair, host arrays, synchronous -> dict(status[nhyp, N], x3d[nhyp, N, 3], cos[nhyp, N], good[nhyp, N], v[nhyp, N, 4], ngood[nhyp],
    parallax[nhyp])"""
    ps = np.ascontiguousarray(poses, dtype=INIT_POSE_DTYPE).reshape(-1)
    k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE); k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
    mt = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1, 2); fl = np.ascontiguousarray(flags, dtype=np.uint8)
    H, N = len(ps), len(mt)
    if len(fl) != N:
        raise ValueError("one flag per match entry")
    o = dict(status=np.zeros((H, N), np.uint8), x3d=np.zeros((H, N, 3), np.float32), cos=np.zeros((H, N), np.float32), good=np.zeros((H, N), np.uint8),
             v=np.zeros((H, N, 4), np.float32), ngood=np.zeros(H, np.int32), parallax=np.zeros(H, np.float32))
    rc = lib().orbi_check_rt(float(fx), float(fy), float(cx), float(cy), ps.ctypes.data, H, k1.ctypes.data, len(k1), k2.ctypes.data, len(k2), mt.ctypes.data, N,
                             fl.ctypes.data, float(th2), o["status"].ctypes.data, o["x3d"].ctypes.data, o["cos"].ctypes.data, o["good"].ctypes.data,
                             o["v"].ctypes.data, o["ngood"].ctypes.data, o["parallax"].ctypes.data, device)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbi_check_rt")
    return o


def epipolar_bound(sigma2):
    return float(lib().orbs_epipolar_bound(ctypes.c_float(sigma2)))


def agreement_batch_device(d_match12, d_n1, cap1, d_match21, d_n2, cap2, nproblems, d_out12, d_nfound, stream=0):
    """the "check agreement" tail of ORBmatcher::SearchBySim3"""
    rc = lib().orbs_agreement_batch_device(d_match12, d_n1, cap1, d_match21, d_n2, cap2, nproblems, d_out12, d_nfound, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_agreement_batch_device")


def stream_create(device=0):
    """a raw non-blocking HIP stream (address) from the C ABI: creation order is under the caller's control"""
    p = ctypes.c_void_p()
    rc = lib().orbx_stream_create(device, ctypes.byref(p))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_stream_create")
    return p.value


def stream_destroy(device, stream):
    lib().orbx_stream_destroy(device, ctypes.c_void_p(stream))


def bow_ranges_batch_device(d_fvq_node, d_fvq_off, d_nfv_q, d_fvt_node, d_fvt_off, d_nfv_t, cap, nproblems, d_qrange, d_nq, stream=0):
    rc = lib().orbs_bow_ranges_batch_device(d_fvq_node, d_fvq_off, d_nfv_q, d_fvt_node, d_fvt_off, d_nfv_t, cap, nproblems, d_qrange, d_nq, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_bow_ranges_batch_device")


def bow_rows_search_batch_device(th, ratio, check_orientation, d_pair, npairs, d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap,
                                 d_qvalid, d_claimed, d_q2t, d_t2q, d_best, d_second, d_nmatches, stream=0):
    """SearchByBoW over the rows of a resident key-frame store, every (query row, train row) pair in one launch (include/orbs.h); device
    pointers as ints (0 = NULL).  Asynchronous on `stream`."""
    prm = SearchParams(RULE_BOW, th, ratio, 1 if check_orientation else 0)
    rc = lib().orbs_bow_rows_search_batch_device(ctypes.byref(prm), d_pair or None, npairs, d_kps or None, d_desc or None, d_nt or None, d_fv_node or None,
                                                 d_fv_off or None, d_fv_feat or None, d_nfv or None, nrows, cap, d_qvalid or None, d_claimed or None,
                                                 d_q2t or None, d_t2q or None, d_best or None, d_second or None, d_nmatches or None, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_bow_rows_search_batch_device")


def bow_rows_search(th, ratio, check_orientation, pairs, kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap, qvalid=None, claimed=None,
                    rows_on_device=False, want_dist=True, stream=0):
    """The same, synchronous: pairs[npairs, 2] and the per-pair flags qvalid / claimed [npairs, cap] are host arrays; the rows are host arrays
    (kps[nrows, cap] of KP_DTYPE, desc[nrows, cap, 32], nt[nrows], fv_node[nrows, cap], fv_off[nrows, cap + 1], fv_feat[nrows, cap], nfv[nrows]) or,
    with rows_on_device, device pointers as ints for all but the counts nt and nfv, which stay host arrays.  -> (nmatches[npairs], q2t[npairs, cap], t2q[npairs, cap], best, second (None without want_dist))"""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs = len(pr)
    keep = []

    def flags(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != (npairs, cap):
            raise ValueError("per-pair flags must be [npairs, cap]")
        keep.append(a)
        return a.ctypes.data

    if rows_on_device:
        counts = [np.ascontiguousarray(a, dtype=np.int32) for a in (nt, nfv)]
        if any(a.shape != (nrows,) for a in counts):
            raise ValueError("nt and nfv must have one entry per row")
        keep.extend(counts)
        rows = [int(kps) or None, int(desc) or None, counts[0].ctypes.data, int(fv_node) or None, int(fv_off) or None, int(fv_feat) or None, counts[1].ctypes.data]
    else:
        shapes = ((KP_DTYPE, (nrows, cap)), (np.uint8, (nrows, cap, 32)), (np.int32, (nrows,)), (np.uint32, (nrows, cap)), (np.int32, (nrows, cap + 1)),
                  (np.uint32, (nrows, cap)), (np.int32, (nrows,)))
        rows = []
        for a, (dt, shape) in zip((kps, desc, nt, fv_node, fv_off, fv_feat, nfv), shapes):
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != shape:
                raise ValueError("a row array has the wrong shape: %s, not %s" % (a.shape, shape))
            keep.append(a)
            rows.append(a.ctypes.data)
    n = max(npairs, 1)
    nm = np.zeros(n, np.int32)
    q2t = np.zeros((n, cap), np.int32); t2q = np.zeros((n, cap), np.int32)
    best = np.zeros((n, cap), np.int32) if want_dist else None
    second = np.zeros((n, cap), np.int32) if want_dist else None
    prm = SearchParams(RULE_BOW, th, ratio, 1 if check_orientation else 0)
    rc = lib().orbs_bow_rows_search(ctypes.byref(prm), pr.ctypes.data if npairs else None, npairs, *rows, nrows, cap, 1 if rows_on_device else 0,
                                    flags(qvalid), flags(claimed), q2t.ctypes.data, t2q.ctypes.data, best.ctypes.data if want_dist else None,
                                    second.ctypes.data if want_dist else None, nm.ctypes.data, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_bow_rows_search")
    return nm[:npairs], q2t[:npairs], t2q[:npairs], (best[:npairs] if want_dist else None), (second[:npairs] if want_dist else None)


def _host_rows(kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap, rows_on_device, keep):
    """the seven row arguments of the searches over resident rows as ctypes values: host arrays of the stated shapes, or with rows_on_device device
    pointers as ints for all but the counts nt and nfv"""
    if rows_on_device:
        counts = [np.ascontiguousarray(a, dtype=np.int32) for a in (nt, nfv)]
        if any(a.shape != (nrows,) for a in counts):
            raise ValueError("nt and nfv must have one entry per row")
        keep.extend(counts)
        return [int(kps) or None, int(desc) or None, counts[0].ctypes.data, int(fv_node) or None, int(fv_off) or None, int(fv_feat) or None, counts[1].ctypes.data]
    shapes = ((KP_DTYPE, (nrows, cap)), (np.uint8, (nrows, cap, 32)), (np.int32, (nrows,)), (np.uint32, (nrows, cap)), (np.int32, (nrows, cap + 1)),
              (np.uint32, (nrows, cap)), (np.int32, (nrows,)))
    rows = []
    for a, (dt, shape) in zip((kps, desc, nt, fv_node, fv_off, fv_feat, nfv), shapes):
        a = np.ascontiguousarray(a, dtype=dt)
        if a.shape != shape:
            raise ValueError("a row array has the wrong shape: %s, not %s" % (a.shape, shape))
        keep.append(a)
        rows.append(a.ctypes.data)
    return rows


def tri_rows_search_batch_device(th, check_orientation, d_pair, npairs, d_F12, level_sigma2, d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv,
                                 nrows, cap, d_qvalid, qstride, d_claimed, d_q2t, d_t2q, d_best, d_second, d_nmatches, stream=0):
    """SearchForTriangulation over the rows of a resident key-frame store, every (query row, train row) pair in one launch (include/orbs.h);
    device pointers as ints (0 = NULL), level_sigma2 a host float array (mvLevelSigma2 of pKF2).  Asynchronous on `stream`."""
    prm = SearchParams(RULE_TRIANGULATION, th, 0.0, 1 if check_orientation else 0)
    s2 = np.ascontiguousarray(level_sigma2, dtype=np.float32)
    rc = lib().orbs_tri_rows_search_batch_device(ctypes.byref(prm), d_pair or None, npairs, d_F12 or None, s2.ctypes.data, len(s2), d_kps or None,
                                                 d_desc or None, d_nt or None, d_fv_node or None, d_fv_off or None, d_fv_feat or None, d_nfv or None, nrows,
                                                 cap, d_qvalid or None, qstride, d_claimed or None, d_q2t or None, d_t2q or None, d_best or None,
                                                 d_second or None, d_nmatches or None, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_tri_rows_search_batch_device")


def tri_rows_search(th, check_orientation, pairs, F12, level_sigma2, kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap, qvalid=None, claimed=None,
                    rows_on_device=False, want_dist=True, stream=0):
    """The same, synchronous: pairs[npairs, 2], F12[npairs, 9] and the flags are host arrays (qvalid [cap]: shared by the pairs, or [npairs, cap];
    claimed [npairs, cap]); the rows as in bow_rows_search.  -> (nmatches[npairs], q2t[npairs, cap], t2q[npairs, cap], best, second (None without want_dist))"""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs = len(pr)
    keep = []
    F = np.ascontiguousarray(F12, dtype=np.float32).reshape(-1, 9)
    if len(F) != npairs:
        raise ValueError("F12 must have nine floats per pair")
    s2 = np.ascontiguousarray(level_sigma2, dtype=np.float32)
    qstride, qv, cl = 0, None, None
    if qvalid is not None:
        qv = np.ascontiguousarray(qvalid, dtype=np.uint8)
        if qv.shape not in ((cap,), (npairs, cap)):
            raise ValueError("qvalid must be [cap] or [npairs, cap]")
        qstride = cap if qv.ndim == 2 else 0
    if claimed is not None:
        cl = np.ascontiguousarray(claimed, dtype=np.uint8)
        if cl.shape != (npairs, cap):
            raise ValueError("claimed must be [npairs, cap]")
    rows = _host_rows(kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap, rows_on_device, keep)
    n = max(npairs, 1)
    nm = np.zeros(n, np.int32)
    q2t = np.zeros((n, cap), np.int32); t2q = np.zeros((n, cap), np.int32)
    best = np.zeros((n, cap), np.int32) if want_dist else None
    second = np.zeros((n, cap), np.int32) if want_dist else None
    prm = SearchParams(RULE_TRIANGULATION, th, 0.0, 1 if check_orientation else 0)
    rc = lib().orbs_tri_rows_search(ctypes.byref(prm), pr.ctypes.data if npairs else None, npairs, F.ctypes.data if npairs else None, s2.ctypes.data, len(s2),
                                    *rows, nrows, cap, 1 if rows_on_device else 0, qv.ctypes.data if qv is not None else None, qstride,
                                    cl.ctypes.data if cl is not None else None, q2t.ctypes.data, t2q.ctypes.data, best.ctypes.data if want_dist else None,
                                    second.ctypes.data if want_dist else None, nm.ctypes.data, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbs_tri_rows_search")
    return nm[:npairs], q2t[:npairs], t2q[:npairs], (best[:npairs] if want_dist else None), (second[:npairs] if want_dist else None)


def new_points_rows_device(th, check_orientation, pairs, d_pairs, d_F12, factors1, sigma2_1, factors2, sigma2_2, d_kps, d_desc, d_nt, d_fv_node, d_fv_off,
                           d_fv_feat, d_nfv, nrows, cap, d_qvalid, d_claimed, d_q2t, d_t2q, d_nmatches, d_status, d_x3d, d_v, d_match12, d_acc_idx,
                           d_acc_x3d, d_count, d_overflow, ocap, stream=0):
    """The neighbour loop of LocalMapping::CreateNewMapPoints as one stream-ordered chain over resident rows (include/orbt.h): per pair the
    search, its finish and the triangulation, whose flag updates the next pair's search reads.  pairs[npairs, 2] is a HOST list; device pointers
    as ints (0 = NULL); the level tables host float arrays.  Asynchronous on `stream`."""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    f1, s1, f2, s2 = _level_tables(factors1, sigma2_1, factors2, sigma2_2)
    prm = SearchParams(RULE_TRIANGULATION, th, 0.0, 1 if check_orientation else 0)
    rc = lib().orbt_new_points_rows_device(ctypes.byref(prm), pr.ctypes.data if len(pr) else None, len(pr), d_pairs or None, d_F12 or None, f1.ctypes.data,
                                           s1.ctypes.data, f2.ctypes.data, s2.ctypes.data, len(f1), d_kps or None, d_desc or None, d_nt or None,
                                           d_fv_node or None, d_fv_off or None, d_fv_feat or None, d_nfv or None, nrows, cap, d_qvalid or None,
                                           d_claimed or None, d_q2t or None, d_t2q or None, d_nmatches or None, d_status or None, d_x3d or None,
                                           d_v or None, d_match12 or None, d_acc_idx or None, d_acc_x3d or None, d_count or None, d_overflow or None, ocap,
                                           stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbt_new_points_rows_device")


def new_points_rows(th, check_orientation, pairs, tri_pairs, F12, factors1, sigma2_1, factors2, sigma2_2, kps, desc, nt, fv_node, fv_off, fv_feat, nfv,
                    nrows, cap, qvalid, claimed, ocap=None, rows_on_device=False, want_v=True, stream=0):
    """The same, synchronous, over host arrays: tri_pairs[npairs] of TRI_PAIR_DTYPE, F12[npairs, 9], qvalid[cap], claimed[npairs, cap] (both are
    copied; the updated flags are returned).  -> dict(nmatches, q2t, t2q, status, x3d, v (None without want_v), match12, acc_idx, acc_x3d, count,
    overflow, qvalid, claimed), per pair; acc_idx[p, :count[p]] are the accepted (idx1, idx2) in ascending idx1"""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs = len(pr)
    tp = np.ascontiguousarray(tri_pairs, dtype=TRI_PAIR_DTYPE).reshape(-1)
    F = np.ascontiguousarray(F12, dtype=np.float32).reshape(-1, 9)
    if len(tp) != npairs or len(F) != npairs:
        raise ValueError("one orbt_pair record and nine floats of F12 per pair")
    f1, s1, f2, s2 = _level_tables(factors1, sigma2_1, factors2, sigma2_2)
    qv = np.array(qvalid, dtype=np.uint8); cl = np.array(claimed, dtype=np.uint8).reshape(-1, cap)
    if qv.shape != (cap,) or cl.shape != (npairs, cap):
        raise ValueError("qvalid must be [cap], claimed [npairs, cap]")
    keep = []
    rows = _host_rows(kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap, rows_on_device, keep)
    ocap = cap if ocap is None else ocap
    n = max(npairs, 1)
    o = dict(nmatches=np.zeros(n, np.int32), q2t=np.zeros((n, cap), np.int32), t2q=np.zeros((n, cap), np.int32), status=np.zeros((n, cap), np.uint8),
             x3d=np.zeros((n, cap, 3), np.float32), v=np.zeros((n, cap, 4), np.float32) if want_v else None, match12=np.zeros((n, cap), np.int32),
             acc_idx=np.zeros((n, max(ocap, 1), 2), np.int32), acc_x3d=np.zeros((n, max(ocap, 1), 3), np.float32), count=np.zeros(n, np.int32),
             overflow=np.zeros(n, np.int32))
    prm = SearchParams(RULE_TRIANGULATION, th, 0.0, 1 if check_orientation else 0)
    rc = lib().orbt_new_points_rows(ctypes.byref(prm), pr.ctypes.data if npairs else None, npairs, tp.ctypes.data if npairs else None,
                                    F.ctypes.data if npairs else None, f1.ctypes.data, s1.ctypes.data, f2.ctypes.data, s2.ctypes.data, len(f1), *rows, nrows,
                                    cap, 1 if rows_on_device else 0, qv.ctypes.data, cl.ctypes.data, o["q2t"].ctypes.data, o["t2q"].ctypes.data,
                                    o["nmatches"].ctypes.data, o["status"].ctypes.data, o["x3d"].ctypes.data, o["v"].ctypes.data if want_v else None,
                                    o["match12"].ctypes.data, o["acc_idx"].ctypes.data, o["acc_x3d"].ctypes.data, o["count"].ctypes.data,
                                    o["overflow"].ctypes.data, ocap, stream or None)
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbt_new_points_rows")
    o = {k: (a[:npairs] if a is not None else None) for k, a in o.items()}
    o["qvalid"], o["claimed"] = qv, cl
    return o


class KeyFrameDatabase:
    """The device half of ORB_SLAM::KeyFrameDatabase (reference src/KeyFrameDatabase.cc) over include/orbd.h: key frames are
    caller-chosen slots; query() returns what DetectLoopCandidates / DetectRelocalisationCandidates compute from the inverted
    file (the key frames sharing words in lKFsSharingWords order, their counts, the 0.8 threshold and the scores above it).
    The KeyFrame-walking rest is host C++ (orb_slam_amd/cpp/KeyFrameDatabase.cc) or, for tests, tests/kfdb_ref.py."""

    def __init__(self, voc, capacity, device=0):
        self.h = ctypes.c_void_p()
        self.device = device
        rc = lib().orbd_create(voc.h, capacity, device, ctypes.byref(self.h))
        if rc != ORBX_OK:
            self.h = None
            raise OrbxError(rc, "orbd_create")

    def close(self):
        if getattr(self, "h", None):
            lib().orbd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except TypeError:           # interpreter shutdown
            pass

    def __len__(self):
        return lib().orbd_size(self.h)

    def add(self, slot, ids, vals):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert len(ids) == len(vals)
        rc = lib().orbd_add(self.h, slot, ids.ctypes.data, vals.ctypes.data, len(ids))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbd_add")

    def add_batch_device(self, slots, d_bow_id, d_bow_val, d_n_bow, cap, d_status=None, stream=0):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        rc = lib().orbd_add_batch_device(self.h, slots.ctypes.data, len(slots), d_bow_id, d_bow_val, d_n_bow, cap, d_status, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbd_add_batch_device")

    def erase(self, slot):
        rc = lib().orbd_erase(self.h, slot)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbd_erase")

    def clear(self):
        rc = lib().orbd_clear(self.h)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbd_clear")

    def query(self, ids, vals, excl=(), out_cap=None):
        """-> dict(slot, words, score, min_common, excl_words); raises OrbxError(ORBX_ERR_CAPACITY) when out_cap is too small"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        excl = np.ascontiguousarray(excl, dtype=np.int32)
        cap = lib().orbd_size(self.h) if out_cap is None else out_cap
        slot = np.zeros(max(cap, 1), np.int32); words = np.zeros(max(cap, 1), np.int32); score = np.zeros(max(cap, 1), np.float64)
        xw = np.zeros(max(len(excl), 1), np.int32)
        ns, mc = ctypes.c_int(), ctypes.c_int()
        rc = lib().orbd_query(self.h, ids.ctypes.data, vals.ctypes.data, len(ids), excl.ctypes.data, len(excl), xw.ctypes.data,
                              slot.ctypes.data, words.ctypes.data, score.ctypes.data, cap, ctypes.byref(ns), ctypes.byref(mc), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbd_query (n_share=%d)" % ns.value)
        n = ns.value
        return dict(slot=slot[:n], words=words[:n], score=score[:n], min_common=mc.value, excl_words=xw[:len(excl)])

    def query_batch_device(self, nq, d_bow_id, d_bow_val, d_n_bow, qcap, d_excl_off, d_excl_slot, d_excl_words, d_share_slot, d_share_words,
                           d_share_score, out_cap, d_n_share, d_min_common, d_status, stream=0):
        rc = lib().orbd_query_batch_device(self.h, nq, d_bow_id, d_bow_val, d_n_bow, qcap, d_excl_off, d_excl_slot, d_excl_words, d_share_slot,
                                           d_share_words, d_share_score, out_cap, d_n_share, d_min_common, d_status, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbd_query_batch_device")


class MapPointTable:
    """The local map's points in HBM (include/orbp.h): position, mean viewing direction, scale-invariance distances and descriptor per
    caller-chosen slot; project / track run Frame::isInFrustum and Tracking's local-map search for whole batches of poses."""

    def __init__(self, capacity, device=0):
        self.h = ctypes.c_void_p()
        self.device = device
        rc = lib().orbp_create(capacity, device, ctypes.byref(self.h))
        if rc != ORBX_OK:
            self.h = None
            raise OrbxError(rc, "orbp_create")
        self.capacity = capacity

    def close(self):
        if getattr(self, "h", None):
            lib().orbp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except TypeError:           # interpreter shutdown
            pass

    def __len__(self):
        return lib().orbp_size(self.h)

    def put(self, slots, pos, normal, min_dist, max_dist, desc=None):
        """host arrays; desc=None keeps the stored descriptors (every slot must then be live)"""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(slots)
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(n, 3)
        normal = np.ascontiguousarray(normal, dtype=np.float32).reshape(n, 3)
        dmin = np.ascontiguousarray(min_dist, dtype=np.float32).reshape(n)
        dmax = np.ascontiguousarray(max_dist, dtype=np.float32).reshape(n)
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(n, 32)
        rc = lib().orbp_put(self.h, slots.ctypes.data, n, pos.ctypes.data, normal.ctypes.data, dmin.ctypes.data, dmax.ctypes.data,
                            desc.ctypes.data if desc is not None else None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_put")

    def put_device(self, slots, d_pos, d_normal, d_min_dist, d_max_dist, d_desc=0, stream=0):
        """slots: host array; the data: device pointers as ints (d_desc 0 keeps the stored descriptors)"""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        rc = lib().orbp_put_device(self.h, slots.ctypes.data, len(slots), d_pos, d_normal, d_min_dist, d_max_dist, d_desc or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_put_device")

    def erase(self, slots):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        rc = lib().orbp_erase(self.h, slots.ctypes.data, len(slots))
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_erase")

    def clear(self):
        rc = lib().orbp_clear(self.h)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_clear")

    def get(self, slot):
        """-> None for a free slot, else dict(pos, normal, min_dist, max_dist, desc)"""
        live = ctypes.c_int()
        pos = np.zeros(3, np.float32); nrm = np.zeros(3, np.float32); dmin = np.zeros(1, np.float32); dmax = np.zeros(1, np.float32)
        desc = np.zeros(32, np.uint8)
        rc = lib().orbp_get(self.h, slot, ctypes.byref(live), pos.ctypes.data, nrm.ctypes.data, dmin.ctypes.data, dmax.ctypes.data, desc.ctypes.data)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_get")
        return dict(pos=pos, normal=nrm, min_dist=dmin[0], max_dist=dmax[0], desc=desc) if live.value else None

    def refresh_batch_device(self, slots, d_pos, d_obs_off, d_obs, d_ref, d_skip, d_kf_ow, d_kf_bad, d_kf_kps, d_kf_desc, nkf, cap, factors,
                             what=REFRESH_NORMAL_DEPTH | REFRESH_DESCRIPTOR, d_out=0, stream=0):
        """MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors for the listed slots, in place and asynchronous.  slots, factors: host
        arrays; everything else device pointers as ints (0 = NULL: d_pos keeps the stored positions)"""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_refresh_batch_device(self.h, slots.ctypes.data, len(slots), d_pos or None, d_obs_off or None, d_obs or None, d_ref or None,
                                             d_skip or None, d_kf_ow or None, d_kf_bad or None, d_kf_kps or None, d_kf_desc or None, nkf, cap,
                                             f.ctypes.data, len(f), what, d_out or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_refresh_batch_device")

    def refresh(self, slots, obs_off, obs, ref, kf_ow, kf_kps, kf_desc, factors, pos=None, skip=None, kf_bad=None, nkf=None, cap=None,
                what=REFRESH_NORMAL_DEPTH | REFRESH_DESCRIPTOR):
        """The same with host arrays, synchronous (the latency form): -> the records (REFRESHED_DTYPE[n]).  obs: (total, 2) int32 pairs {kf, idx};
        kf_kps (nkf, cap) KP_DTYPE and kf_desc (nkf, cap, 32) are host arrays, or device pointers as ints (nkf and cap must then be given)."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(slots)
        f = np.ascontiguousarray(factors, dtype=np.float32)
        obs_off = np.ascontiguousarray(obs_off, dtype=np.int32)
        obs = np.ascontiguousarray(obs, dtype=np.int32).reshape(-1, 2)
        assert len(obs_off) == n + 1 and (n == 0 or len(obs) >= obs_off[-1])
        opt = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)
        ref = opt(ref, np.int32, n); pos = opt(pos, np.float32, (n, 3)); skip = opt(skip, np.uint8, n)
        kf_dev = isinstance(kf_kps, int) or isinstance(kf_desc, int)
        if not kf_dev:
            if kf_kps is not None:
                kf_kps = np.ascontiguousarray(kf_kps)
                assert kf_kps.dtype.itemsize == 28 and kf_kps.ndim == 2
                nkf, cap = kf_kps.shape
            if kf_desc is not None:
                kf_desc = np.ascontiguousarray(kf_desc, dtype=np.uint8)
                assert kf_desc.ndim == 3 and kf_desc.shape[2] == 32 and (kf_kps is None or kf_desc.shape[:2] == kf_kps.shape)
                nkf, cap = kf_desc.shape[:2]
        kf_ow = opt(kf_ow, np.float32, (nkf, 3)); kf_bad = opt(kf_bad, np.uint8, nkf)
        out = np.zeros(max(n, 1), REFRESHED_DTYPE)
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        rc = lib().orbp_refresh(self.h, ptr(slots), n, ptr(pos), ptr(obs_off), ptr(obs), ptr(ref), ptr(skip), ptr(kf_ow), ptr(kf_bad), ptr(kf_kps),
                                ptr(kf_desc), 1 if kf_dev else 0, nkf, cap, f.ctypes.data, len(f), what, ptr(out), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_refresh")
        return out[:n]

    def fuse_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, bounds, orb_dist, d_kps_un, d_desc, d_cell_off, d_cell_feat,
                          d_nt, nframes, cap, d_frame, d_best_idx, d_best_dist, d_rec=0, stream=0):
        """The search of ORBmatcher::Fuse(pKF, vpMapPoints, th) for nviews key-frame views in one launch, asynchronous.  factors: host array;
        everything else device pointers as ints (0 = NULL: d_skip, d_frame, d_rec)"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_fuse_batch_device(self.h, d_views or None, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap, d_skip or None,
                                          ctypes.addressof(bounds), orb_dist, d_kps_un or None, d_desc or None, d_cell_off or None, d_cell_feat or None,
                                          d_nt or None, nframes, cap, d_frame or None, d_best_idx or None, d_best_dist or None, d_rec or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_fuse_batch_device")

    def fuse(self, views, factors, lists, nlist, bounds, orb_dist, kps_un, desc, cell_off, cell_feat, nt, skip=None, frame=None, nframes=None, cap=None,
             best_idx=None, best_dist=None, rec=None):
        """The same with host arrays, synchronous: -> (best_idx i32[nviews, lcap], best_dist i32[nviews, lcap], rec FUSED_DTYPE[nviews, lcap]);
        entries at i >= nlist[p] are left as they are (-1 / INT32_MAX / zero when the arrays are made here).  views: VIEW_DTYPE[nviews];
        lists (nviews, lcap) int32 slots.  The key frames in the batch layout: kps_un (nframes, cap) KP_DTYPE, desc (nframes, cap, 32),
        cell_off (nframes, GRID_CELLS + 1), cell_feat (nframes, cap) are host arrays, or device pointers as ints (nframes and cap must then
        be given); nt (nframes) and frame (nviews, optional) are host arrays."""
        views = np.ascontiguousarray(views, dtype=VIEW_DTYPE).reshape(-1)
        nviews = len(views)
        f = np.ascontiguousarray(factors, dtype=np.float32)
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        lists = lists.reshape(nviews, -1) if nviews else lists.reshape(0, lists.shape[-1] if lists.ndim == 2 and lists.shape[-1] else 1)
        lcap = lists.shape[1]
        nlist = np.ascontiguousarray(nlist, dtype=np.int32).reshape(nviews)
        opt = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)
        skip = opt(skip, np.uint8, (nviews, lcap)); frame = opt(frame, np.int32, nviews)
        on_dev = isinstance(kps_un, int)
        if not on_dev:
            kps_un = np.ascontiguousarray(kps_un)
            assert kps_un.dtype.itemsize == 28 and kps_un.ndim == 2
            nframes, cap = kps_un.shape
            desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(nframes, cap, 32)
            cell_off = np.ascontiguousarray(cell_off, dtype=np.int32).reshape(nframes, GRID_CELLS + 1)
            cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32).reshape(nframes, cap)
        nt = np.ascontiguousarray(nt, dtype=np.int32).reshape(nframes)
        if best_idx is None:
            best_idx = np.full((nviews, lcap), -1, np.int32)
        if best_dist is None:
            best_dist = np.full((nviews, lcap), np.iinfo(np.int32).max, np.int32)
        if rec is None:
            rec = np.zeros((nviews, lcap), FUSED_DTYPE)
        assert best_idx.dtype == np.int32 and best_dist.dtype == np.int32 and rec.dtype == FUSED_DTYPE
        assert all(a.flags.c_contiguous and a.size == nviews * lcap for a in (best_idx, best_dist, rec))
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        rc = lib().orbp_fuse(self.h, ptr(views), nviews, f.ctypes.data, len(f), ptr(lists), ptr(nlist), lcap, ptr(skip), ctypes.addressof(bounds), orb_dist,
                             ptr(kps_un), ptr(desc), ptr(cell_off), ptr(cell_feat), ptr(nt), nframes, cap, 1 if on_dev else 0, ptr(frame), ptr(best_idx),
                             ptr(best_dist), ptr(rec), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_fuse")
        return best_idx, best_dist, rec

    def sim3_search_batch_device(self, d_dirs, npairs, factors, d_list, d_nlist, lcap, d_skip, d_frame, d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt,
                                 nframes, cap, bounds, orb_dist, d_best_idx, d_best_dist, d_rec, d_match12, d_nfound, stream=0):
        """ORBmatcher::SearchBySim3 for npairs pairs of key frames, asynchronous: both directions of every pair in one launch (rows 2p and 2p + 1 of the
        per-row arrays), the agreement in a second.  factors: host array; everything else device pointers as ints (0 = NULL: d_skip, d_frame, d_rec)"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_sim3_search_batch_device(self.h, d_dirs or None, npairs, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap, d_skip or None,
                                                 d_frame or None, d_kps_un or None, d_desc or None, d_cell_off or None, d_cell_feat or None, d_nt or None,
                                                 nframes, cap, ctypes.addressof(bounds), orb_dist, d_best_idx or None, d_best_dist or None, d_rec or None,
                                                 d_match12 or None, d_nfound or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_sim3_search_batch_device")

    def sim3_search(self, dirs, factors, lists, nlist, frame, bounds, orb_dist, kps_un, desc, cell_off, cell_feat, nt, skip=None, nframes=None, cap=None):
        """The same with host arrays, synchronous: -> dict(match12 i32[npairs, lcap] (vpMatches12[i1] = key frame 2's feature, -1 none), nfound
        i32[npairs], best_idx / best_dist i32[2 npairs, lcap], rec FUSED_DTYPE[2 npairs, lcap]); entries at i >= nlist[row] are -1 / INT32_MAX / zero.
        dirs: SIM3_DIR_DTYPE[2 npairs] (sim3_from_pair per pair); lists (2 npairs, lcap) int32 slots by source feature (-1: no map point); frame
        (2 npairs) the key frame each row searches (None: row r searches key frame r).  The key frames in the batch layout as for fuse(): host
        arrays, or device pointers as ints (nframes and cap must then be given); nt (nframes) is a host array."""
        dirs = np.ascontiguousarray(dirs, dtype=SIM3_DIR_DTYPE).reshape(-1)
        assert len(dirs) % 2 == 0
        nrows, npairs = len(dirs), len(dirs) // 2
        f = np.ascontiguousarray(factors, dtype=np.float32)
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        lists = lists.reshape(nrows, -1) if nrows else lists.reshape(0, lists.shape[-1] if lists.ndim == 2 and lists.shape[-1] else 1)
        lcap = lists.shape[1]
        nlist = np.ascontiguousarray(nlist, dtype=np.int32).reshape(nrows)
        opt = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)
        skip = opt(skip, np.uint8, (nrows, lcap)); frame = opt(frame, np.int32, nrows)
        on_dev = isinstance(kps_un, int)
        if not on_dev:
            kps_un = np.ascontiguousarray(kps_un)
            assert kps_un.dtype.itemsize == 28 and kps_un.ndim == 2
            nframes, cap = kps_un.shape
            desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(nframes, cap, 32)
            cell_off = np.ascontiguousarray(cell_off, dtype=np.int32).reshape(nframes, GRID_CELLS + 1)
            cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32).reshape(nframes, cap)
        nt = np.ascontiguousarray(nt, dtype=np.int32).reshape(nframes)
        best_idx = np.full((nrows, lcap), -1, np.int32)
        best_dist = np.full((nrows, lcap), np.iinfo(np.int32).max, np.int32)
        rec = np.zeros((nrows, lcap), FUSED_DTYPE)
        match12 = np.full((npairs, lcap), -1, np.int32)
        nfound = np.zeros(max(npairs, 1), np.int32)
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        rc = lib().orbp_sim3_search(self.h, ptr(dirs), npairs, f.ctypes.data, len(f), ptr(lists), ptr(nlist), lcap, ptr(skip), ptr(frame), ptr(kps_un),
                                    ptr(desc), ptr(cell_off), ptr(cell_feat), ptr(nt), nframes, cap, 1 if on_dev else 0, ctypes.addressof(bounds), orb_dist,
                                    ptr(best_idx), ptr(best_dist), ptr(rec), ptr(match12), ptr(nfound), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_sim3_search")
        return dict(match12=match12, nfound=nfound[:npairs], best_idx=best_idx, best_dist=best_dist, rec=rec)

    def local_votes_batch_device(self, d_query, d_nquery, qcap, nproblems, d_kf_slot, d_kf_nt, nkf, cap, d_votes, stream=0):
        """The votes of Tracking::UpdateReferenceKeyFrames / KeyFrame::UpdateConnections for nproblems queries over the map-point column of nkf
        resident rows, asynchronous: d_votes[p*nkf + k].  Device pointers as ints."""
        rc = lib().orbp_local_votes_batch_device(self.h, d_query or None, d_nquery or None, qcap, nproblems, d_kf_slot or None, d_kf_nt or None, nkf, cap,
                                                 d_votes or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_local_votes_batch_device")

    @staticmethod
    def _columns(kf_slot, kf_nt, nkf, cap):
        """the columns as host arrays (nkf, cap) / (nkf), or device pointers as ints (nkf and cap must then be given)"""
        on_dev = isinstance(kf_slot, int)
        if not on_dev:
            kf_slot = np.ascontiguousarray(kf_slot, dtype=np.int32)
            assert kf_slot.ndim == 2
            nkf, cap = kf_slot.shape
            kf_nt = np.ascontiguousarray(kf_nt, dtype=np.int32).reshape(nkf)
        return kf_slot, kf_nt, nkf, cap, on_dev

    @staticmethod
    def _padded(lists, width=None):
        """a sequence of int sequences (or a 2-D array with its counts) as (array (n, width), counts (n))"""
        n = np.array([len(q) for q in lists], np.int32)
        width = width or max(1, int(n.max()) if len(n) else 1)
        out = np.full((len(lists), width), -1, np.int32)
        for p, q in enumerate(lists):
            out[p, :len(q)] = q
        return out, n

    def local_votes(self, queries, kf_slot, kf_nt, nkf=None, cap=None):
        """The same with host arrays, synchronous: queries is a sequence of slot sequences -> votes i32[nproblems, nkf]."""
        query, nquery = self._padded(queries)
        kf_slot, kf_nt, nkf, cap, on_dev = self._columns(kf_slot, kf_nt, nkf, cap)
        votes = np.zeros((len(nquery), nkf), np.int32)
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        rc = lib().orbp_local_votes(self.h, ptr(query), ptr(nquery), query.shape[1], len(nquery), ptr(kf_slot), ptr(kf_nt), 1 if on_dev else 0, nkf, cap,
                                    ptr(votes), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_local_votes")
        return votes

    def local_points_batch_device(self, d_query, d_nquery, qcap, nproblems, d_rows, d_nrows, rcap, d_kf_slot, d_kf_nt, nkf, cap, d_list, d_nlist, d_skip,
                                  d_overflow, lcap, stream=0):
        """The list of Tracking::UpdateReferencePoints with the skip flags of SearchReferencePointsInFrustum's first loop, asynchronous, in the
        layout track_batch_device reads.  Device pointers as ints (d_query 0: no query, every flag 0)."""
        rc = lib().orbp_local_points_batch_device(self.h, d_query or None, d_nquery or None, qcap, nproblems, d_rows or None, d_nrows or None, rcap,
                                                  d_kf_slot or None, d_kf_nt or None, nkf, cap, d_list or None, d_nlist or None, d_skip or None,
                                                  d_overflow or None, lcap, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_local_points_batch_device")

    def local_points(self, queries, rows, kf_slot, kf_nt, lcap, nkf=None, cap=None):
        """The same with host arrays, synchronous: queries (or None) and rows are sequences of sequences, one per problem
        -> (list i32[nproblems, lcap], nlist i32[nproblems], skip u8[nproblems, lcap], overflow i32[nproblems]); entries behind a list are -1 / 0."""
        rws, nrows = self._padded(rows)
        npr = len(nrows)
        query, nquery = self._padded(queries) if queries is not None else (None, None)
        assert query is None or len(nquery) == npr
        kf_slot, kf_nt, nkf, cap, on_dev = self._columns(kf_slot, kf_nt, nkf, cap)
        lst = np.full((npr, lcap), -1, np.int32)
        skip = np.zeros((npr, lcap), np.uint8)
        nlist = np.zeros(npr, np.int32)
        overflow = np.zeros(npr, np.int32)
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        rc = lib().orbp_local_points(self.h, ptr(query), ptr(nquery), query.shape[1] if query is not None else 1, npr, ptr(rws), ptr(nrows), rws.shape[1],
                                     ptr(kf_slot), ptr(kf_nt), 1 if on_dev else 0, nkf, cap, ptr(lst), ptr(nlist), ptr(skip), ptr(overflow), lcap, None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_local_points")
        return lst, nlist, skip, overflow

    def rows_purge_device(self, slots, d_kf_slot, nkf, cap, stream=0):
        """every entry of the device column d_kf_slot[nkf*cap] that names one of `slots` (host array) becomes -1; asynchronous"""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        rc = lib().orbp_rows_purge_device(self.h, slots.ctypes.data, len(slots), d_kf_slot or None, nkf, cap, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_rows_purge_device")

    def cull_batch_device(self, d_cand, ncand, d_kf_slot, d_kf_oct, d_kf_nt, nkf, cap, nlevels, d_nmps, d_nred, d_cull, stream=0):
        """The decisions of LocalMapping::KeyFrameCulling for the candidate rows d_cand, in list order, over the slot and octave columns of nkf
        resident rows, asynchronous: d_nmps / d_nred / d_cull[ncand].  Device pointers as ints."""
        rc = lib().orbp_cull_batch_device(self.h, d_cand or None, ncand, d_kf_slot or None, d_kf_oct or None, d_kf_nt or None, nkf, cap, nlevels,
                                          d_nmps or None, d_nred or None, d_cull or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_cull_batch_device")

    def cull(self, cand, kf_slot, kf_oct, kf_nt, nlevels=8, nkf=None, cap=None):
        """The same with host arrays, synchronous -> (nmps, nred, cull), i32[ncand] each.  The columns are host arrays (nkf, cap) / (nkf), or device
        pointers as ints (nkf and cap must then be given)."""
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1)
        kf_slot, kf_nt, nkf, cap, on_dev = self._columns(kf_slot, kf_nt, nkf, cap)
        if not on_dev:
            kf_oct = np.ascontiguousarray(kf_oct, dtype=np.uint8)
            assert kf_oct.shape == (nkf, cap)
        nmps, nred, cull = (np.zeros(len(cand), np.int32) for _ in range(3))
        ptr = lambda a: (a or None) if isinstance(a, int) else a.ctypes.data
        rc = lib().orbp_cull(self.h, ptr(cand), len(cand), ptr(kf_slot), ptr(kf_oct), ptr(kf_nt), 1 if on_dev else 0, nkf, cap, nlevels, ptr(nmps),
                             ptr(nred), ptr(cull), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_cull")
        return nmps, nred, cull

    def project_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, d_rec, d_qxyr, d_qlev, d_qdesc, d_qpos, d_nq,
                             d_overflow, qcap, stream=0):
        """device pointers as ints (0 = NULL); factors: host float array (mvScaleFactors)"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_project_batch_device(self.h, d_views, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap, d_skip or None,
                                             d_rec or None, d_qxyr, d_qlev, d_qdesc, d_qpos, d_nq, d_overflow, qcap, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_project_batch_device")

    def track_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, bounds, ratio, d_kps_un, d_desc, d_cell_off,
                           d_cell_feat, d_nt, cap, d_claimed, qcap, d_rec, d_t2slot, d_nmatches, d_nq, d_overflow, stream=0):
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_track_batch_device(self.h, d_views, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap, d_skip or None,
                                           ctypes.byref(bounds), ratio, d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed or None, qcap,
                                           d_rec or None, d_t2slot, d_nmatches, d_nq, d_overflow, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_track_batch_device")

    def track(self, view, factors, bounds, ratio, kps_un, desc, cell_off, cell_feat, claimed=None, list=None, skip=None, qcap=None,
              want_records=True):
        """One view, host arrays (the latency form): -> dict(t2slot, nmatches, nvisible, rec).  list=None: all live slots (records by slot).
        Raises OrbxError(ORBX_ERR_CAPACITY) when more than qcap points are visible."""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        kps_un = np.ascontiguousarray(kps_un)
        nt = len(kps_un)
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(nt, 32)
        cell_off = np.ascontiguousarray(cell_off, dtype=np.int32)
        cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32)
        assert kps_un.dtype.itemsize == 28 and len(cell_off) == GRID_CELLS + 1
        if claimed is not None:
            claimed = np.ascontiguousarray(claimed, dtype=np.uint8)
        if list is not None:
            list = np.ascontiguousarray(list, dtype=np.int32)
        nlist = self.capacity if list is None else len(list)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            assert len(skip) == nlist
        qcap = qcap or max(1, min(nlist, 8192))
        rec = np.zeros(max(nlist, 1), RECORD_DTYPE) if want_records else None
        t2slot = np.full(max(nt, 1), -1, np.int32)
        nm, nv = ctypes.c_int(), ctypes.c_int()
        ptr = lambda a: a.ctypes.data if a is not None else None
        rc = lib().orbp_track(self.h, ctypes.byref(view), f.ctypes.data, len(f), ptr(list), nlist, ptr(skip), ctypes.byref(bounds), ratio,
                              ptr(kps_un), ptr(desc), ptr(cell_off), ptr(cell_feat), ptr(claimed), nt, 0, qcap, ptr(rec), ptr(t2slot),
                              ctypes.byref(nm), ctypes.byref(nv), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_track (nvisible=%d)" % nv.value)
        return dict(t2slot=t2slot[:nt], nmatches=nm.value, nvisible=nv.value, rec=rec[:nlist] if rec is not None else None)

    def project_source_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, d_src_kps, d_src_desc, d_qxyr, d_qlev, d_qdesc,
                                    d_qangle, d_qpos, d_nq, d_overflow, qcap, stream=0):
        """the queries of the last-frame / key-frame projection searches (view.mode = MODE_LAST_FRAME / MODE_KEYFRAME): device pointers as ints"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_project_source_batch_device(self.h, d_views, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap,
                                                    d_skip or None, d_src_kps or None, d_src_desc or None, d_qxyr, d_qlev, d_qdesc, d_qangle, d_qpos,
                                                    d_nq, d_overflow, qcap, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_project_source_batch_device")

    def track_source_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, d_src_kps, d_src_desc, bounds, th, check_orientation,
                                  d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed, qcap, d_t2pos, d_t2slot, d_nmatches, d_nq,
                                  d_overflow, stream=0):
        """th: TH_HIGH (last frame) or ORBdist (key frame)"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        prm = SearchParams(RULE_BEST, int(th), 0.0, 1 if check_orientation else 0)
        rc = lib().orbp_track_source_batch_device(self.h, d_views, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap, d_skip or None,
                                                  d_src_kps or None, d_src_desc or None, ctypes.byref(bounds), ctypes.byref(prm), d_kps_un, d_desc,
                                                  d_cell_off, d_cell_feat, d_nt, cap, d_claimed or None, qcap, d_t2pos, d_t2slot or None, d_nmatches,
                                                  d_nq, d_overflow, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_track_source_batch_device")

    def track_source(self, view, factors, list, skip, src_kps, src_desc, bounds, th, check_orientation, kps_un, desc, cell_off, cell_feat,
                     claimed=None, nt=None, qcap=None):
        """One view (the latency form): -> dict(t2pos, t2slot, nmatches, nvisible).  list / skip: host arrays.  The source frame (src_kps, src_desc)
        and the current frame (kps_un, desc, cell_off, cell_feat, claimed) are host arrays, or device pointers as ints (each frame all of one kind;
        nt must then be given for the current frame).  Raises OrbxError(ORBX_ERR_CAPACITY) when more than qcap entries project inside."""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        list = np.ascontiguousarray(list, dtype=np.int32)
        nlist = len(list)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            assert len(skip) == nlist
        src_dev = isinstance(src_kps, int)
        if not src_dev:
            src_kps = np.ascontiguousarray(src_kps)
            assert src_kps.dtype.itemsize == 28 and len(src_kps) == nlist
            if src_desc is not None:
                src_desc = np.ascontiguousarray(src_desc, dtype=np.uint8).reshape(nlist, 32)
        frame_dev = isinstance(kps_un, int)
        if not frame_dev:
            kps_un = np.ascontiguousarray(kps_un)
            nt = len(kps_un)
            desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(nt, 32)
            cell_off = np.ascontiguousarray(cell_off, dtype=np.int32)
            cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32)
            assert kps_un.dtype.itemsize == 28 and len(cell_off) == GRID_CELLS + 1
            if claimed is not None:
                claimed = np.ascontiguousarray(claimed, dtype=np.uint8)
        qcap = qcap or max(1, min(nlist, 8192))
        t2pos = np.full(max(nt, 1), -1, np.int32)
        t2slot = np.full(max(nt, 1), -1, np.int32)
        nm, nv = ctypes.c_int(), ctypes.c_int()
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        prm = SearchParams(RULE_BEST, int(th), 0.0, 1 if check_orientation else 0)
        rc = lib().orbp_track_source(self.h, ctypes.byref(view), f.ctypes.data, len(f), ptr(list), nlist, ptr(skip), ptr(src_kps), ptr(src_desc),
                                     1 if src_dev else 0, ctypes.byref(bounds), ctypes.byref(prm), ptr(kps_un), ptr(desc), ptr(cell_off),
                                     ptr(cell_feat), ptr(claimed), nt, 1 if frame_dev else 0, qcap, ptr(t2pos), ptr(t2slot), ctypes.byref(nm),
                                     ctypes.byref(nv), None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_track_source (nvisible=%d)" % nv.value)
        return dict(t2pos=t2pos[:nt], t2slot=t2slot[:nt], nmatches=nm.value, nvisible=nv.value)

    def loop_project_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, d_rec, d_qxyr, d_qlev, d_qdesc, d_qpos, d_nq,
                                  d_overflow, qcap, stream=0):
        """the queries of loop closing's SearchByProjection(pKF, Scw, ...) (view.mode = MODE_LOOP), compacted in list order: device pointers
        as ints (0 = NULL: d_skip, d_rec); d_rec is FUSED_DTYPE"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_loop_project_batch_device(self.h, d_views or None, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap,
                                                  d_skip or None, d_rec or None, d_qxyr or None, d_qlev or None, d_qdesc or None, d_qpos or None,
                                                  d_nq or None, d_overflow or None, qcap, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_loop_project_batch_device")

    def loop_search_batch_device(self, d_views, nviews, factors, d_list, d_nlist, lcap, d_skip, bounds, orb_dist, d_kps_un, d_desc, d_cell_off,
                                 d_cell_feat, d_nt, nframes, cap, d_frame, d_claimed, qcap, d_rec, d_t2pos, d_t2slot, d_nmatches, d_nq, d_overflow,
                                 stream=0):
        """projection, in-order window search (RULE_BEST, orb_dist, no rotation check) and the result by feature; the key frames in the batch
        layout, view p searching row d_frame[p] (0: row p); d_claimed per view"""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        rc = lib().orbp_loop_search_batch_device(self.h, d_views or None, nviews, f.ctypes.data, len(f), d_list or None, d_nlist or None, lcap,
                                                 d_skip or None, ctypes.addressof(bounds), orb_dist, d_kps_un or None, d_desc or None, d_cell_off or None,
                                                 d_cell_feat or None, d_nt or None, nframes, cap, d_frame or None, d_claimed or None, qcap, d_rec or None,
                                                 d_t2pos or None, d_t2slot or None, d_nmatches or None, d_nq or None, d_overflow or None, stream or None)
        if rc != ORBX_OK:
            raise OrbxError(rc, "orbp_loop_search_batch_device")

    def loop_search(self, view, factors, list, skip, bounds, orb_dist, kps_un, desc, cell_off, cell_feat, claimed=None, nt=None, qcap=None,
                    want_records=True):
        """One view (the latency form): -> dict(t2pos, t2slot, nmatches, nvisible, rec).  view: a View or one VIEW_DTYPE record; list / skip /
        claimed: host arrays.  The key frame (kps_un, desc, cell_off, cell_feat) is host arrays, or device pointers as ints (nt must then be
        given).  Raises OrbxError(ORBX_ERR_CAPACITY) when more than qcap entries pass (e.nvisible holds the count)."""
        f = np.ascontiguousarray(factors, dtype=np.float32)
        list = np.ascontiguousarray(list, dtype=np.int32)
        nlist = len(list)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            assert len(skip) == nlist
        frame_dev = isinstance(kps_un, int)
        if not frame_dev:
            kps_un = np.ascontiguousarray(kps_un)
            nt = len(kps_un)
            desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(nt, 32)
            cell_off = np.ascontiguousarray(cell_off, dtype=np.int32)
            cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32)
            assert kps_un.dtype.itemsize == 28 and len(cell_off) == GRID_CELLS + 1
        if claimed is not None:
            claimed = np.ascontiguousarray(claimed, dtype=np.uint8)
            assert len(claimed) == nt
        if isinstance(view, np.ndarray):
            view = np.ascontiguousarray(view, dtype=VIEW_DTYPE).reshape(-1)[:1]
        qcap = qcap or max(1, min(nlist, 8192))
        rec = np.zeros(max(nlist, 1), FUSED_DTYPE) if want_records else None
        t2pos = np.full(max(nt, 1), -1, np.int32)
        t2slot = np.full(max(nt, 1), -1, np.int32)
        nm, nv = ctypes.c_int(), ctypes.c_int()
        ptr = lambda a: (a or None) if isinstance(a, int) else (a.ctypes.data if a is not None else None)
        rc = lib().orbp_loop_search(self.h, ptr(view) if isinstance(view, np.ndarray) else ctypes.addressof(view), f.ctypes.data, len(f), ptr(list), nlist,
                                    ptr(skip), ctypes.addressof(bounds), orb_dist, ptr(kps_un), ptr(desc), ptr(cell_off), ptr(cell_feat), ptr(claimed), nt,
                                    1 if frame_dev else 0, qcap, ptr(rec), ptr(t2pos), ptr(t2slot), ctypes.byref(nm), ctypes.byref(nv), None)
        if rc != ORBX_OK:
            e = OrbxError(rc, "orbp_loop_search (nvisible=%d)" % nv.value)
            e.nvisible = nv.value
            raise e
        return dict(t2pos=t2pos[:nt], t2slot=t2slot[:nt], nmatches=nm.value, nvisible=nv.value, rec=rec[:nlist] if rec is not None else None)
