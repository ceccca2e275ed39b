"""ctypes binding of include/ctag.h (libctag_hip.so).  Plumbing only: no arithmetic happens here."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("CTAG_HIP_LIB") or os.path.join(_HERE, "_build", "libctag_hip.so")  # override: A/B builds (tools/)

MAX_FEATURES, MAX_MARKERS = 100, 100
FEATURE_DT = np.dtype([("pos", "<i4"), ("id", "<i4"), ("id_left", "<i4"), ("id_right", "<i4"),
                       ("corners", "<f4", (16,)), ("center", "<f4", (2,)), ("edge_length", "<f4"),
                       ("cr_left", "<f4"), ("cr_right", "<f4")])
MARKER_DT = np.dtype([("marker_id", "<i4"), ("first_feature", "<i4"), ("n_features", "<i4"), ("n_pos", "<i4")])
RESULT_DT = np.dtype([("status", "<i4"), ("n_markers", "<i4"), ("n_features", "<i4"), ("flags", "<u4"),
                      ("markers", MARKER_DT, (MAX_MARKERS,)), ("features", FEATURE_DT, (MAX_FEATURES,))])
STAGE_NAMES = ["decimate", "threshold_ccl", "seam_merge", "resolve", "candidates", "quad_pack", "quad_edges", "quad_edges_big",
               "line_sort", "welsch", "quad_final", "features", "edge_refine", "markers"]
QUAD_STAGES = ["quad_pack", "quad_edges", "quad_edges_big", "line_sort", "welsch", "quad_final"]  # a4: edgeExtraction

OPT_MAX_CHUNK, OPT_TIMING, OPT_KEEP_PREMARKERS, OPT_HOST_SUBCHUNK, OPT_GRAPH, OPT_WAVE_POINTS, OPT_FUSED_SWEEP, OPT_STREAMS, OPT_EXPAND_EXACT, OPT_BGR_DIRECT = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10

# every symbol include/ctag.h declares (tests check the library exports all of them)
EXPORTS = ["ctag_create", "ctag_create_ex", "ctag_params_default", "ctag_destroy", "ctag_load_marker_file", "ctag_free", "ctag_detect_u8", "ctag_detect_batch_u8",
           "ctag_detect_batch_device", "ctag_detect_bgr8", "ctag_detect_batch_bgr8", "ctag_detect_batch_bgr8_device", "ctag_host_alloc", "ctag_host_free", "ctag_sync", "ctag_stream", "ctag_set_option", "ctag_get_timings", "ctag_get_counters", "ctag_submit_u8", "ctag_collect",
           "ctag_stage_name", "ctag_strerror", "ctag_version"]
# ... and include/ctag_pose.h
POSE_EXPORTS = ["ctag_model_load", "ctag_model_create", "ctag_model_free", "ctag_model_get_view", "ctag_camera_load",
                "ctag_pose_batch_device", "ctag_estimate_pose", "ctag_pose_last_ms", "ctag_draw_axis", "ctag_draw_axis_batch_device",
                "ctag_rigs_create", "ctag_rigs_free", "ctag_rig_pose_batch_device", "ctag_estimate_rig_pose",
                "ctag_camera_set_create", "ctag_camera_set_free", "ctag_mv_rig_pose_batch_device", "ctag_estimate_mv_rig_pose",
                "ctag_cov_opts_default", "ctag_pose_cov_batch_device", "ctag_rig_pose_cov_batch_device", "ctag_mv_rig_pose_cov_batch_device",
                "ctag_estimate_pose_cov", "ctag_estimate_rig_pose_cov", "ctag_estimate_mv_rig_pose_cov",
                "ctag_robust_opts_default", "ctag_pose_robust_batch_device", "ctag_rig_pose_robust_batch_device", "ctag_mv_rig_pose_robust_batch_device",
                "ctag_estimate_pose_robust", "ctag_estimate_rig_pose_robust", "ctag_estimate_mv_rig_pose_robust",
                "ctag_track_opts_default", "ctag_rig_track_smooth_device", "ctag_mv_rig_track_smooth_device", "ctag_rig_track_smooth",
                "ctag_mv_rig_track_smooth", "ctag_track_last_ms",
                "ctag_track_filter_opts_default", "ctag_track_filter_create", "ctag_track_filter_free", "ctag_track_filter_reset",
                "ctag_rig_track_filter_device", "ctag_mv_rig_track_filter_device", "ctag_rig_track_filter", "ctag_mv_rig_track_filter",
                "ctag_track_filter_predict_device", "ctag_track_filter_predict", "ctag_track_filter_last_ms", "ctag_track_filter_set_cov_scale",
                "ctag_track_noise_opts_default", "ctag_rig_track_noise_fit_device", "ctag_mv_rig_track_noise_fit_device", "ctag_rig_track_noise_fit",
                "ctag_mv_rig_track_noise_fit", "ctag_rig_track_noise_score_device", "ctag_mv_rig_track_noise_score_device",
                "ctag_rig_track_noise_score", "ctag_mv_rig_track_noise_score", "ctag_track_noise_last_ms",
                "ctag_hand_eye_opts_default", "ctag_rig_hand_eye_fit_device", "ctag_mv_rig_hand_eye_fit_device", "ctag_rig_hand_eye_fit",
                "ctag_mv_rig_hand_eye_fit", "ctag_hand_eye_last_ms",
                "ctag_model_fit_opts_default", "ctag_model_fit_device", "ctag_model_fit", "ctag_model_save", "ctag_model_fit_last_ms",
                "ctag_rig_fit_opts_default", "ctag_rig_fit_device", "ctag_rig_fit", "ctag_rig_fit_last_ms",
                "ctag_camera_fit_opts_default", "ctag_camera_fit_device", "ctag_camera_fit", "ctag_camera_fit_last_ms", "ctag_camera_set_get",
                "ctag_intrinsics_fit_opts_default", "ctag_intrinsics_fit_device", "ctag_intrinsics_fit", "ctag_intrinsics_fit_last_ms"]
# ... and include/ctag_gather.h
GATHER_EXPORTS = ["ctag_shard_range", "ctag_packed_capacity", "ctag_pack_results", "ctag_unpack_results", "ctag_comm_unique_id",
                  "ctag_comm_init", "ctag_comm_attach", "ctag_comm_destroy", "ctag_comm_native", "ctag_comm_last_error", "ctag_gather_begin",
                  "ctag_gather_end", "ctag_gather_wait", "ctag_gather", "ctag_gather_set_timeout", "ctag_gather_last_bytes"]
EXPORTS = EXPORTS + POSE_EXPORTS + GATHER_EXPORTS
COMM_ID_BYTES = 128

POSE_DT = np.dtype([("status", "<i4"), ("model_index", "<i4"), ("frame", "<i4"), ("marker", "<i4"),
                    ("n_points", "<i4"), ("iterations", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)),
                    ("rvec0", "<f8", (3,)), ("tvec0", "<f8", (3,)), ("cost0", "<f8"), ("cost", "<f8")])
POSE_OK, POSE_NO_MODEL, POSE_TOO_FEW, POSE_BAD_POS, POSE_DEGENERATE, POSE_NOT_SEEN = range(6)
# ctag_rig_pose_rec: one pose per rig of markers (include/ctag_pose.h)
RIG_POSE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("n_members", "<i4"), ("n_excluded", "<i4"),
                        ("n_points", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"), ("member_mask", "<u4", (4,)),
                        ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("rvec0", "<f8", (3,)), ("tvec0", "<f8", (3,)),
                        ("cost0", "<f8"), ("cost", "<f8")])
RIG_MAX_POINTS = 800
# ctag_mv_pose_rec: one pose per rig from several cameras (include/ctag_pose.h)
MV_MAX_CAMERAS = 8
MV_POSE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("n_cameras", "<i4"), ("start_camera", "<i4"),
                       ("n_members", "<i4"), ("n_excluded", "<i4"), ("n_points", "<i4"), ("iterations", "<i4"), ("iterations_cam", "<i4"),
                       ("points_of_camera", "<i4", (MV_MAX_CAMERAS,)), ("member_mask", "<u4", (MV_MAX_CAMERAS, 4)), ("reserved", "<i4", (2,)),
                       ("rvec_epnp", "<f8", (3,)), ("tvec_epnp", "<f8", (3,)), ("rvec_cam", "<f8", (3,)), ("tvec_cam", "<f8", (3,)),
                       ("cost_cam0", "<f8"), ("cost_cam", "<f8"), ("rvec_start", "<f8", (3,)), ("tvec_start", "<f8", (3,)), ("cost0", "<f8"),
                       ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("cost", "<f8")])
assert MV_POSE_DT.itemsize == 432
# ctag_pose_cov_rec: the covariance and residual diagnostics of one pose record of any kind (include/ctag_pose.h)
POSE_COV_DT = np.dtype([("status", "<i4"), ("n_points", "<i4"), ("dof", "<i4"), ("worst_point", "<i4"), ("n_outliers", "<i4"), ("param", "<i4"),
                        ("cost", "<f8"), ("sigma2_hat", "<f8"), ("sigma2_used", "<f8"), ("max_residual_px", "<f8"), ("min_pivot", "<f8"),
                        ("cov", "<f8", (6, 6))])
assert POSE_COV_DT.itemsize == 352
COV_OK, COV_NO_POSE, COV_BAD_RECORD, COV_SINGULAR = range(4)
COV_PARAM_TANGENT, COV_PARAM_RVEC = 0, 1
# ctag_robust_pose_rec: one pose record of any kind minimised again under a loss (include/ctag_pose.h, robust refit)
ROBUST_POSE_DT = np.dtype([("status", "<i4"), ("n_points", "<i4"), ("n_inliers", "<i4"), ("iterations", "<i4"), ("loss", "<i4"), ("worst_point", "<i4"),
                           ("inlier_mask", "<u4", (25,)), ("reserved", "<i4"), ("scale_px", "<f8"), ("sigma_hat", "<f8"), ("cost_ls0", "<f8"),
                           ("cost_ls", "<f8"), ("cost0", "<f8"), ("cost", "<f8"), ("max_residual_px", "<f8"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert ROBUST_POSE_DT.itemsize == 232
ROBUST_OK, ROBUST_NO_POSE, ROBUST_BAD_RECORD, ROBUST_DEGENERATE = range(4)
LOSS_HUBER, LOSS_CAUCHY = 0, 1
# ctag_track_rec / ctag_track_stat: one record per (frame, rig) / per rig of a track smoothing (include/ctag_pose.h)
TRACK_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("flags", "<u4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)),
                     ("w", "<f8", (3,)), ("v", "<f8", (3,)), ("cov", "<f8", (6, 6)), ("vel_sigma", "<f8", (6,)), ("mahalanobis2", "<f8"),
                     ("weight", "<f8")])
assert TRACK_DT.itemsize == 464
TRACK_STAT_DT = np.dtype([("status", "<i4"), ("n_measured", "<i4"), ("n_pieces", "<i4"), ("n_tracked", "<i4"), ("longest_piece", "<i4"),
                          ("rounds", "<i4"), ("cost0", "<f8"), ("cost", "<f8")])
assert TRACK_STAT_DT.itemsize == 40
TRACK_OK, TRACK_NOT_TRACKED, TRACK_BAD_INPUT, TRACK_SINGULAR = range(4)
TRACK_LOSS_NONE = 2
TRACK_MAX_ITEMS = 65536
TRACK_FLAG_MEASURED, TRACK_FLAG_DOWNWEIGHTED, TRACK_FLAG_GATED, TRACK_FLAG_STARTED = 1, 2, 4, 8
# ctag_track_noise_rec / _round / _score: the track noise fit's result, trace row and score entry (include/ctag_pose.h)
TRACK_NOISE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("n_terms", "<i4"), ("n_free", "<i4"), ("rounds", "<i4"), ("flags", "<u4"),
                           ("q_rot", "<f8"), ("q_trans", "<f8"), ("cov_scale", "<f8"), ("log2_sigma", "<f8", (3,)), ("score", "<f8"),
                           ("score_start", "<f8"), ("mean_m2", "<f8")])
assert TRACK_NOISE_DT.itemsize == 96
TRACK_NOISE_ROUND_DT = np.dtype([("u", "<f8", (3,)), ("value", "<f8", (3,)), ("L", "<f8"), ("winner", "<i4"), ("reserved", "<i4")])
assert TRACK_NOISE_ROUND_DT.itemsize == 64
TRACK_NOISE_SCORE_DT = np.dtype([("L", "<f8"), ("sum_m2", "<f8"), ("n_terms", "<i4"), ("n_singular", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
assert TRACK_NOISE_SCORE_DT.itemsize == 32
NOISE_OK, NOISE_BAD_INPUT, NOISE_TOO_FEW, NOISE_SINGULAR = range(4)
NOISE_PER_RIG, NOISE_POOLED = 0, 1
NOISE_FREE_Q_ROT, NOISE_FREE_Q_TRANS, NOISE_FREE_COV_SCALE = 1, 2, 4
NOISE_FLAG_EDGE = 1
NOISE_MAX_SCORE_CAND = 64
# ctag_link_pose / ctag_hand_eye_rec / ctag_hand_eye_frame_rec: a link pose per frame in, one record per rig and one per (frame, rig) out of a
# hand-eye calibration (include/ctag_pose.h)
LINK_POSE_DT = np.dtype([("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert LINK_POSE_DT.itemsize == 48
HAND_EYE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("n_used", "<i4"), ("n_downweighted", "<i4"), ("rounds", "<i4"), ("dof", "<i4"),
                        ("P", LINK_POSE_DT), ("Q", LINK_POSE_DT), ("cost0", "<f8"), ("cost", "<f8"), ("lambda", "<f8"), ("sigma2_hat", "<f8"),
                        ("min_pivot", "<f8"), ("cov", "<f8", (12, 12))])
assert HAND_EYE_DT.itemsize == 1312
HAND_EYE_FRAME_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("flags", "<u4"), ("e", "<f8", (6,)), ("mahalanobis2", "<f8"),
                              ("weight", "<f8")])
assert HAND_EYE_FRAME_DT.itemsize == 80
HE_OK, HE_TOO_FEW, HE_BAD_INPUT, HE_SINGULAR = range(4)
HAND_EYE_CAMERA_ON_LINK, HAND_EYE_RIG_ON_LINK = 0, 1
HAND_EYE_MAX_ITEMS = 65536
HE_FLAG_USED, HE_FLAG_DOWNWEIGHTED = 1, 2
# ctag_model_fit_stat: one record per model of a model reconstruction (include/ctag_pose.h)
MODEL_FIT_STAT_DT = np.dtype([("status", "<i4"), ("n_records", "<i4"), ("n_points_fitted", "<i4"), ("n_points_held", "<i4"), ("rounds", "<i4"),
                              ("reserved", "<i4"), ("cost0", "<f8"), ("cost", "<f8"), ("lambda", "<f8"), ("rms_px", "<f8")])
assert MODEL_FIT_STAT_DT.itemsize == 56
# ctag_rig_fit_stat / ctag_rig_fit_model_stat: one record per rig / per model of a rig assembly (include/ctag_pose.h)
RIG_FIT_MAX_MODELS = 16
RIG_FIT_STAT_DT = np.dtype([("status", "<i4"), ("anchor", "<i4"), ("n_placed", "<i4"), ("n_unplaced", "<i4"), ("n_records", "<i4"), ("n_points", "<i4"),
                            ("rounds", "<i4"), ("reserved", "<i4"), ("cost_init", "<f8"), ("cost", "<f8"), ("lambda", "<f8"), ("rms_px", "<f8")])
assert RIG_FIT_STAT_DT.itemsize == 64
RIG_FIT_MODEL_STAT_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("parent", "<i4"), ("n_frames_with_parent", "<i4"), ("n_records", "<i4"),
                                  ("reserved", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert RIG_FIT_MODEL_STAT_DT.itemsize == 72
# ctag_camera_fit_stat / ctag_camera_fit_cam_stat: one record per call / per camera of a camera set fit (include/ctag_pose.h)
CAMERA_FIT_STAT_DT = np.dtype([("status", "<i4"), ("anchor", "<i4"), ("n_placed", "<i4"), ("n_unplaced", "<i4"), ("n_records", "<i4"), ("n_points", "<i4"),
                               ("rounds", "<i4"), ("reserved", "<i4"), ("cost_init", "<f8"), ("cost", "<f8"), ("lambda", "<f8"), ("rms_px", "<f8")])
assert CAMERA_FIT_STAT_DT.itemsize == 64
CAMERA_FIT_CAM_STAT_DT = np.dtype([("status", "<i4"), ("parent", "<i4"), ("n_items_with_parent", "<i4"), ("n_records", "<i4"), ("n_points", "<i4"),
                                   ("reserved", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert CAMERA_FIT_CAM_STAT_DT.itemsize == 72
# ctag_intrinsics_fit_stat: one record per intrinsics fit (include/ctag_pose.h); parameter order fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
INTR_PARAMS = 16
INTR_PARAM_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "s1", "s2", "s3", "s4")
INTRINSICS_FIT_STAT_DT = np.dtype([("status", "<i4"), ("n_records", "<i4"), ("n_points", "<i4"), ("n_free", "<i4"), ("rounds", "<i4"), ("free_mask", "<u4"),
                                   ("cost0", "<f8"), ("cost", "<f8"), ("lambda", "<f8"), ("rms_px", "<f8"), ("sigma2_hat", "<f8"), ("pose_cost", "<f8"),
                                   ("sigma", "<f8", (INTR_PARAMS,))])
assert INTRINSICS_FIT_STAT_DT.itemsize == 200


class ParamsC(C.Structure):  # ctag_params (include/ctag_types.h): the reference's tunables
    _fields_ = [("struct_size", C.c_uint32), ("threshold_line", C.c_float), ("threshold_expand", C.c_float), ("threshold_RAC", C.c_float), ("threshold_angle", C.c_float),
                ("threshold_vertical", C.c_float), ("ID_cr_correspond", C.c_float * 4), ("cr_covariance_left", C.c_float * 4),
                ("cr_covariance_right", C.c_float * 4), ("dark_cap", C.c_float), ("area_min", C.c_int32), ("area_max_fraction", C.c_double),
                ("collinear_cost", C.c_double)]


def default_params():
    """ctag_params_default: the reference's values (header/corner_detector.h:90,110,122,135-137,144; corner_detector.cpp:71,88,285)."""
    p = ParamsC()
    load_library().ctag_params_default(C.byref(p))
    return p


COUNTER_NAMES = ["components", "candidates", "quads", "features", "markers"]
PENDING = -5  # CTAG_PENDING
ERR_ARG, ERR_HIP, ERR_LIMIT, ERR_UNSUPPORTED = -1, -2, -3, -4  # include/ctag_types.h


class CountersC(C.Structure):  # ctag_counters (include/ctag_types.h)
    _fields_ = [("frames", C.c_int64), ("sum", C.c_int64 * 5), ("max", C.c_int32 * 5), ("reruns", C.c_int32)]


class CameraC(C.Structure):  # ctag_camera
    _fields_ = [("K", C.c_float * 9), ("dist", C.c_float * 14), ("n_dist", C.c_int32)]


class CameraPoseC(C.Structure):  # ctag_camera_pose: X_cam = R(rvec) X_ref + tvec
    _fields_ = [("rvec", C.c_double * 3), ("tvec", C.c_double * 3)]


class CovOptsC(C.Structure):  # ctag_cov_opts
    _fields_ = [("struct_size", C.c_uint32), ("param", C.c_int32), ("sigma_px", C.c_double), ("outlier_k", C.c_double)]


def cov_opts(param=None, sigma_px=None, outlier_k=None):
    """ctag_cov_opts_default, then the given fields."""
    o = CovOptsC()
    load_library().ctag_cov_opts_default(C.byref(o))
    if param is not None:
        o.param = int(param)
    if sigma_px is not None:
        o.sigma_px = float(sigma_px)
    if outlier_k is not None:
        o.outlier_k = float(outlier_k)
    return o


class RobustOptsC(C.Structure):  # ctag_robust_opts
    _fields_ = [("struct_size", C.c_uint32), ("loss", C.c_int32), ("max_iterations", C.c_int32), ("reserved", C.c_int32), ("scale_px", C.c_double),
                ("auto_k", C.c_double), ("min_scale_px", C.c_double)]


def robust_opts(loss=None, max_iterations=None, scale_px=None, auto_k=None, min_scale_px=None):
    """ctag_robust_opts_default, then the given fields."""
    o = RobustOptsC()
    load_library().ctag_robust_opts_default(C.byref(o))
    if loss is not None:
        o.loss = int(loss)
    if max_iterations is not None:
        o.max_iterations = int(max_iterations)
    for k, v in (("scale_px", scale_px), ("auto_k", auto_k), ("min_scale_px", min_scale_px)):
        if v is not None:
            setattr(o, k, float(v))
    return o


class TrackOptsC(C.Structure):  # ctag_track_opts
    _fields_ = [("struct_size", C.c_uint32), ("loss", C.c_int32), ("max_iterations", C.c_int32), ("max_gap", C.c_int32), ("segment_frames", C.c_int32),
                ("reserved", C.c_int32), ("dt", C.c_double), ("q_rot", C.c_double), ("q_trans", C.c_double), ("vel0_sigma_rot", C.c_double),
                ("vel0_sigma_trans", C.c_double), ("loss_scale", C.c_double), ("lambda0", C.c_double)]


def track_opts(**fields):
    """ctag_track_opts_default, then the given fields."""
    o = TrackOptsC()
    load_library().ctag_track_opts_default(C.byref(o))
    for k, v in fields.items():
        if k in ("loss", "max_iterations", "max_gap", "segment_frames", "struct_size"):
            setattr(o, k, int(v))
        elif k in ("dt", "q_rot", "q_trans", "vel0_sigma_rot", "vel0_sigma_trans", "loss_scale", "lambda0"):
            setattr(o, k, float(v))
        else:
            raise TypeError("ctag_track_opts has no field %r" % k)
    return o


class TrackFilterOptsC(C.Structure):  # ctag_track_filter_opts
    _fields_ = [("struct_size", C.c_uint32), ("loss", C.c_int32), ("max_gap", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double),
                ("q_rot", C.c_double), ("q_trans", C.c_double), ("vel0_sigma_rot", C.c_double), ("vel0_sigma_trans", C.c_double),
                ("loss_scale", C.c_double), ("gate", C.c_double)]


def track_filter_opts(**fields):
    """ctag_track_filter_opts_default, then the given fields."""
    o = TrackFilterOptsC()
    load_library().ctag_track_filter_opts_default(C.byref(o))
    for k, v in fields.items():
        if k in ("loss", "max_gap", "struct_size"):
            setattr(o, k, int(v))
        elif k in ("dt", "q_rot", "q_trans", "vel0_sigma_rot", "vel0_sigma_trans", "loss_scale", "gate"):
            setattr(o, k, float(v))
        else:
            raise TypeError("ctag_track_filter_opts has no field %r" % k)
    return o


class TrackNoiseOptsC(C.Structure):  # ctag_track_noise_opts
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("free_mask", C.c_int32), ("rounds", C.c_int32), ("max_gap", C.c_int32),
                ("min_terms", C.c_int32), ("dt", C.c_double), ("q_rot", C.c_double), ("q_trans", C.c_double), ("cov_scale", C.c_double),
                ("vel0_sigma_rot", C.c_double), ("vel0_sigma_trans", C.c_double), ("span", C.c_double)]


def track_noise_opts(**fields):
    """ctag_track_noise_opts_default, then the given fields."""
    o = TrackNoiseOptsC()
    load_library().ctag_track_noise_opts_default(C.byref(o))
    for k, v in fields.items():
        if k in ("mode", "free_mask", "rounds", "max_gap", "min_terms", "struct_size"):
            setattr(o, k, int(v))
        elif k in ("dt", "q_rot", "q_trans", "cov_scale", "vel0_sigma_rot", "vel0_sigma_trans", "span"):
            setattr(o, k, float(v))
        else:
            raise TypeError("ctag_track_noise_opts has no field %r" % k)
    return o


def apply_track_noise(rec, **over):
    """A fitted TRACK_NOISE_DT record -> (track_filter_opts with its q_rot and q_trans and the fields of `over`, cov_scale): the options to
    create a filter with and the scale to give its set_cov_scale."""
    rec = np.asarray(rec, TRACK_NOISE_DT).reshape(-1)
    if len(rec) != 1:
        raise ValueError("apply_track_noise: one record, got %d" % len(rec))
    fields = dict(q_rot=float(rec["q_rot"][0]), q_trans=float(rec["q_trans"][0]))
    fields.update(over)
    return track_filter_opts(**fields), float(rec["cov_scale"][0])


class HandEyeOptsC(C.Structure):  # ctag_hand_eye_opts
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("loss", C.c_int32), ("max_iterations", C.c_int32), ("loss_scale", C.c_double),
                ("lambda0", C.c_double)]


def hand_eye_opts(**fields):
    """ctag_hand_eye_opts_default, then the given fields."""
    o = HandEyeOptsC()
    load_library().ctag_hand_eye_opts_default(C.byref(o))
    for k, v in fields.items():
        if k in ("mode", "loss", "max_iterations", "struct_size"):
            setattr(o, k, int(v))
        elif k in ("loss_scale", "lambda0"):
            setattr(o, k, float(v))
        else:
            raise TypeError("ctag_hand_eye_opts has no field %r" % k)
    return o


def apply_robust(pose_records, robust_records):
    """A copy of the pose records (POSE_DT, RIG_POSE_DT or MV_POSE_DT) with rvec, tvec replaced by the refit's where the robust record's
    status is ROBUST_OK: what the covariance and overlay calls take in place of the least-squares poses."""
    poses = np.array(pose_records, copy=True)
    rob = np.asarray(robust_records)
    if rob.dtype != ROBUST_POSE_DT or rob.shape != poses.shape or "rvec" not in (poses.dtype.names or ()):
        raise ValueError("apply_robust: one ROBUST_POSE_DT record per pose record")
    ok = rob["status"] == ROBUST_OK
    poses["rvec"][ok] = rob["rvec"][ok]
    poses["tvec"][ok] = rob["tvec"][ok]
    return poses


class ModelFitOptsC(C.Structure):  # ctag_model_fit_opts
    _fields_ = [("max_rounds", C.c_int32), ("min_obs", C.c_int32), ("lambda0", C.c_double), ("lambda_max", C.c_double), ("rel_tol", C.c_double),
                ("strip_height", C.c_double)]


def model_fit_opts(**fields):
    """ctag_model_fit_opts_default, then the given fields."""
    o = ModelFitOptsC()
    load_library().ctag_model_fit_opts_default(C.byref(o))
    for k, v in fields.items():
        if k not in ("max_rounds", "min_obs", "lambda0", "lambda_max", "rel_tol", "strip_height"):
            raise TypeError("ctag_model_fit_opts has no field %r" % k)
        setattr(o, k, v)
    return o


class RigFitOptsC(C.Structure):  # ctag_rig_fit_opts
    _fields_ = [("max_rounds", C.c_int32), ("min_frames", C.c_int32), ("lambda0", C.c_double), ("lambda_max", C.c_double), ("rel_tol", C.c_double)]


def rig_fit_opts(**fields):
    """ctag_rig_fit_opts_default, then the given fields."""
    o = RigFitOptsC()
    load_library().ctag_rig_fit_opts_default(C.byref(o))
    for k, v in fields.items():
        if k not in ("max_rounds", "min_frames", "lambda0", "lambda_max", "rel_tol"):
            raise TypeError("ctag_rig_fit_opts has no field %r" % k)
        setattr(o, k, v)
    return o


class CameraFitOptsC(C.Structure):  # ctag_camera_fit_opts
    _fields_ = [("max_rounds", C.c_int32), ("min_items", C.c_int32), ("min_points", C.c_int32), ("reserved", C.c_int32), ("lambda0", C.c_double),
                ("lambda_max", C.c_double), ("rel_tol", C.c_double)]


def camera_fit_opts(**fields):
    """ctag_camera_fit_opts_default, then the given fields."""
    o = CameraFitOptsC()
    load_library().ctag_camera_fit_opts_default(C.byref(o))
    for k, v in fields.items():
        if k not in ("max_rounds", "min_items", "min_points", "lambda0", "lambda_max", "rel_tol"):
            raise TypeError("ctag_camera_fit_opts has no field %r" % k)
        setattr(o, k, v)
    return o


class IntrinsicsFitOptsC(C.Structure):  # ctag_intrinsics_fit_opts
    _fields_ = [("max_rounds", C.c_int32), ("min_points", C.c_int32), ("free_mask", C.c_uint32), ("tie_focal", C.c_int32), ("lambda0", C.c_double),
                ("lambda_max", C.c_double), ("rel_tol", C.c_double)]


def intrinsics_fit_opts(**fields):
    """ctag_intrinsics_fit_opts_default, then the given fields."""
    o = IntrinsicsFitOptsC()
    load_library().ctag_intrinsics_fit_opts_default(C.byref(o))
    for k, v in fields.items():
        if k not in ("max_rounds", "min_points", "free_mask", "tie_focal", "lambda0", "lambda_max", "rel_tol"):
            raise TypeError("ctag_intrinsics_fit_opts has no field %r" % k)
        setattr(o, k, v)
    return o


class ModelViewC(C.Structure):  # ctag_model_view
    _fields_ = [("n_models", C.c_int32), ("model_size", C.c_int32), ("marker_id", C.POINTER(C.c_int32)),
                ("base", C.POINTER(C.c_float)), ("axis", C.POINTER(C.c_float)), ("corners", C.POINTER(C.c_float))]


class CtagError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__("%s (status %d)%s" % (_strerror(status), status, (": " + what) if what else ""))


def lib_path():
    return _LIB


def build(verbose=False):
    """Compile the HIP library in-tree (hipcc cross-compiles for gfx950 without a GPU)."""
    subprocess.check_call(["make", "-C", _HERE, "-j4"] + ([] if verbose else ["-s"]))


_lib = None


def load_library():
    """Load libctag_hip.so; raises if it has not been built.  There is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    try:  # torch wheels bundle their own libamdhip64: let it load first so the process holds ONE HIP runtime
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(_LIB):
        raise FileNotFoundError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(the detection path has no CPU fallback)" % _LIB)
    L = C.CDLL(_LIB)
    vp, i32p, u8p = C.c_void_p, C.POINTER(C.c_int32), C.c_void_p
    L.ctag_create.restype = C.c_int
    L.ctag_create.argtypes = [i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.ctag_create_ex.restype = C.c_int
    L.ctag_create_ex.argtypes = [i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ParamsC), C.POINTER(vp)]
    L.ctag_params_default.restype = None
    L.ctag_params_default.argtypes = [C.POINTER(ParamsC)]
    L.ctag_destroy.argtypes = [vp]
    L.ctag_destroy.restype = None
    L.ctag_load_marker_file.restype = C.c_int
    L.ctag_load_marker_file.argtypes = [C.c_char_p, C.POINTER(i32p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
    L.ctag_free.argtypes = [vp]
    L.ctag_free.restype = None
    L.ctag_detect_u8.restype = C.c_int
    L.ctag_detect_u8.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_int, C.c_int, vp]
    L.ctag_detect_batch_u8.restype = C.c_int
    L.ctag_detect_batch_u8.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_int,
                                       C.c_int, vp]
    L.ctag_detect_batch_device.restype = C.c_int
    L.ctag_detect_batch_device.argtypes = L.ctag_detect_batch_u8.argtypes
    L.ctag_detect_bgr8.restype = C.c_int
    L.ctag_detect_bgr8.argtypes = L.ctag_detect_u8.argtypes
    L.ctag_detect_batch_bgr8.restype = C.c_int
    L.ctag_detect_batch_bgr8.argtypes = L.ctag_detect_batch_u8.argtypes
    L.ctag_detect_batch_bgr8_device.restype = C.c_int
    L.ctag_detect_batch_bgr8_device.argtypes = L.ctag_detect_batch_u8.argtypes
    L.ctag_host_alloc.restype = vp
    L.ctag_host_alloc.argtypes = [C.c_size_t]
    L.ctag_host_free.restype = None
    L.ctag_host_free.argtypes = [vp]
    L.ctag_sync.restype = C.c_int
    L.ctag_sync.argtypes = [vp]
    L.ctag_stream.restype = vp
    L.ctag_stream.argtypes = [vp]
    L.ctag_set_option.restype = C.c_int
    L.ctag_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.ctag_submit_u8.restype = C.c_int
    L.ctag_submit_u8.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_int, C.c_int]
    L.ctag_collect.restype = C.c_int
    L.ctag_collect.argtypes = [vp, vp]
    L.ctag_get_counters.restype = C.c_int
    L.ctag_get_counters.argtypes = [vp, C.POINTER(CountersC)]
    L.ctag_get_timings.restype = C.c_int
    L.ctag_get_timings.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    L.ctag_stage_name.restype = C.c_char_p
    L.ctag_stage_name.argtypes = [C.c_int]
    L.ctag_strerror.restype = C.c_char_p
    L.ctag_strerror.argtypes = [C.c_int]
    L.ctag_version.restype = C.c_int
    L.ctag_model_load.restype = C.c_int
    L.ctag_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.ctag_model_create.restype = C.c_int
    L.ctag_model_create.argtypes = [C.POINTER(ModelViewC), C.POINTER(vp)]
    L.ctag_model_free.restype = None
    L.ctag_model_free.argtypes = [vp]
    L.ctag_model_get_view.restype = C.c_int
    L.ctag_model_get_view.argtypes = [vp, C.POINTER(ModelViewC)]
    L.ctag_camera_load.restype = C.c_int
    L.ctag_camera_load.argtypes = [C.c_char_p, C.POINTER(CameraC)]
    L.ctag_pose_batch_device.restype = C.c_int
    L.ctag_pose_batch_device.argtypes = [vp, vp, C.c_int, vp, C.POINTER(CameraC), vp, vp, C.c_int]
    L.ctag_estimate_pose.restype = C.c_int
    L.ctag_estimate_pose.argtypes = [vp, vp, vp, C.POINTER(CameraC), vp]
    L.ctag_pose_last_ms.restype = C.c_float
    L.ctag_pose_last_ms.argtypes = [vp]
    L.ctag_draw_axis.restype = C.c_int
    L.ctag_draw_axis.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t, vp, vp, C.c_int, vp, C.POINTER(CameraC), C.c_int, vp, C.c_ssize_t]
    L.ctag_draw_axis_batch_device.restype = C.c_int
    L.ctag_draw_axis_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, vp, vp, vp, C.c_int, vp,
                                              C.POINTER(CameraC), C.c_int, vp, C.c_ssize_t, C.c_ssize_t]
    L.ctag_rigs_create.restype = C.c_int
    L.ctag_rigs_create.argtypes = [vp, i32p, C.c_int, C.POINTER(vp)]
    L.ctag_rigs_free.restype = None
    L.ctag_rigs_free.argtypes = [vp]
    L.ctag_rig_pose_batch_device.restype = C.c_int
    L.ctag_rig_pose_batch_device.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(CameraC), vp]
    L.ctag_estimate_rig_pose.restype = C.c_int
    L.ctag_estimate_rig_pose.argtypes = [vp, vp, vp, vp, C.POINTER(CameraC), vp]
    L.ctag_camera_set_create.restype = C.c_int
    L.ctag_camera_set_create.argtypes = [C.POINTER(CameraC), C.POINTER(CameraPoseC), C.c_int, C.POINTER(vp)]
    L.ctag_camera_set_free.restype = None
    L.ctag_camera_set_free.argtypes = [vp]
    L.ctag_mv_rig_pose_batch_device.restype = C.c_int
    L.ctag_mv_rig_pose_batch_device.argtypes = [vp, C.POINTER(vp), C.c_int, vp, vp, vp, vp]
    L.ctag_estimate_mv_rig_pose.restype = C.c_int
    L.ctag_estimate_mv_rig_pose.argtypes = [vp, vp, vp, vp, vp, vp]
    optp = C.POINTER(CovOptsC)
    L.ctag_cov_opts_default.restype = None
    L.ctag_cov_opts_default.argtypes = [optp]
    L.ctag_pose_cov_batch_device.restype = C.c_int
    L.ctag_pose_cov_batch_device.argtypes = [vp, vp, C.c_int, vp, C.POINTER(CameraC), vp, vp, C.c_int, optp, vp]
    L.ctag_rig_pose_cov_batch_device.restype = C.c_int
    L.ctag_rig_pose_cov_batch_device.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(CameraC), vp, optp, vp]
    L.ctag_mv_rig_pose_cov_batch_device.restype = C.c_int
    L.ctag_mv_rig_pose_cov_batch_device.argtypes = [vp, C.POINTER(vp), C.c_int, vp, vp, vp, vp, optp, vp]
    L.ctag_estimate_pose_cov.restype = C.c_int
    L.ctag_estimate_pose_cov.argtypes = [vp, vp, vp, C.POINTER(CameraC), vp, optp, vp]
    L.ctag_estimate_rig_pose_cov.restype = C.c_int
    L.ctag_estimate_rig_pose_cov.argtypes = [vp, vp, vp, vp, C.POINTER(CameraC), vp, optp, vp]
    L.ctag_estimate_mv_rig_pose_cov.restype = C.c_int
    L.ctag_estimate_mv_rig_pose_cov.argtypes = [vp, vp, vp, vp, vp, vp, optp, vp]
    optp = C.POINTER(RobustOptsC)
    L.ctag_robust_opts_default.restype = None
    L.ctag_robust_opts_default.argtypes = [optp]
    L.ctag_pose_robust_batch_device.restype = C.c_int
    L.ctag_pose_robust_batch_device.argtypes = [vp, vp, C.c_int, vp, C.POINTER(CameraC), vp, vp, C.c_int, optp, vp]
    L.ctag_rig_pose_robust_batch_device.restype = C.c_int
    L.ctag_rig_pose_robust_batch_device.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(CameraC), vp, optp, vp]
    L.ctag_mv_rig_pose_robust_batch_device.restype = C.c_int
    L.ctag_mv_rig_pose_robust_batch_device.argtypes = [vp, C.POINTER(vp), C.c_int, vp, vp, vp, vp, optp, vp]
    L.ctag_estimate_pose_robust.restype = C.c_int
    L.ctag_estimate_pose_robust.argtypes = [vp, vp, vp, C.POINTER(CameraC), vp, optp, vp]
    L.ctag_estimate_rig_pose_robust.restype = C.c_int
    L.ctag_estimate_rig_pose_robust.argtypes = [vp, vp, vp, vp, C.POINTER(CameraC), vp, optp, vp]
    L.ctag_estimate_mv_rig_pose_robust.restype = C.c_int
    L.ctag_estimate_mv_rig_pose_robust.argtypes = [vp, vp, vp, vp, vp, vp, optp, vp]
    trkp = C.POINTER(TrackOptsC)
    L.ctag_track_opts_default.restype = None
    L.ctag_track_opts_default.argtypes = [trkp]
    for fn in (L.ctag_rig_track_smooth_device, L.ctag_mv_rig_track_smooth_device, L.ctag_rig_track_smooth, L.ctag_mv_rig_track_smooth):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, vp, vp, C.c_int, vp, trkp, vp, vp]
    L.ctag_track_last_ms.restype = C.c_int
    L.ctag_track_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    tfp = C.POINTER(TrackFilterOptsC)
    L.ctag_track_filter_opts_default.restype = None
    L.ctag_track_filter_opts_default.argtypes = [tfp]
    L.ctag_track_filter_create.restype = C.c_int
    L.ctag_track_filter_create.argtypes = [vp, vp, tfp, C.POINTER(vp)]
    L.ctag_track_filter_free.restype = None
    L.ctag_track_filter_free.argtypes = [vp]
    L.ctag_track_filter_reset.restype = C.c_int
    L.ctag_track_filter_reset.argtypes = [vp]
    for fn in (L.ctag_rig_track_filter_device, L.ctag_mv_rig_track_filter_device, L.ctag_rig_track_filter, L.ctag_mv_rig_track_filter):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    for fn in (L.ctag_track_filter_predict_device, L.ctag_track_filter_predict):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_double, vp]
    L.ctag_track_filter_last_ms.restype = C.c_int
    L.ctag_track_filter_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ctag_track_filter_set_cov_scale.restype = C.c_int
    L.ctag_track_filter_set_cov_scale.argtypes = [vp, C.c_double]
    tnp = C.POINTER(TrackNoiseOptsC)
    L.ctag_track_noise_opts_default.restype = None
    L.ctag_track_noise_opts_default.argtypes = [tnp]
    for fn in (L.ctag_rig_track_noise_fit_device, L.ctag_mv_rig_track_noise_fit_device, L.ctag_rig_track_noise_fit, L.ctag_mv_rig_track_noise_fit):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, vp, vp, C.c_int, vp, tnp, vp, vp]
    for fn in (L.ctag_rig_track_noise_score_device, L.ctag_mv_rig_track_noise_score_device, L.ctag_rig_track_noise_score, L.ctag_mv_rig_track_noise_score):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, vp, vp, C.c_int, vp, tnp, vp, C.c_int, vp]
    L.ctag_track_noise_last_ms.restype = C.c_int
    L.ctag_track_noise_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    hep = C.POINTER(HandEyeOptsC)
    L.ctag_hand_eye_opts_default.restype = None
    L.ctag_hand_eye_opts_default.argtypes = [hep]
    for fn in (L.ctag_rig_hand_eye_fit_device, L.ctag_mv_rig_hand_eye_fit_device, L.ctag_rig_hand_eye_fit, L.ctag_mv_rig_hand_eye_fit):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, vp, vp, C.c_int, vp, hep, vp, vp]
    L.ctag_hand_eye_last_ms.restype = C.c_int
    L.ctag_hand_eye_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    fitp = C.POINTER(ModelFitOptsC)
    L.ctag_model_fit_opts_default.restype = None
    L.ctag_model_fit_opts_default.argtypes = [fitp]
    L.ctag_model_fit_device.restype = C.c_int
    L.ctag_model_fit_device.argtypes = [vp, vp, C.c_int, vp, C.POINTER(CameraC), fitp, C.POINTER(vp), vp]
    L.ctag_model_fit.restype = C.c_int
    L.ctag_model_fit.argtypes = [vp, vp, C.c_int, vp, C.POINTER(CameraC), fitp, C.POINTER(vp), vp]
    L.ctag_model_save.restype = C.c_int
    L.ctag_model_save.argtypes = [vp, C.c_char_p]
    L.ctag_model_fit_last_ms.restype = C.c_int
    L.ctag_model_fit_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    rfitp = C.POINTER(RigFitOptsC)
    L.ctag_rig_fit_opts_default.restype = None
    L.ctag_rig_fit_opts_default.argtypes = [rfitp]
    L.ctag_rig_fit_device.restype = C.c_int
    L.ctag_rig_fit_device.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(CameraC), rfitp, C.POINTER(vp), vp, vp]
    L.ctag_rig_fit.restype = C.c_int
    L.ctag_rig_fit.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(CameraC), rfitp, C.POINTER(vp), vp, vp]
    L.ctag_rig_fit_last_ms.restype = C.c_int
    L.ctag_rig_fit_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    cfitp = C.POINTER(CameraFitOptsC)
    L.ctag_camera_fit_opts_default.restype = None
    L.ctag_camera_fit_opts_default.argtypes = [cfitp]
    L.ctag_camera_fit_device.restype = C.c_int
    L.ctag_camera_fit_device.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, vp, vp, C.POINTER(CameraC), cfitp, C.POINTER(vp), vp, vp]
    L.ctag_camera_fit.restype = C.c_int
    L.ctag_camera_fit.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(CameraC), cfitp, C.POINTER(vp), vp, vp]
    L.ctag_camera_fit_last_ms.restype = C.c_int
    L.ctag_camera_fit_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    ifitp = C.POINTER(IntrinsicsFitOptsC)
    L.ctag_intrinsics_fit_opts_default.restype = None
    L.ctag_intrinsics_fit_opts_default.argtypes = [ifitp]
    for fn in (L.ctag_intrinsics_fit_device, L.ctag_intrinsics_fit):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(CameraC), ifitp, C.POINTER(CameraC), vp, vp]
    L.ctag_intrinsics_fit_last_ms.restype = C.c_int
    L.ctag_intrinsics_fit_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ctag_camera_set_get.restype = C.c_int
    L.ctag_camera_set_get.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(CameraC), C.POINTER(CameraPoseC)]
    u64p = C.POINTER(C.c_uint64)
    L.ctag_shard_range.restype = C.c_int
    L.ctag_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ctag_packed_capacity.restype = C.c_size_t
    L.ctag_packed_capacity.argtypes = [C.c_int]
    L.ctag_pack_results.restype = C.c_int
    L.ctag_pack_results.argtypes = [vp, vp, C.c_int, vp, C.c_size_t, u64p]
    L.ctag_unpack_results.restype = C.c_int
    L.ctag_unpack_results.argtypes = [vp, vp, C.c_int, vp]
    L.ctag_comm_unique_id.restype = C.c_int
    L.ctag_comm_unique_id.argtypes = [vp]
    L.ctag_comm_init.restype = C.c_int
    L.ctag_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    L.ctag_comm_attach.restype = C.c_int
    L.ctag_comm_attach.argtypes = [vp, vp, C.c_int, C.c_int]
    L.ctag_comm_destroy.restype = C.c_int
    L.ctag_comm_destroy.argtypes = [vp]
    L.ctag_comm_native.restype = vp
    L.ctag_comm_native.argtypes = [vp]
    L.ctag_comm_last_error.restype = C.c_char_p
    L.ctag_comm_last_error.argtypes = [vp]
    L.ctag_gather_begin.restype = C.c_int
    L.ctag_gather_begin.argtypes = [vp, vp, C.c_int, C.c_int]
    L.ctag_gather_end.restype = C.c_int
    L.ctag_gather_end.argtypes = [vp, vp]
    L.ctag_gather_wait.restype = C.c_int
    L.ctag_gather_wait.argtypes = [vp]
    L.ctag_gather.restype = C.c_int
    L.ctag_gather.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.ctag_gather_last_bytes.restype = C.c_int
    L.ctag_gather_last_bytes.argtypes = [vp, u64p, u64p]
    L.ctag_gather_set_timeout.restype = C.c_int
    L.ctag_gather_set_timeout.argtypes = [vp, C.c_int]
    _lib = L
    return L


def _strerror(status):
    try:
        return load_library().ctag_strerror(status).decode()
    except Exception:  # pragma: no cover
        return "ctag error"


def comm_unique_id():
    """ncclGetUniqueId through the C ABI: 128 bytes rank 0 hands to the other ranks."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    st = load_library().ctag_comm_unique_id(buf)
    if st != 0:
        raise CtagError(st, "ctag_comm_unique_id (RCCL not loadable?)")
    return bytes(buf)


def shard_range(n_total, rank, world):
    lo, hi = C.c_int(), C.c_int()
    st = load_library().ctag_shard_range(n_total, rank, world, C.byref(lo), C.byref(hi))
    if st != 0:
        raise CtagError(st, "ctag_shard_range")
    return lo.value, hi.value


def packed_capacity(n):
    return int(load_library().ctag_packed_capacity(n))


def load_marker_file(path):
    """CylinderTag::load_from_file through the C ABI -> (state[int32 rows x cols], feature_size)."""
    L = load_library()
    p = C.POINTER(C.c_int32)()
    r, c, fs = C.c_int(), C.c_int(), C.c_int()
    st = L.ctag_load_marker_file(os.fsencode(path), C.byref(p), C.byref(r), C.byref(c), C.byref(fs))
    if st != 0:
        raise CtagError(st, path)
    try:
        state = np.ctypeslib.as_array(p, shape=(r.value, c.value)).copy()
    finally:
        L.ctag_free(p)
    return state, fs.value


class Model:
    """ctag_model: the reference's vector<ModelInfo> (CylinderTag::loadModel, CylinderTag.cpp:161-190)."""

    def __init__(self, path=None, ids=None, corners=None, model_size=None, base=None, axis=None):
        self.L = load_library()
        m = C.c_void_p()
        if path is not None:
            st = self.L.ctag_model_load(os.fsencode(path), C.byref(m))
        else:
            ids = np.ascontiguousarray(ids, np.int32)
            corners = np.ascontiguousarray(corners, np.float32)
            base = np.ascontiguousarray(base if base is not None else np.zeros((ids.size, 3)), np.float32)
            axis = np.ascontiguousarray(axis if axis is not None else np.zeros((ids.size, 3)), np.float32)
            fp = C.POINTER(C.c_float)
            v = ModelViewC(ids.size, int(model_size), ids.ctypes.data_as(C.POINTER(C.c_int32)), base.ctypes.data_as(fp),
                           axis.ctypes.data_as(fp), corners.ctypes.data_as(fp))
            st = self.L.ctag_model_create(C.byref(v), C.byref(m))
        if st != 0:
            raise CtagError(st, "model %s" % (path or "from arrays"))
        self.m = m

    def view(self):
        v = ModelViewC()
        self.L.ctag_model_get_view(self.m, C.byref(v))
        n, size = v.n_models, v.model_size
        return {"ids": np.ctypeslib.as_array(v.marker_id, (n,)).copy(), "size": size,
                "base": np.ctypeslib.as_array(v.base, (n, 3)).copy(), "axis": np.ctypeslib.as_array(v.axis, (n, 3)).copy(),
                "corners": np.ctypeslib.as_array(v.corners, (n, size * 8, 3)).copy()}

    @classmethod
    def _adopt(cls, handle):
        """A Model around a ctag_model* the library handed out (ctag_model_fit*)."""
        self = cls.__new__(cls)
        self.L = load_library()
        self.m = handle
        return self

    def save(self, path):
        """ctag_model_save: the .model text format of CylinderTag.cpp:168-188; Model(path) reads back the same float bits."""
        st = self.L.ctag_model_save(self.m, os.fsencode(path))
        if st != 0:
            raise CtagError(st, "ctag_model_save %s" % path)

    def close(self):
        if getattr(self, "m", None):
            self.L.ctag_model_free(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Rigs:
    """ctag_rigs: rig_of_model[model's n_models] maps each model index to a rig (-1: none, 0 .. n_rigs-1).  n_rigs defaults
    to one more than the largest entry."""

    def __init__(self, model, rig_of_model, n_rigs=None):
        self.L = load_library()
        self.rig_of_model = np.ascontiguousarray(rig_of_model, np.int32).ravel()
        self.n_rigs = int(n_rigs if n_rigs is not None else (self.rig_of_model.max(initial=-1) + 1))
        r = C.c_void_p()
        st = self.L.ctag_rigs_create(model.m, self.rig_of_model.ctypes.data_as(C.POINTER(C.c_int32)), self.n_rigs, C.byref(r))
        if st != 0:
            raise CtagError(st, "ctag_rigs_create")
        self.r = r

    def close(self):
        if getattr(self, "r", None):
            self.L.ctag_rigs_free(self.r)
            self.r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CameraSet:
    """ctag_camera_set: cameras (CameraC each) and poses [(rvec, tvec)] of the cameras in one reference frame,
    X_cam = R(rvec) X_ref + tvec."""

    def __init__(self, cameras, poses):
        self.L = load_library()
        cameras, poses = list(cameras), list(poses)
        if len(cameras) != len(poses):
            raise ValueError("%d cameras, %d poses" % (len(cameras), len(poses)))
        self.n = len(cameras)
        cams = (CameraC * max(self.n, 1))(*cameras)
        ps = (CameraPoseC * max(self.n, 1))()
        for c, (rv, tv) in enumerate(poses):
            for i in range(3):
                ps[c].rvec[i], ps[c].tvec[i] = float(rv[i]), float(tv[i])
        s = C.c_void_p()
        st = self.L.ctag_camera_set_create(cams, ps, self.n, C.byref(s))
        if st != 0:
            raise CtagError(st, "ctag_camera_set_create")
        self.s = s

    @classmethod
    def _adopt(cls, s):
        """The CameraSet that owns the ctag_camera_set* a C call handed out."""
        self = cls.__new__(cls)
        self.L = load_library()
        self.s = s
        self.n = len(self.poses())
        return self

    def _get(self):
        n = C.c_int()
        cams, ps = (CameraC * MV_MAX_CAMERAS)(), (CameraPoseC * MV_MAX_CAMERAS)()
        st = self.L.ctag_camera_set_get(self.s, C.byref(n), cams, ps)
        if st != 0:
            raise CtagError(st, "ctag_camera_set_get")
        return n.value, cams, ps

    def poses(self):
        """ctag_camera_set_get: [(rvec, tvec)] of the set's cameras, the doubles it was created from."""
        n, _, ps = self._get()
        return [(np.array(ps[c].rvec[:], np.float64), np.array(ps[c].tvec[:], np.float64)) for c in range(n)]

    def cameras(self):
        """ctag_camera_set_get: the CameraC of every camera of the set."""
        n, cams, _ = self._get()
        out = []
        for c in range(n):
            cam = CameraC()
            C.memmove(C.byref(cam), C.byref(cams[c]), C.sizeof(CameraC))
            out.append(cam)
        return out

    def close(self):
        if getattr(self, "s", None):
            self.L.ctag_camera_set_free(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_camera(path):
    """CylinderTag::loadCamera (CylinderTag.cpp:192-196) through the C ABI -> CameraC."""
    cam = CameraC()
    st = load_library().ctag_camera_load(os.fsencode(path), C.byref(cam))
    if st != 0:
        raise CtagError(st, path)
    return cam


def make_camera(K, dist):
    cam = CameraC()
    for i, v in enumerate(np.asarray(K, np.float32).ravel()):
        cam.K[i] = float(v)
    d = np.asarray(dist, np.float32).ravel()
    for i in range(d.size):
        cam.dist[i] = float(d[i])
    cam.n_dist = int(d.size)
    return cam


class _Pinned:
    """Owner of one ctag_host_alloc() block (page-locked host memory)."""

    def __init__(self, nbytes):
        self.L = load_library()
        self.ptr = self.L.ctag_host_alloc(max(1, nbytes))
        if not self.ptr:
            raise MemoryError("ctag_host_alloc(%d)" % nbytes)
        self.buf = (C.c_ubyte * max(1, nbytes)).from_address(self.ptr)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.L.ctag_host_free(self.ptr)
            self.ptr = None


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in page-locked host memory (ctag_host_alloc); the memory lives as long as the array's base."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    owner = _Pinned(n)
    arr = np.frombuffer(owner.buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    arr_owner = owner  # keep alive through the ctypes buffer's _objects chain
    owner.buf._pinned_owner = arr_owner
    return arr


class TrackFilter:
    """ctag_track_filter (include/ctag_pose.h, track filtering): the causal filter of rigs.n_rigs rig pose tracks on a detector's handle;
    its state lives on the device between calls.  Made by Detector.track_filter; it keeps its detector alive, and the detector's close()
    closes it first."""

    def __init__(self, det, rigs, opts=None):
        self.L, self.det, self.n_rigs = det.L, det, rigs.n_rigs
        f = C.c_void_p()
        st = self.L.ctag_track_filter_create(det.h, rigs.r, C.byref(opts) if opts is not None else None, C.byref(f))
        if st != 0:
            raise CtagError(st, "ctag_track_filter_create")
        self.f = f

    @staticmethod
    def _times(name, times, n_frames):
        if times is None:
            return None
        t = np.ascontiguousarray(np.atleast_1d(times), np.float64).reshape(-1)
        if len(t) != n_frames:
            raise ValueError("%s: %d times for %d frames" % (name, len(t), n_frames))
        return t

    def _step(self, fn, name, rec_dt, poses, cov, n_frames, times):
        n = n_frames * self.n_rigs
        poses = np.ascontiguousarray(poses, rec_dt).reshape(-1)
        cov = np.ascontiguousarray(cov, POSE_COV_DT).reshape(-1)
        if len(poses) != n or len(cov) != n:
            raise ValueError("%s: %d pose and %d covariance records for %d frames x %d rigs" % (name, len(poses), len(cov), n_frames, self.n_rigs))
        t = self._times(name, times, n_frames)
        out = np.zeros(max(n, 1), TRACK_DT)
        st = fn(self.f, poses.ctypes.data, cov.ctypes.data, n_frames, None if t is None else t.ctypes.data, out.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return out[:n].reshape(n_frames, self.n_rigs)

    def step(self, rig_poses, cov, n_frames=1, times=None):
        """n_frames x n_rigs host RIG_POSE_DT records with their POSE_COV_DT records, in order -> TRACK_DT [n_frames, n_rigs].  Waits."""
        return self._step(self.L.ctag_rig_track_filter, "ctag_rig_track_filter", RIG_POSE_DT, rig_poses, cov, n_frames, times)

    def step_mv(self, mv_poses, cov, n_frames=1, times=None):
        """The same from MV_POSE_DT records."""
        return self._step(self.L.ctag_mv_rig_track_filter, "ctag_mv_rig_track_filter", MV_POSE_DT, mv_poses, cov, n_frames, times)

    def _step_device(self, fn, name, poses_ptr, cov_ptr, n_frames, times, out_ptr):
        t = self._times(name, times, n_frames)
        st = fn(self.f, poses_ptr, cov_ptr, n_frames, None if t is None else t.ctypes.data, out_ptr)
        if st != 0:
            raise CtagError(st, name)

    def step_device(self, rig_poses_ptr, cov_ptr, out_ptr, n_frames=1, times=None):
        """Device records in, n_frames * n_rigs device TRACK_DT records at out_ptr; enqueued."""
        self._step_device(self.L.ctag_rig_track_filter_device, "ctag_rig_track_filter_device", rig_poses_ptr, cov_ptr, n_frames, times, out_ptr)

    def step_mv_device(self, mv_poses_ptr, cov_ptr, out_ptr, n_frames=1, times=None):
        self._step_device(self.L.ctag_mv_rig_track_filter_device, "ctag_mv_rig_track_filter_device", mv_poses_ptr, cov_ptr, n_frames, times, out_ptr)

    def predict(self, t):
        """The prediction to time t, TRACK_DT [n_rigs]; the state is untouched.  Waits."""
        out = np.zeros(self.n_rigs, TRACK_DT)
        st = self.L.ctag_track_filter_predict(self.f, float(t), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_track_filter_predict")
        return out

    def predict_device(self, t, out_ptr):
        st = self.L.ctag_track_filter_predict_device(self.f, float(t), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_track_filter_predict_device")

    def reset(self):
        st = self.L.ctag_track_filter_reset(self.f)
        if st != 0:
            raise CtagError(st, "ctag_track_filter_reset")

    def set_cov_scale(self, s):
        """From the next call on every covariance is read as s * cov (ctag_track_filter_set_cov_scale); s positive and finite."""
        st = self.L.ctag_track_filter_set_cov_scale(self.f, float(s))
        if st != 0:
            raise CtagError(st, "ctag_track_filter_set_cov_scale")

    def track_filter_last_ms(self):
        """Device milliseconds of the last step call's kernel (needs OPT_TIMING)."""
        out = C.c_float()
        self.L.ctag_track_filter_last_ms(self.f, C.byref(out))
        return float(out.value)

    def close(self):
        if getattr(self, "f", None):
            self.L.ctag_track_filter_free(self.f)
            self.f = None
            if self in getattr(self.det, "_filters", ()):
                self.det._filters.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Detector:
    """One ctag_handle (one GPU).  Mirrors the reference's usage: construct with the dictionary, call detect()."""

    def __init__(self, state, feature_size, device=0, params=None):
        """params: a ParamsC (default_params() edited) for ctag_create_ex; None = the reference's tunables (ctag_create)."""
        self.L = load_library()
        self.state = np.ascontiguousarray(state, dtype=np.int32)
        self.feature_size = int(feature_size)
        h = C.c_void_p()
        if params is None:
            st = self.L.ctag_create(self.state.ctypes.data_as(C.POINTER(C.c_int32)), self.state.shape[0],
                                    self.state.shape[1], self.feature_size, device, C.byref(h))
        else:
            st = self.L.ctag_create_ex(self.state.ctypes.data_as(C.POINTER(C.c_int32)), self.state.shape[0],
                                       self.state.shape[1], self.feature_size, device, C.byref(params), C.byref(h))
        if st != 0:
            raise CtagError(st, "ctag_create")
        self.h = h

    def close(self):
        for f in list(getattr(self, "_filters", ())):   # a filter's state hangs on the handle: freed first, as CylinderTag's destructor does
            f.close()
        if getattr(self, "h", None):
            self.L.ctag_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt, value):
        st = self.L.ctag_set_option(self.h, opt, int(value))
        if st != 0:
            raise CtagError(st, "ctag_set_option")

    # ---- host-memory entry points
    def detect(self, gray, adaptive_thresh=5, subpix=True, subpix_dist=5):
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        res = np.zeros(1, RESULT_DT)
        st = self.L.ctag_detect_u8(self.h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0],
                                   adaptive_thresh, int(subpix), subpix_dist, res.ctypes.data)
        if st < 0:
            raise CtagError(st, "ctag_detect_u8")
        return res[0]

    def submit(self, gray, adaptive_thresh=5, subpix=True, subpix_dist=5):
        """ctag_submit_u8: start one frame without waiting (at most two in flight); `gray` must stay alive until its collect()."""
        assert gray.dtype == np.uint8 and gray.ndim == 2 and gray.strides[1] == 1
        st = self.L.ctag_submit_u8(self.h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0], adaptive_thresh, int(subpix), subpix_dist)
        if st != 0:
            raise CtagError(st, "ctag_submit_u8")

    def collect(self, out=None):
        """ctag_collect: the record of the oldest submitted frame."""
        res = np.zeros(1, RESULT_DT) if out is None else out
        st = self.L.ctag_collect(self.h, res.ctypes.data)
        if st < 0:
            raise CtagError(st, "ctag_collect")
        return res[0]

    def detect_batch(self, frames, adaptive_thresh=5, subpix=True, subpix_dist=5, out=None):
        """frames: (n, rows, cols) uint8 in host memory; pass arrays from pinned_empty() to overlap upload and detection."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, rows, cols = frames.shape
        res = np.zeros(n, RESULT_DT) if out is None else out
        assert res.dtype == RESULT_DT and res.shape == (n,) and res.flags.c_contiguous
        st = self.L.ctag_detect_batch_u8(self.h, frames.ctypes.data, n, rows, cols, frames.strides[1], frames.strides[0],
                                         adaptive_thresh, int(subpix), subpix_dist, res.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_detect_batch_u8")
        return res

    # ---- BGR frames (rows, cols, 3) uint8: cvtColor(BGR2GRAY) of main.cpp:36,52-54 happens on the device
    def detect_bgr(self, bgr, adaptive_thresh=5, subpix=True, subpix_dist=5):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        assert bgr.ndim == 3 and bgr.shape[2] == 3
        res = np.zeros(1, RESULT_DT)
        st = self.L.ctag_detect_bgr8(self.h, bgr.ctypes.data, bgr.shape[0], bgr.shape[1], bgr.strides[0], adaptive_thresh, int(subpix), subpix_dist,
                                     res.ctypes.data)
        if st < 0:
            raise CtagError(st, "ctag_detect_bgr8")
        return res[0]

    def detect_batch_bgr(self, frames, adaptive_thresh=5, subpix=True, subpix_dist=5, out=None):
        """frames: (n, rows, cols, 3) uint8 in host memory (pinned_empty() arrays overlap upload and detection)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, rows, cols, ch = frames.shape
        assert ch == 3
        res = np.zeros(n, RESULT_DT) if out is None else out
        assert res.dtype == RESULT_DT and res.shape == (n,) and res.flags.c_contiguous
        st = self.L.ctag_detect_batch_bgr8(self.h, frames.ctypes.data, n, rows, cols, frames.strides[1], frames.strides[0], adaptive_thresh, int(subpix),
                                           subpix_dist, res.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_detect_batch_bgr8")
        return res

    def detect_batch_bgr_device(self, frames_ptr, n, rows, cols, row_stride, frame_stride, out_ptr, adaptive_thresh=5, subpix=True, subpix_dist=5):
        st = self.L.ctag_detect_batch_bgr8_device(self.h, frames_ptr, n, rows, cols, row_stride, frame_stride, adaptive_thresh, int(subpix), subpix_dist,
                                                  out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_detect_batch_bgr8_device")

    # ---- device-memory entry point (pointers are plain integers, e.g. torch.Tensor.data_ptr())
    def detect_batch_device(self, frames_ptr, n, rows, cols, row_stride, frame_stride, out_ptr, adaptive_thresh=5,
                            subpix=True, subpix_dist=5):
        st = self.L.ctag_detect_batch_device(self.h, frames_ptr, n, rows, cols, row_stride, frame_stride,
                                             adaptive_thresh, int(subpix), subpix_dist, out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_detect_batch_device")

    def sync(self):
        st = self.L.ctag_sync(self.h)
        if st != 0:
            raise CtagError(st, "ctag_sync")

    def stream(self):
        return self.L.ctag_stream(self.h)

    def counters(self):
        """Per-frame counts of the last chunk: {name: (mean, max)} for components / candidates / quads / features / markers, plus
        'frames' and 'reruns' (frames completed through the any-frame workspace since the handle was created)."""
        c = CountersC()
        st = self.L.ctag_get_counters(self.h, C.byref(c))
        if st != 0:
            raise CtagError(st, "ctag_get_counters")
        out = {"frames": int(c.frames), "reruns": int(c.reruns)}
        for k, name in enumerate(COUNTER_NAMES):
            out[name] = (c.sum[k] / c.frames if c.frames else 0.0, int(c.max[k]))
        return out

    def timings(self):
        buf = (C.c_float * len(STAGE_NAMES))()
        n = self.L.ctag_get_timings(self.h, buf, len(STAGE_NAMES))
        return {STAGE_NAMES[i]: float(buf[i]) for i in range(n)}

    # ---- multi-GPU gather (include/ctag_gather.h); pointers are plain integers
    def _gcheck(self, st, what):
        if st != 0:
            raise CtagError(st, "%s: %s" % (what, self.L.ctag_comm_last_error(self.h).decode()))

    def pack_results(self, results_ptr, n, packed_ptr, capacity):
        nbytes = C.c_uint64()
        self._gcheck(self.L.ctag_pack_results(self.h, results_ptr, n, packed_ptr, capacity, C.byref(nbytes)), "ctag_pack_results")
        return int(nbytes.value)

    def unpack_results(self, packed_ptr, n, out_ptr):
        self._gcheck(self.L.ctag_unpack_results(self.h, packed_ptr, n, out_ptr), "ctag_unpack_results")

    def comm_init(self, id_bytes, rank, world):
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        self._gcheck(self.L.ctag_comm_init(self.h, buf, rank, world), "ctag_comm_init")

    def comm_destroy(self):
        self.L.ctag_comm_destroy(self.h)

    def comm_native(self):
        return self.L.ctag_comm_native(self.h)

    def comm_attach(self, nccl_comm, rank, world):
        self._gcheck(self.L.ctag_comm_attach(self.h, nccl_comm, rank, world), "ctag_comm_attach")

    def gather_begin(self, local_ptr, n_local, n_total):
        self._gcheck(self.L.ctag_gather_begin(self.h, local_ptr, n_local, n_total), "ctag_gather_begin")

    def gather_end(self, out_ptr):
        self._gcheck(self.L.ctag_gather_end(self.h, out_ptr), "ctag_gather_end")

    def gather_wait(self):
        self._gcheck(self.L.ctag_gather_wait(self.h), "ctag_gather_wait")

    def gather(self, local_ptr, n_local, n_total, out_ptr):
        self._gcheck(self.L.ctag_gather(self.h, local_ptr, n_local, n_total, out_ptr), "ctag_gather")

    def gather_set_timeout(self, timeout_ms):
        """Deadline of the gather's host waits (ms; 0 none; < 0 the default: CTAG_GATHER_TIMEOUT_MS, else 60 s)."""
        self._gcheck(self.L.ctag_gather_set_timeout(self.h, int(timeout_ms)), "ctag_gather_set_timeout")

    def gather_last_bytes(self):
        a, b = C.c_uint64(), C.c_uint64()
        self.L.ctag_gather_last_bytes(self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- pose back end (include/ctag_pose.h)
    def estimate_pose(self, result, model, camera):
        """One frame: host ctag_frame_result record -> POSE_DT records, one per marker (CylinderTag::estimatePose
        before its erase of the model-less entries)."""
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        n = int(res[0]["n_markers"]) if res[0]["status"] == 0 else 0
        out = np.zeros(max(n, 1), POSE_DT)
        st = self.L.ctag_estimate_pose(self.h, res.ctypes.data, model.m, C.byref(camera), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_pose")
        return out[:n]

    def pose_batch_device(self, results_ptr, n_frames, model, camera, offsets_ptr, poses_ptr, capacity):
        st = self.L.ctag_pose_batch_device(self.h, results_ptr, n_frames, model.m, C.byref(camera), offsets_ptr, poses_ptr,
                                           capacity)
        if st != 0:
            raise CtagError(st, "ctag_pose_batch_device")

    def estimate_rig_pose(self, result, model, rigs, camera):
        """One frame: host ctag_frame_result record -> rigs.n_rigs RIG_POSE_DT records (record g = rig g)."""
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        out = np.zeros(rigs.n_rigs, RIG_POSE_DT)
        st = self.L.ctag_estimate_rig_pose(self.h, res.ctypes.data, model.m, rigs.r, C.byref(camera), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_rig_pose")
        return out

    def rig_pose_batch_device(self, results_ptr, n_frames, model, rigs, camera, out_ptr):
        """n_frames device result records -> n_frames * rigs.n_rigs device RIG_POSE_DT records at out_ptr (record f*n_rigs + g);
        enqueued on the handle's stream."""
        st = self.L.ctag_rig_pose_batch_device(self.h, results_ptr, n_frames, model.m, rigs.r, C.byref(camera), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_rig_pose_batch_device")

    def estimate_mv_rig_pose(self, results, model, rigs, cams):
        """One instant: cams.n host ctag_frame_result records (record c from camera c) -> rigs.n_rigs MV_POSE_DT records."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == RESULT_DT
        if len(res) != cams.n:
            raise ValueError("%d records for %d cameras" % (len(res), cams.n))
        out = np.zeros(rigs.n_rigs, MV_POSE_DT)
        st = self.L.ctag_estimate_mv_rig_pose(self.h, res.ctypes.data, model.m, rigs.r, cams.s, out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_mv_rig_pose")
        return out

    def mv_rig_pose_batch_device(self, results_ptrs, n_frames, model, rigs, cams, out_ptr):
        """results_ptrs: one device pointer per camera of cams, n_frames result records each -> n_frames * rigs.n_rigs device
        MV_POSE_DT records at out_ptr (record f*n_rigs + g); enqueued on the handle's stream."""
        ptrs = list(results_ptrs)
        if len(ptrs) != cams.n:
            raise ValueError("%d pointers for %d cameras" % (len(ptrs), cams.n))
        arr = (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(int(p) if p else None) for p in ptrs])
        st = self.L.ctag_mv_rig_pose_batch_device(self.h, arr, n_frames, model.m, rigs.r, cams.s, out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_mv_rig_pose_batch_device")

    def pose_last_ms(self):
        return float(self.L.ctag_pose_last_ms(self.h))

    # ---- model reconstruction (include/ctag_pose.h): opts is a ModelFitOptsC (model_fit_opts(...)) or None for the defaults
    def _fit(self, fn, name, results_arg, n_frames, seed, camera, opts):
        n_models = int(seed.view()["ids"].size)
        stats = np.zeros(max(n_models, 1), MODEL_FIT_STAT_DT)
        m = C.c_void_p()
        st = fn(self.h, results_arg, n_frames, seed.m, C.byref(camera), C.byref(opts) if opts is not None else None, C.byref(m), stats.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return Model._adopt(m), stats[:n_models]

    def fit_model(self, results, seed, camera, opts=None):
        """ctag_model_fit: host ctag_frame_result records of many frames and a seed Model -> (the Model that minimises the reprojection
        error over them, MODEL_FIT_STAT_DT records, one per model).  Waits."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == RESULT_DT
        return self._fit(self.L.ctag_model_fit, "ctag_model_fit", res.ctypes.data if len(res) else None, len(res), seed, camera, opts)

    def fit_model_device(self, results_ptr, n_frames, seed, camera, opts=None):
        """ctag_model_fit_device: the same from n_frames result records in device memory (as detect_batch_device leaves them)."""
        return self._fit(self.L.ctag_model_fit_device, "ctag_model_fit_device", results_ptr, n_frames, seed, camera, opts)

    def model_fit_last_ms(self):
        """Device milliseconds of the last fit call by kernel kind (needs OPT_TIMING): pose, record, assemble, solve."""
        out = (C.c_float * 4)()
        self.L.ctag_model_fit_last_ms(self.h, out)
        return dict(zip(("pose", "record", "assemble", "solve"), (float(v) for v in out)))

    # ---- rig assembly (include/ctag_pose.h): opts is a RigFitOptsC (rig_fit_opts(...)) or None for the defaults
    def _fit_rigs(self, fn, name, results_arg, n_frames, model, rigs, camera, opts):
        n_models = int(model.view()["ids"].size)
        rig_stats = np.zeros(max(rigs.n_rigs, 1), RIG_FIT_STAT_DT)
        model_stats = np.zeros(max(n_models, 1), RIG_FIT_MODEL_STAT_DT)
        m = C.c_void_p()
        st = fn(self.h, results_arg, n_frames, model.m, rigs.r, C.byref(camera), C.byref(opts) if opts is not None else None, C.byref(m),
                rig_stats.ctypes.data, model_stats.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        model_stats = model_stats[:n_models]
        placed = np.where(model_stats["status"] == POSE_OK, rigs.rig_of_model[:n_models], -1).astype(np.int32)
        return Model._adopt(m), rig_stats[:rigs.n_rigs], model_stats, placed

    def fit_rigs(self, results, model, rigs, camera, opts=None):
        """ctag_rig_fit: host ctag_frame_result records of many frames, a Model whose models each have their own frame and the Rigs that
        groups them -> (the Model with every rig's models in the frame of the rig's anchor, RIG_FIT_STAT_DT records, one per rig,
        RIG_FIT_MODEL_STAT_DT records, one per model, rig_of_model with the unplaced models at -1: what Rigs takes for the result).  Waits."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == RESULT_DT
        return self._fit_rigs(self.L.ctag_rig_fit, "ctag_rig_fit", res.ctypes.data if len(res) else None, len(res), model, rigs, camera, opts)

    def fit_rigs_device(self, results_ptr, n_frames, model, rigs, camera, opts=None):
        """ctag_rig_fit_device: the same from n_frames result records in device memory (as detect_batch_device leaves them)."""
        return self._fit_rigs(self.L.ctag_rig_fit_device, "ctag_rig_fit_device", results_ptr, n_frames, model, rigs, camera, opts)

    def rig_fit_last_ms(self):
        """Device milliseconds of the last assembly by kernel kind (needs OPT_TIMING): marker pose, rig pose, record + assemble, solve."""
        out = (C.c_float * 4)()
        self.L.ctag_rig_fit_last_ms(self.h, out)
        return dict(zip(("marker_pose", "rig_pose", "record", "solve"), (float(v) for v in out)))

    # ---- camera set fit (include/ctag_pose.h): opts is a CameraFitOptsC (camera_fit_opts(...)), or its fields as keywords
    def _fit_camera_set(self, fn, name, results_arg, n_cameras, n_frames, model, rigs, cameras, opts, fields):
        if fields:
            if opts is not None:
                raise TypeError("opts and option keywords together")
            opts = camera_fit_opts(**fields)
        cameras = list(cameras)
        if len(cameras) != n_cameras:
            raise ValueError("%d cameras for %d record arrays" % (len(cameras), n_cameras))
        cams = (CameraC * max(n_cameras, 1))(*cameras)
        stat = np.zeros(1, CAMERA_FIT_STAT_DT)
        cam_stats = np.zeros(max(n_cameras, 1), CAMERA_FIT_CAM_STAT_DT)
        s = C.c_void_p()
        st = fn(self.h, results_arg, n_cameras, n_frames, model.m, rigs.r, cams, C.byref(opts) if opts is not None else None, C.byref(s),
                stat.ctypes.data, cam_stats.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return (CameraSet._adopt(s) if s.value else None), stat[0], cam_stats[:n_cameras]

    def fit_camera_set(self, records_per_camera, model, rigs, cameras, opts=None, **fields):
        """ctag_camera_fit: records_per_camera[c][f] = the host ctag_frame_result record of camera c at instant f, and the cameras'
        intrinsics (CameraC each) -> (the CameraSet with every camera's pose in the anchor camera's frame, or None when a camera could
        not be placed; one CAMERA_FIT_STAT_DT record; CAMERA_FIT_CAM_STAT_DT records, one per camera).  Waits."""
        res = np.ascontiguousarray(records_per_camera)
        assert res.dtype == RESULT_DT and res.ndim == 2
        return self._fit_camera_set(self.L.ctag_camera_fit, "ctag_camera_fit", res.ctypes.data if res.size else None, res.shape[0], res.shape[1], model, rigs,
                                    cameras, opts, fields)

    def fit_camera_set_device(self, results_ptrs, n_frames, model, rigs, cameras, opts=None, **fields):
        """ctag_camera_fit_device: the same from one device pointer per camera, n_frames result records each."""
        ptrs = (C.c_void_p * max(len(results_ptrs), 1))(*[int(p) for p in results_ptrs])
        return self._fit_camera_set(self.L.ctag_camera_fit_device, "ctag_camera_fit_device", ptrs, len(results_ptrs), n_frames, model, rigs, cameras, opts, fields)

    def camera_fit_last_ms(self):
        """Device milliseconds of the last camera set fit by kernel kind (needs OPT_TIMING): per-camera rig pose, multi-view pose, record + assemble, solve."""
        out = (C.c_float * 4)()
        self.L.ctag_camera_fit_last_ms(self.h, out)
        return dict(zip(("rig_pose", "mv_pose", "record", "solve"), (float(v) for v in out)))

    # ---- intrinsics fit (include/ctag_pose.h): opts is an IntrinsicsFitOptsC (intrinsics_fit_opts(...)), or its fields as keywords
    def _fit_intrinsics(self, fn, name, results_arg, n_frames, model, rigs, seed, opts, fields):
        if fields:
            if opts is not None:
                raise TypeError("opts and option keywords together")
            opts = intrinsics_fit_opts(**fields)
        if rigs is None:  # every model a rig of its own
            n_models = int(model.view()["ids"].size)
            rigs = Rigs(model, np.arange(n_models, dtype=np.int32), n_models)
        out = CameraC()
        stat = np.zeros(1, INTRINSICS_FIT_STAT_DT)
        poses = np.zeros(max(n_frames * rigs.n_rigs, 1), RIG_POSE_DT)
        st = fn(self.h, results_arg, n_frames, model.m, rigs.r, C.byref(seed), C.byref(opts) if opts is not None else None, C.byref(out), stat.ctypes.data,
                poses.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return out, stat[0], poses[:n_frames * rigs.n_rigs]

    def fit_intrinsics(self, results, model, rigs, seed, opts=None, **fields):
        """ctag_intrinsics_fit: host ctag_frame_result records of many views of rigs whose models are known, and a rough seed CameraC ->
        (the fitted CameraC, one INTRINSICS_FIT_STAT_DT record with the parameters' sigmas, the RIG_POSE_DT records of every view under
        it, record f * n_rigs + g).  rigs=None makes every model a rig of its own.  Waits."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == RESULT_DT
        return self._fit_intrinsics(self.L.ctag_intrinsics_fit, "ctag_intrinsics_fit", res.ctypes.data if len(res) else None, len(res), model, rigs, seed, opts, fields)

    def fit_intrinsics_device(self, results_ptr, n_frames, model, rigs, seed, opts=None, **fields):
        """ctag_intrinsics_fit_device: the same from n_frames result records in device memory (as detect_batch_device leaves them)."""
        return self._fit_intrinsics(self.L.ctag_intrinsics_fit_device, "ctag_intrinsics_fit_device", results_ptr, n_frames, model, rigs, seed, opts, fields)

    def intrinsics_fit_last_ms(self):
        """Device milliseconds of the last intrinsics fit by kernel kind (needs OPT_TIMING): rig pose, view pose, record + assemble, solve."""
        out = (C.c_float * 4)()
        self.L.ctag_intrinsics_fit_last_ms(self.h, out)
        return dict(zip(("rig_pose", "view_pose", "record", "solve"), (float(v) for v in out)))

    # ---- track smoothing (include/ctag_pose.h): opts is a TrackOptsC (track_opts(...)) or None for the defaults
    def _smooth(self, fn, name, rec_dt, rigs, poses, cov, n_frames, times, opts):
        n = n_frames * rigs.n_rigs
        poses = np.ascontiguousarray(poses, rec_dt).reshape(-1)
        cov = np.ascontiguousarray(cov, POSE_COV_DT).reshape(-1)
        if len(poses) != n or len(cov) != n:
            raise ValueError("%s: %d pose and %d covariance records for %d frames x %d rigs" % (name, len(poses), len(cov), n_frames, rigs.n_rigs))
        t = None if times is None else np.ascontiguousarray(times, np.float64).reshape(-1)
        if t is not None and len(t) != n_frames:
            raise ValueError("%s: %d times for %d frames" % (name, len(t), n_frames))
        out, stat = np.zeros(max(n, 1), TRACK_DT), np.zeros(rigs.n_rigs, TRACK_STAT_DT)
        st = fn(self.h, rigs.r, poses.ctypes.data, cov.ctypes.data, n_frames, None if t is None else t.ctypes.data, self._optp(opts),
                out.ctypes.data, stat.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return out[:n].reshape(n_frames, rigs.n_rigs), stat

    def smooth_rig_track(self, rigs, rig_poses, cov, n_frames, times=None, opts=None):
        """n_frames x rigs.n_rigs host RIG_POSE_DT records with their POSE_COV_DT records -> (TRACK_DT [n_frames, n_rigs], TRACK_STAT_DT [n_rigs]).
        Waits."""
        return self._smooth(self.L.ctag_rig_track_smooth, "ctag_rig_track_smooth", RIG_POSE_DT, rigs, rig_poses, cov, n_frames, times, opts)

    def smooth_mv_rig_track(self, rigs, mv_poses, cov, n_frames, times=None, opts=None):
        """The same from MV_POSE_DT records (poses in the reference frame)."""
        return self._smooth(self.L.ctag_mv_rig_track_smooth, "ctag_mv_rig_track_smooth", MV_POSE_DT, rigs, mv_poses, cov, n_frames, times, opts)

    def _smooth_device(self, fn, name, rigs, poses_ptr, cov_ptr, n_frames, times, opts, out_ptr, stat_ptr):
        t = None if times is None else np.ascontiguousarray(times, np.float64).reshape(-1)
        if t is not None and len(t) != n_frames:
            raise ValueError("%s: %d times for %d frames" % (name, len(t), n_frames))
        st = fn(self.h, rigs.r, poses_ptr, cov_ptr, n_frames, None if t is None else t.ctypes.data, self._optp(opts), out_ptr, stat_ptr)
        if st != 0:
            raise CtagError(st, name)

    def smooth_rig_track_device(self, rigs, rig_poses_ptr, cov_ptr, n_frames, out_ptr, stat_ptr, times=None, opts=None):
        """Device RIG_POSE_DT / POSE_COV_DT records -> n_frames * n_rigs device TRACK_DT records at out_ptr, n_rigs TRACK_STAT_DT at stat_ptr; enqueued."""
        self._smooth_device(self.L.ctag_rig_track_smooth_device, "ctag_rig_track_smooth_device", rigs, rig_poses_ptr, cov_ptr, n_frames, times, opts, out_ptr, stat_ptr)

    def smooth_mv_rig_track_device(self, rigs, mv_poses_ptr, cov_ptr, n_frames, out_ptr, stat_ptr, times=None, opts=None):
        """The same from device MV_POSE_DT records."""
        self._smooth_device(self.L.ctag_mv_rig_track_smooth_device, "ctag_mv_rig_track_smooth_device", rigs, mv_poses_ptr, cov_ptr, n_frames, times, opts, out_ptr, stat_ptr)

    def track_last_ms(self):
        """Device milliseconds of the last smoothing call (needs OPT_TIMING): gather + pieces + start, the rounds, marginals + records, the whole call."""
        out = (C.c_float * 4)()
        self.L.ctag_track_last_ms(self.h, out)
        return dict(zip(("setup", "rounds", "marginals", "total"), (float(v) for v in out)))

    def track_filter(self, rigs, opts=None):
        """A TrackFilter for rigs.n_rigs rigs on this detector (include/ctag_pose.h, track filtering); opts is a TrackFilterOptsC
        (track_filter_opts(...)) or None for the defaults.  The detector closes the filters it made that are still open when it is closed."""
        f = TrackFilter(self, rigs, opts)
        if not hasattr(self, "_filters"):
            self._filters = []
        self._filters.append(f)
        return f

    # ---- track noise fit (include/ctag_pose.h): opts is a TrackNoiseOptsC (track_noise_opts(...)) or None for the defaults
    @staticmethod
    def _noise_inputs(name, rec_dt, rigs, poses, cov, n_frames, times):
        n = n_frames * rigs.n_rigs
        poses = np.ascontiguousarray(poses, rec_dt).reshape(-1)
        cov = np.ascontiguousarray(cov, POSE_COV_DT).reshape(-1)
        if len(poses) != n or len(cov) != n:
            raise ValueError("%s: %d pose and %d covariance records for %d frames x %d rigs" % (name, len(poses), len(cov), n_frames, rigs.n_rigs))
        return poses, cov, Detector._noise_times(name, times, n_frames)

    @staticmethod
    def _noise_times(name, times, n_frames):
        t = None if times is None else np.ascontiguousarray(times, np.float64).reshape(-1)
        if t is not None and len(t) != n_frames:
            raise ValueError("%s: %d times for %d frames" % (name, len(t), n_frames))
        return t

    @staticmethod
    def _noise_searches(rigs, opts):
        o = opts if opts is not None else track_noise_opts()
        return (1 if o.mode == NOISE_POOLED else rigs.n_rigs), max(int(o.rounds), 1)

    def _fit_noise(self, fn, name, rec_dt, rigs, poses, cov, n_frames, times, opts, trace):
        poses, cov, t = self._noise_inputs(name, rec_dt, rigs, poses, cov, n_frames, times)
        ns, rounds = self._noise_searches(rigs, opts)
        out = np.zeros(ns, TRACK_NOISE_DT)
        tr = np.zeros(ns * min(rounds, 16), TRACK_NOISE_ROUND_DT) if trace else None
        st = fn(self.h, rigs.r, poses.ctypes.data, cov.ctypes.data, n_frames, None if t is None else t.ctypes.data, self._optp(opts),
                out.ctypes.data, None if tr is None else tr.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return (out, tr.reshape(ns, -1)) if trace else out

    def fit_track_noise(self, rigs, rig_poses, cov, n_frames, times=None, opts=None, trace=False):
        """The filter's q_rot, q_trans and covariance scale from n_frames x rigs.n_rigs host RIG_POSE_DT records with their POSE_COV_DT
        records -> TRACK_NOISE_DT [n_rigs] (per rig) or [1] (pooled); with trace=True also TRACK_NOISE_ROUND_DT [searches, rounds].  Waits."""
        return self._fit_noise(self.L.ctag_rig_track_noise_fit, "ctag_rig_track_noise_fit", RIG_POSE_DT, rigs, rig_poses, cov, n_frames, times, opts, trace)

    def fit_mv_track_noise(self, rigs, mv_poses, cov, n_frames, times=None, opts=None, trace=False):
        """The same from MV_POSE_DT records."""
        return self._fit_noise(self.L.ctag_mv_rig_track_noise_fit, "ctag_mv_rig_track_noise_fit", MV_POSE_DT, rigs, mv_poses, cov, n_frames, times, opts, trace)

    def _fit_noise_device(self, fn, name, rigs, poses_ptr, cov_ptr, n_frames, times, opts, out_ptr, trace_ptr):
        t = self._noise_times(name, times, n_frames)
        st = fn(self.h, rigs.r, poses_ptr, cov_ptr, n_frames, None if t is None else t.ctypes.data, self._optp(opts), out_ptr, trace_ptr)
        if st != 0:
            raise CtagError(st, name)

    def fit_track_noise_device(self, rigs, rig_poses_ptr, cov_ptr, n_frames, out_ptr, trace_ptr=None, times=None, opts=None):
        """Device RIG_POSE_DT / POSE_COV_DT records -> device TRACK_NOISE_DT records at out_ptr and, when trace_ptr is given, the trace; enqueued."""
        self._fit_noise_device(self.L.ctag_rig_track_noise_fit_device, "ctag_rig_track_noise_fit_device", rigs, rig_poses_ptr, cov_ptr, n_frames, times, opts,
                               out_ptr, trace_ptr)

    def fit_mv_track_noise_device(self, rigs, mv_poses_ptr, cov_ptr, n_frames, out_ptr, trace_ptr=None, times=None, opts=None):
        """The same from device MV_POSE_DT records."""
        self._fit_noise_device(self.L.ctag_mv_rig_track_noise_fit_device, "ctag_mv_rig_track_noise_fit_device", rigs, mv_poses_ptr, cov_ptr, n_frames, times,
                               opts, out_ptr, trace_ptr)

    @staticmethod
    def _noise_cands(name, cands):
        c = np.ascontiguousarray(cands, np.float64).reshape(-1, 3)
        return c

    def _score_noise(self, fn, name, rec_dt, rigs, poses, cov, n_frames, cands, times, opts):
        poses, cov, t = self._noise_inputs(name, rec_dt, rigs, poses, cov, n_frames, times)
        c = self._noise_cands(name, cands)
        out = np.zeros(max(len(c), 1) * rigs.n_rigs, TRACK_NOISE_SCORE_DT)
        st = fn(self.h, rigs.r, poses.ctypes.data, cov.ctypes.data, n_frames, None if t is None else t.ctypes.data, self._optp(opts),
                c.ctypes.data, len(c), out.ctypes.data)
        if st != 0:
            raise CtagError(st, name)
        return out[:len(c) * rigs.n_rigs].reshape(len(c), rigs.n_rigs)

    def score_track_noise(self, rigs, rig_poses, cov, n_frames, cands, times=None, opts=None):
        """The score alone at cands [n_cand, 3] = (q_rot, q_trans, cov_scale) -> TRACK_NOISE_SCORE_DT [n_cand, n_rigs].  Waits."""
        return self._score_noise(self.L.ctag_rig_track_noise_score, "ctag_rig_track_noise_score", RIG_POSE_DT, rigs, rig_poses, cov, n_frames, cands, times, opts)

    def score_mv_track_noise(self, rigs, mv_poses, cov, n_frames, cands, times=None, opts=None):
        """The same from MV_POSE_DT records."""
        return self._score_noise(self.L.ctag_mv_rig_track_noise_score, "ctag_mv_rig_track_noise_score", MV_POSE_DT, rigs, mv_poses, cov, n_frames, cands, times, opts)

    def _score_noise_device(self, fn, name, rigs, poses_ptr, cov_ptr, n_frames, cands, times, opts, out_ptr):
        t = self._noise_times(name, times, n_frames)
        c = self._noise_cands(name, cands)
        st = fn(self.h, rigs.r, poses_ptr, cov_ptr, n_frames, None if t is None else t.ctypes.data, self._optp(opts), c.ctypes.data, len(c), out_ptr)
        if st != 0:
            raise CtagError(st, name)

    def score_track_noise_device(self, rigs, rig_poses_ptr, cov_ptr, n_frames, cands, out_ptr, times=None, opts=None):
        """Device records in, n_cand * n_rigs device TRACK_NOISE_SCORE_DT entries at out_ptr; enqueued."""
        self._score_noise_device(self.L.ctag_rig_track_noise_score_device, "ctag_rig_track_noise_score_device", rigs, rig_poses_ptr, cov_ptr, n_frames, cands,
                                 times, opts, out_ptr)

    def score_mv_track_noise_device(self, rigs, mv_poses_ptr, cov_ptr, n_frames, cands, out_ptr, times=None, opts=None):
        self._score_noise_device(self.L.ctag_mv_rig_track_noise_score_device, "ctag_mv_rig_track_noise_score_device", rigs, mv_poses_ptr, cov_ptr, n_frames,
                                 cands, times, opts, out_ptr)

    def track_noise_last_ms(self):
        """Device milliseconds of the last noise call's kernels (needs OPT_TIMING)."""
        out = C.c_float()
        self.L.ctag_track_noise_last_ms(self.h, C.byref(out))
        return float(out.value)

    # ---- hand-eye calibration (include/ctag_pose.h): opts is a HandEyeOptsC (hand_eye_opts(...)) or None for the defaults
    @staticmethod
    def _links(name, links, n_frames):
        links = np.ascontiguousarray(links, LINK_POSE_DT).reshape(-1)
        if len(links) != n_frames:
            raise ValueError("%s: %d link poses for %d frames" % (name, len(links), n_frames))
        return links

    def _hand_eye(self, fn, name, rec_dt, rigs, poses, cov, n_frames, links, opts, want_frames):
        n = n_frames * rigs.n_rigs
        poses = np.ascontiguousarray(poses, rec_dt).reshape(-1)
        cov = np.ascontiguousarray(cov, POSE_COV_DT).reshape(-1)
        if len(poses) != n or len(cov) != n:
            raise ValueError("%s: %d pose and %d covariance records for %d frames x %d rigs" % (name, len(poses), len(cov), n_frames, rigs.n_rigs))
        links = self._links(name, links, n_frames)
        out = np.zeros(rigs.n_rigs, HAND_EYE_DT)
        frames = np.zeros(max(n, 1), HAND_EYE_FRAME_DT) if want_frames else None
        st = fn(self.h, rigs.r, poses.ctypes.data, cov.ctypes.data, n_frames, links.ctypes.data, self._optp(opts), out.ctypes.data,
                frames.ctypes.data if want_frames else None)
        if st != 0:
            raise CtagError(st, name)
        return out, (frames[:n].reshape(n_frames, rigs.n_rigs) if want_frames else None)

    def fit_hand_eye(self, rigs, rig_poses, cov, n_frames, links, opts=None, frames=True):
        """n_frames x rigs.n_rigs host RIG_POSE_DT records with their POSE_COV_DT records and n_frames LINK_POSE_DT link poses ->
        (HAND_EYE_DT [n_rigs], HAND_EYE_FRAME_DT [n_frames, n_rigs] or None when frames is false).  Waits."""
        return self._hand_eye(self.L.ctag_rig_hand_eye_fit, "ctag_rig_hand_eye_fit", RIG_POSE_DT, rigs, rig_poses, cov, n_frames, links, opts, frames)

    def fit_mv_hand_eye(self, rigs, mv_poses, cov, n_frames, links, opts=None, frames=True):
        """The same from MV_POSE_DT records (poses in the reference frame)."""
        return self._hand_eye(self.L.ctag_mv_rig_hand_eye_fit, "ctag_mv_rig_hand_eye_fit", MV_POSE_DT, rigs, mv_poses, cov, n_frames, links, opts, frames)

    def _hand_eye_device(self, fn, name, rigs, poses_ptr, cov_ptr, n_frames, links, opts, out_ptr, frames_ptr):
        links = self._links(name, links, n_frames)
        st = fn(self.h, rigs.r, poses_ptr, cov_ptr, n_frames, links.ctypes.data, self._optp(opts), out_ptr, frames_ptr or None)
        if st != 0:
            raise CtagError(st, name)

    def fit_hand_eye_device(self, rigs, rig_poses_ptr, cov_ptr, n_frames, links, out_ptr, frames_ptr=None, opts=None):
        """Device RIG_POSE_DT / POSE_COV_DT records and host link poses -> n_rigs device HAND_EYE_DT records at out_ptr and, unless frames_ptr
        is None, n_frames * n_rigs HAND_EYE_FRAME_DT records at frames_ptr; enqueued."""
        self._hand_eye_device(self.L.ctag_rig_hand_eye_fit_device, "ctag_rig_hand_eye_fit_device", rigs, rig_poses_ptr, cov_ptr, n_frames, links, opts,
                              out_ptr, frames_ptr)

    def fit_mv_hand_eye_device(self, rigs, mv_poses_ptr, cov_ptr, n_frames, links, out_ptr, frames_ptr=None, opts=None):
        """The same from device MV_POSE_DT records."""
        self._hand_eye_device(self.L.ctag_mv_rig_hand_eye_fit_device, "ctag_mv_rig_hand_eye_fit_device", rigs, mv_poses_ptr, cov_ptr, n_frames, links,
                              opts, out_ptr, frames_ptr)

    def hand_eye_last_ms(self):
        """Device milliseconds of the last hand-eye call (needs OPT_TIMING): gather + start, the rounds, covariance + records, the whole call."""
        out = (C.c_float * 4)()
        self.L.ctag_hand_eye_last_ms(self.h, out)
        return dict(zip(("setup", "rounds", "finish", "total"), (float(v) for v in out)))

    # ---- pose covariance (include/ctag_pose.h): opts is a CovOptsC (cov_opts(...)) or None for the defaults
    @staticmethod
    def _optp(opts):
        return C.byref(opts) if opts is not None else None

    def pose_cov(self, result, poses, model, camera, opts=None):
        """One frame: its host ctag_frame_result record and the POSE_DT records of estimate_pose -> one POSE_COV_DT record per marker."""
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        n = int(res[0]["n_markers"]) if res[0]["status"] == 0 else 0
        poses = np.ascontiguousarray(poses, POSE_DT).reshape(-1)
        if len(poses) != n:
            raise ValueError("%d pose records for %d markers" % (len(poses), n))
        out = np.zeros(max(n, 1), POSE_COV_DT)
        st = self.L.ctag_estimate_pose_cov(self.h, res.ctypes.data, model.m, C.byref(camera), poses.ctypes.data if n else None,
                                           self._optp(opts), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_pose_cov")
        return out[:n]

    def pose_cov_batch_device(self, results_ptr, n_frames, model, camera, offsets_ptr, poses_ptr, capacity, out_ptr, opts=None):
        """Device pointers as pose_batch_device left them -> POSE_COV_DT record w for pose record w at out_ptr; enqueued, does not wait."""
        st = self.L.ctag_pose_cov_batch_device(self.h, results_ptr, n_frames, model.m, C.byref(camera), offsets_ptr, poses_ptr, capacity,
                                               self._optp(opts), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_pose_cov_batch_device")

    def rig_pose_cov(self, result, rig_poses, model, rigs, camera, opts=None):
        """One frame: its host record and the RIG_POSE_DT records of estimate_rig_pose -> rigs.n_rigs POSE_COV_DT records."""
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        rig_poses = np.ascontiguousarray(rig_poses, RIG_POSE_DT).reshape(-1)
        if len(rig_poses) != rigs.n_rigs:
            raise ValueError("%d rig pose records for %d rigs" % (len(rig_poses), rigs.n_rigs))
        out = np.zeros(rigs.n_rigs, POSE_COV_DT)
        st = self.L.ctag_estimate_rig_pose_cov(self.h, res.ctypes.data, model.m, rigs.r, C.byref(camera), rig_poses.ctypes.data,
                                               self._optp(opts), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_rig_pose_cov")
        return out

    def rig_pose_cov_batch_device(self, results_ptr, n_frames, model, rigs, camera, rig_poses_ptr, out_ptr, opts=None):
        """n_frames * rigs.n_rigs device RIG_POSE_DT records -> as many device POSE_COV_DT records at out_ptr; enqueued."""
        st = self.L.ctag_rig_pose_cov_batch_device(self.h, results_ptr, n_frames, model.m, rigs.r, C.byref(camera), rig_poses_ptr,
                                                   self._optp(opts), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_rig_pose_cov_batch_device")

    def mv_rig_pose_cov(self, results, mv_poses, model, rigs, cams, opts=None):
        """One instant: cams.n host records and the MV_POSE_DT records of estimate_mv_rig_pose -> rigs.n_rigs POSE_COV_DT records."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == RESULT_DT
        if len(res) != cams.n:
            raise ValueError("%d records for %d cameras" % (len(res), cams.n))
        mv_poses = np.ascontiguousarray(mv_poses, MV_POSE_DT).reshape(-1)
        if len(mv_poses) != rigs.n_rigs:
            raise ValueError("%d pose records for %d rigs" % (len(mv_poses), rigs.n_rigs))
        out = np.zeros(rigs.n_rigs, POSE_COV_DT)
        st = self.L.ctag_estimate_mv_rig_pose_cov(self.h, res.ctypes.data, model.m, rigs.r, cams.s, mv_poses.ctypes.data, self._optp(opts),
                                                  out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_mv_rig_pose_cov")
        return out

    def mv_rig_pose_cov_batch_device(self, results_ptrs, n_frames, model, rigs, cams, mv_poses_ptr, out_ptr, opts=None):
        """results_ptrs: one device pointer per camera; n_frames * rigs.n_rigs device MV_POSE_DT records -> as many POSE_COV_DT records."""
        ptrs = list(results_ptrs)
        if len(ptrs) != cams.n:
            raise ValueError("%d pointers for %d cameras" % (len(ptrs), cams.n))
        arr = (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(int(p) if p else None) for p in ptrs])
        st = self.L.ctag_mv_rig_pose_cov_batch_device(self.h, arr, n_frames, model.m, rigs.r, cams.s, mv_poses_ptr, self._optp(opts), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_mv_rig_pose_cov_batch_device")

    # ---- robust refit (include/ctag_pose.h): opts is a RobustOptsC (robust_opts(...)) or None for the defaults; apply_robust() puts the
    # refitted poses into the pose records for the covariance and overlay calls
    def robust_pose(self, result, poses, model, camera, opts=None):
        """One frame: its host ctag_frame_result record and the POSE_DT records of estimate_pose -> one ROBUST_POSE_DT record per marker."""
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        n = int(res[0]["n_markers"]) if res[0]["status"] == 0 else 0
        poses = np.ascontiguousarray(poses, POSE_DT).reshape(-1)
        if len(poses) != n:
            raise ValueError("%d pose records for %d markers" % (len(poses), n))
        out = np.zeros(max(n, 1), ROBUST_POSE_DT)
        st = self.L.ctag_estimate_pose_robust(self.h, res.ctypes.data, model.m, C.byref(camera), poses.ctypes.data if n else None,
                                           self._optp(opts), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_pose_robust")
        return out[:n]

    def robust_pose_batch_device(self, results_ptr, n_frames, model, camera, offsets_ptr, poses_ptr, capacity, out_ptr, opts=None):
        """Device pointers as pose_batch_device left them -> ROBUST_POSE_DT record w for pose record w at out_ptr; enqueued, does not wait."""
        st = self.L.ctag_pose_robust_batch_device(self.h, results_ptr, n_frames, model.m, C.byref(camera), offsets_ptr, poses_ptr, capacity,
                                               self._optp(opts), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_pose_robust_batch_device")

    def robust_rig_pose(self, result, rig_poses, model, rigs, camera, opts=None):
        """One frame: its host record and the RIG_POSE_DT records of estimate_rig_pose -> rigs.n_rigs ROBUST_POSE_DT records."""
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        rig_poses = np.ascontiguousarray(rig_poses, RIG_POSE_DT).reshape(-1)
        if len(rig_poses) != rigs.n_rigs:
            raise ValueError("%d rig pose records for %d rigs" % (len(rig_poses), rigs.n_rigs))
        out = np.zeros(rigs.n_rigs, ROBUST_POSE_DT)
        st = self.L.ctag_estimate_rig_pose_robust(self.h, res.ctypes.data, model.m, rigs.r, C.byref(camera), rig_poses.ctypes.data,
                                               self._optp(opts), out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_rig_pose_robust")
        return out

    def robust_rig_pose_batch_device(self, results_ptr, n_frames, model, rigs, camera, rig_poses_ptr, out_ptr, opts=None):
        """n_frames * rigs.n_rigs device RIG_POSE_DT records -> as many device ROBUST_POSE_DT records at out_ptr; enqueued."""
        st = self.L.ctag_rig_pose_robust_batch_device(self.h, results_ptr, n_frames, model.m, rigs.r, C.byref(camera), rig_poses_ptr,
                                                   self._optp(opts), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_rig_pose_robust_batch_device")

    def robust_mv_rig_pose(self, results, mv_poses, model, rigs, cams, opts=None):
        """One instant: cams.n host records and the MV_POSE_DT records of estimate_mv_rig_pose -> rigs.n_rigs ROBUST_POSE_DT records."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == RESULT_DT
        if len(res) != cams.n:
            raise ValueError("%d records for %d cameras" % (len(res), cams.n))
        mv_poses = np.ascontiguousarray(mv_poses, MV_POSE_DT).reshape(-1)
        if len(mv_poses) != rigs.n_rigs:
            raise ValueError("%d pose records for %d rigs" % (len(mv_poses), rigs.n_rigs))
        out = np.zeros(rigs.n_rigs, ROBUST_POSE_DT)
        st = self.L.ctag_estimate_mv_rig_pose_robust(self.h, res.ctypes.data, model.m, rigs.r, cams.s, mv_poses.ctypes.data, self._optp(opts),
                                                  out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_estimate_mv_rig_pose_robust")
        return out

    def robust_mv_rig_pose_batch_device(self, results_ptrs, n_frames, model, rigs, cams, mv_poses_ptr, out_ptr, opts=None):
        """results_ptrs: one device pointer per camera; n_frames * rigs.n_rigs device MV_POSE_DT records -> as many ROBUST_POSE_DT records."""
        ptrs = list(results_ptrs)
        if len(ptrs) != cams.n:
            raise ValueError("%d pointers for %d cameras" % (len(ptrs), cams.n))
        arr = (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(int(p) if p else None) for p in ptrs])
        st = self.L.ctag_mv_rig_pose_robust_batch_device(self.h, arr, n_frames, model.m, rigs.r, cams.s, mv_poses_ptr, self._optp(opts), out_ptr)
        if st != 0:
            raise CtagError(st, "ctag_mv_rig_pose_robust_batch_device")

    # ---- overlay (CylinderTag::drawAxis)
    def draw_axis(self, gray, result, poses, model, camera, axis_length=5, out=None):
        """One frame: gray (rows x cols uint8) + its ctag_frame_result + POSE_DT records -> rows x cols x 3 uint8 overlay.
        Record k draws marker poses[k]["marker"] with model poses[k]["model_index"] (frame field 0).  `out` may be a
        (rows, cols, 3) uint8 view with any row stride (e.g. a slice of a wider buffer); only its pixels are written."""
        gray = np.asarray(gray)
        assert gray.dtype == np.uint8 and gray.ndim == 2 and gray.strides[1] == 1
        res = np.ascontiguousarray(result).reshape(1)
        assert res.dtype == RESULT_DT
        poses = np.ascontiguousarray(poses, POSE_DT).reshape(-1)
        rows, cols = gray.shape
        if out is None:
            out = np.empty((rows, cols, 3), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (rows, cols, 3) and out.strides[1:] == (3, 1)
        st = self.L.ctag_draw_axis(self.h, gray.ctypes.data, rows, cols, gray.strides[0], res.ctypes.data,
                                   poses.ctypes.data if poses.size else None, poses.size, model.m, C.byref(camera),
                                   int(axis_length), out.ctypes.data, out.strides[0])
        if st != 0:
            raise CtagError(st, "ctag_draw_axis")
        return out

    def draw_axis_batch_device(self, frames_ptr, n, rows, cols, row_stride, frame_stride, results_ptr, offsets_ptr, poses_ptr,
                               capacity, model, camera, axis_length, out_ptr, out_row_stride, out_frame_stride):
        """Device pointers throughout (ctag_pose_batch_device's offsets / poses as they are); enqueued, does not wait."""
        st = self.L.ctag_draw_axis_batch_device(self.h, frames_ptr, n, rows, cols, row_stride, frame_stride, results_ptr, offsets_ptr,
                                                poses_ptr, capacity, model.m, C.byref(camera), int(axis_length), out_ptr,
                                                out_row_stride, out_frame_stride)
        if st != 0:
            raise CtagError(st, "ctag_draw_axis_batch_device")
