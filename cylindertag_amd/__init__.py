"""cylindertag_amd -- MI355X-native CylinderTag detection front end.

The product is the C-ABI shared library ``cylindertag_amd/_build/libctag_hip.so`` (hand-written HIP kernels for
gfx950, sources in ``cylindertag_amd/csrc``) plus the C++ class ``CylinderTag`` that mirrors the reference
interface (``csrc/CylinderTag.h``).  This Python module is only the thin ctypes binding the test-suite and
``bench.py`` use to drive that ABI; it contains no detection logic and no CPU fallback -- if the HIP library is
missing or no GPU is usable, construction raises.
"""
from .capi import (CameraC, ParamsC, default_params, CtagError, Detector, Model, POSE_DT, RIG_POSE_DT, MV_POSE_DT, POSE_COV_DT, CovOptsC, cov_opts, ROBUST_POSE_DT, RobustOptsC, robust_opts, apply_robust, TRACK_DT, TRACK_STAT_DT, TrackOptsC, track_opts, TRACK_NOISE_DT, TrackNoiseOptsC, track_noise_opts, apply_track_noise, LINK_POSE_DT, HAND_EYE_DT, HAND_EYE_FRAME_DT, HandEyeOptsC, hand_eye_opts, MODEL_FIT_STAT_DT, ModelFitOptsC, model_fit_opts, RIG_FIT_STAT_DT, RIG_FIT_MODEL_STAT_DT, RigFitOptsC, rig_fit_opts, CAMERA_FIT_STAT_DT, CAMERA_FIT_CAM_STAT_DT, CameraFitOptsC, camera_fit_opts, INTRINSICS_FIT_STAT_DT, INTR_PARAM_NAMES, IntrinsicsFitOptsC, intrinsics_fit_opts, Rigs, CameraSet, CameraPoseC, load_camera, make_camera, FEATURE_DT, MARKER_DT, RESULT_DT, STAGE_NAMES, build, lib_path, load_library,
                   load_marker_file, pinned_empty)

__all__ = ["CameraC", "ParamsC", "default_params", "Model", "POSE_DT", "RIG_POSE_DT", "MV_POSE_DT", "POSE_COV_DT", "CovOptsC", "cov_opts", "ROBUST_POSE_DT", "RobustOptsC", "robust_opts", "apply_robust", "TRACK_DT", "TRACK_STAT_DT", "TrackOptsC", "track_opts", "LINK_POSE_DT", "HAND_EYE_DT", "HAND_EYE_FRAME_DT", "HandEyeOptsC", "hand_eye_opts", "MODEL_FIT_STAT_DT", "ModelFitOptsC", "model_fit_opts", "RIG_FIT_STAT_DT", "RIG_FIT_MODEL_STAT_DT", "RigFitOptsC", "rig_fit_opts", "CAMERA_FIT_STAT_DT", "CAMERA_FIT_CAM_STAT_DT", "CameraFitOptsC", "camera_fit_opts", "INTRINSICS_FIT_STAT_DT", "INTR_PARAM_NAMES", "IntrinsicsFitOptsC", "intrinsics_fit_opts", "Rigs", "CameraSet", "CameraPoseC", "load_camera", "make_camera", "CtagError", "Detector", "FEATURE_DT", "MARKER_DT", "RESULT_DT", "STAGE_NAMES", "build", "lib_path",
           "load_library", "load_marker_file", "pinned_empty"]
