"""ctypes binding of include/ctag_testkit.h (testkit/_build/libctag_testkit.so): TEST AND BENCH SCAFFOLDING around the
product library -- parity probes, device evaluation of the shared math, the synthetic frame generators and the one-GPU
execution of the multi-rank unpack.  Nothing in cylindertag_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import cylindertag_amd as ca
from cylindertag_amd import capi
from cylindertag_amd.capi import CtagError, Model

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("CTAG_TESTKIT_LIB") or os.path.join(_HERE, "_build", "libctag_testkit.so")

TRUTH3D_DT = np.dtype([("n_markers", "<i4"), ("dict_row", "<i4", (8,)), ("_pad", "<i4", (1,)), ("R", "<f8", (8, 9)), ("t", "<f8", (8, 3)),
                       ("radius", "<f8", (8,))])
TRUTH_DT = np.dtype([("n_markers", "<i4"), ("dict_row", "<i4", (8,)), ("strip_len", "<f4", (8,)),
                     ("corners", "<f4", (8, 8))])
DBG_HALF, DBG_LABELS, DBG_CANDIDATES, DBG_CAND_QUADS, DBG_FEATURES0, DBG_FEATURES1, DBG_FEATURES2, DBG_PREMARKERS, DBG_GRAY, DBG_LINES, DBG_MASK, DBG_LINE_POINTS, DBG_LINE_FITS, DBG_PACKS, DBG_PACKS1 = range(1, 16)
SYNTH_SEED = 0x4354616753594E00  # "CTagSYN\0", SURVEY.md 8(d)

# every symbol include/ctag_testkit.h declares (tests check the library exports all of them)
EXPORTS = ["ctag_debug_fetch", "ctag_math_probe", "ctag_testkit_wave_probe", "ctag_testkit_exp32_k0_sweep", "ctag_testkit_unpack_gathered", "ctag_testkit_stall_stream", "ctag_synth_frames_device", "ctag_synth_frame_host",
           "ctag_synth_layout_truth", "ctag_synth3d_frames_device", "ctag_synth3d_frame_host", "ctag_synth3d_model",
           "ctag_testkit_dense_edge_probe", "ctag_testkit_plan", "ctag_testkit_welsch_fit", "ctag_testkit_welsch_limits", "ctag_testkit_refine_sums",
           "ctag_testkit_model_fit_system", "ctag_testkit_model_fit_limits", "ctag_testkit_rig_fit_system", "ctag_testkit_rig_fit_limits",
           "ctag_testkit_camera_fit_system", "ctag_testkit_camera_fit_limits",
           "ctag_testkit_intrinsics_fit_system", "ctag_testkit_intrinsics_fit_poses", "ctag_testkit_intrinsics_fit_limits"]
# the fields ctag_testkit_plan writes, in order (cylindertag_amd/csrc/ctag_internal.h: ChunkPlan)
PLAN_FIELDS = ("fused", "bgr_direct", "zero_first", "dec_zero_kernel", "dec_zero_list", "dec", "dec_xblocks", "dec_yblocks", "dec_band_rows", "dec_bands",
               "ccl", "latency", "small_cfg", "refprm", "mask_scan", "prescan", "all_wave", "fork", "pack_max", "big_points", "pack_gx", "scan_gx",
               "mscan_gx", "big_cols", "big_max_gx", "welsch_gs", "welsch_gx", "refine", "refine_gx", "refine_sums_gx")
DEC_FORMS = ("mask", "mask_bands", "general", "wide", "banded135", "banded", "unaligned")  # ChunkPlan::dec
CCL_FORMS = ("mask", "tw5", "any")                                                          # ChunkPlan::ccl
# the values ctag_testkit_welsch_limits writes, in order (cylindertag_amd/csrc/k_quad.hip: welsch_limits)
WELSCH_LIMITS = ("kWShort", "kWCap", "kWRes", "kWPts", "kWPtsU", "kPickN", "kPickN2", "kWE", "kWT", "kLatLines", "kLatPoints", "kLatChunk", "kLdsLines",
                 "kLatencyFrames", "kLatRankBlocks", "kLineSortBuckets")
REFINE_FORMS = ("none", "one", "split_large", "split_looping", "split")                     # ChunkPlan::refine
# op codes of Detector.math (ctag_math_probe; oracle/ctag_oracle.h lists them) that tests name
MATH_EXP32_NONPOS, MATH_EXP32_NONPOS_K0, MATH_LOG64 = 15, 17, 18
# op codes of Detector.wave (ctag_testkit_wave_probe; include/ctag_testkit.h: CTAG_WAVE_*), in the header's order
WAVE_OPS = ("FROM_PREV", "FROM_NEXT", "SHR1_I32", "SHR2_I32", "SHR4_I32", "SHR1_F32", "SHR1_F64", "XOR1_I32", "XOR2_I32", "HALF_MIRROR_I32", "ROW_MIRROR_I32",
            "XOR1_I64", "XOR2_I64", "HALF_MIRROR_I64", "ROW_MIRROR_I64", "INCL_SCAN", "SG_SUM8_I32", "SG_SUM64_I32", "SG_SUM8_I64", "SG_SUM64_I64",
            "SG_BEST8_NEAREST", "SG_BEST8_FARTHEST", "SG_BEST64_NEAREST", "SG_BEST64_FARTHEST", "SUM_F64", "MAX_F64", "ALL", "PK_MIN_U16", "PK_MAX_U16")
for _i, _n in enumerate(WAVE_OPS):
    globals()["WAVE_" + _n] = _i
WAVE_SENTINEL_F64, WAVE_SENTINEL_I64 = -12345.6789, -0x5a5a5a5a5a5a5a5a  # what a lane that was off keeps (CTAG_WAVE_SENTINEL_*)


def lib_path():
    return _LIB


def build(verbose=False):
    """Compile the product library and the test kit in-tree."""
    ca.build(verbose)
    subprocess.check_call(["make", "-C", _HERE] + ([] if verbose else ["-s"]))


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    capi.load_library()  # the product library first (and torch's HIP runtime before it)
    if not os.path.exists(_LIB):
        raise FileNotFoundError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % _LIB)
    L = C.CDLL(_LIB)
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    L.ctag_debug_fetch.restype = C.c_long
    L.ctag_debug_fetch.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.ctag_math_probe.restype = C.c_int
    L.ctag_math_probe.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.ctag_testkit_wave_probe.restype = C.c_int
    L.ctag_testkit_wave_probe.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.ctag_testkit_exp32_k0_sweep.restype = C.c_int
    L.ctag_testkit_exp32_k0_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.ctag_testkit_unpack_gathered.restype = C.c_int
    L.ctag_testkit_unpack_gathered.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint64, vp]
    L.ctag_testkit_stall_stream.restype = C.c_int
    L.ctag_testkit_stall_stream.argtypes = [vp, C.c_int]
    L.ctag_synth_frames_device.restype = C.c_int
    L.ctag_synth_frames_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t,
                                           C.c_uint64, C.c_int]
    L.ctag_synth_frame_host.restype = C.c_int
    L.ctag_synth_frame_host.argtypes = [i32p, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_uint64,
                                        C.c_int, vp]
    L.ctag_synth_layout_truth.restype = C.c_int
    L.ctag_synth_layout_truth.argtypes = [i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, vp]
    L.ctag_synth3d_frames_device.restype = C.c_int
    L.ctag_synth3d_frames_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_uint64, C.c_int,
                                             C.c_double, C.c_double, C.c_double, C.c_double]
    L.ctag_synth3d_frame_host.restype = C.c_int
    L.ctag_synth3d_frame_host.argtypes = [i32p, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_uint64, C.c_int, C.c_double,
                                          C.c_double, C.c_double, C.c_double, vp]
    L.ctag_synth3d_model.restype = C.c_int
    L.ctag_synth3d_model.argtypes = [i32p, C.c_int, C.c_int, vp]
    L.ctag_testkit_plan.restype = C.c_int
    L.ctag_testkit_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_int, C.c_int,
                                    C.c_int, i32p, C.c_int]
    L.ctag_testkit_dense_edge_probe.restype = C.c_int
    L.ctag_testkit_dense_edge_probe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                                C.c_double, C.c_double, vp, vp]
    L.ctag_testkit_welsch_fit.restype = C.c_int
    L.ctag_testkit_welsch_fit.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.ctag_testkit_refine_sums.restype = C.c_int
    L.ctag_testkit_refine_sums.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.ctag_testkit_welsch_limits.restype = C.c_int
    L.ctag_testkit_welsch_limits.argtypes = [i32p, C.c_int]
    L.ctag_testkit_model_fit_system.restype = C.c_int
    L.ctag_testkit_model_fit_system.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.POINTER(capi.CameraC), C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, vp,
                                                vp, i32p]
    L.ctag_testkit_model_fit_limits.restype = C.c_int
    L.ctag_testkit_model_fit_limits.argtypes = [i32p, C.c_int]
    L.ctag_testkit_rig_fit_system.restype = C.c_int
    L.ctag_testkit_rig_fit_system.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.POINTER(capi.CameraC), C.c_int, C.c_double, C.c_int, vp, vp, vp, i32p, i32p]
    L.ctag_testkit_rig_fit_limits.restype = C.c_int
    L.ctag_testkit_rig_fit_limits.argtypes = [i32p, C.c_int]
    L.ctag_testkit_camera_fit_system.restype = C.c_int
    L.ctag_testkit_camera_fit_system.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_double, C.c_int, vp, vp, vp, i32p, i32p]
    L.ctag_testkit_camera_fit_limits.restype = C.c_int
    L.ctag_testkit_camera_fit_limits.argtypes = [i32p, C.c_int]
    L.ctag_testkit_intrinsics_fit_system.restype = C.c_int
    L.ctag_testkit_intrinsics_fit_system.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.POINTER(capi.CameraC), C.c_uint32, C.c_int, C.c_double, C.c_int, vp, vp, vp,
                                                     i32p, i32p]
    L.ctag_testkit_intrinsics_fit_poses.restype = C.c_int
    L.ctag_testkit_intrinsics_fit_poses.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.POINTER(capi.CameraC), vp, i32p]
    L.ctag_testkit_intrinsics_fit_limits.restype = C.c_int
    L.ctag_testkit_intrinsics_fit_limits.argtypes = [i32p, C.c_int]
    _lib = L
    return L


def exp32_k0_sweep(first_bits, last_bits, step=1):
    """exp32_nonpos_k0 / exp32_k_is_zero against exp32_nonpos on the host over the floats of bit patterns first_bits, first_bits + step, ... <= last_bits
    (ctag_testkit_exp32_k0_sweep) -> dict of visited, k_is_zero, predicate_mismatches, bit_mismatches, first_bad (a bit pattern, or None).  Host only."""
    counts = (C.c_uint64 * 4)()
    first_bad = C.c_uint32()
    st = load_library().ctag_testkit_exp32_k0_sweep(int(first_bits), int(last_bits), int(step), counts, C.byref(first_bad))
    if st != 0:
        raise CtagError(st, "ctag_testkit_exp32_k0_sweep")
    out = dict(zip(("visited", "k_is_zero", "predicate_mismatches", "bit_mismatches"), (int(v) for v in counts)))
    out["first_bad"] = int(first_bad.value) if out["predicate_mismatches"] or out["bit_mismatches"] else None
    return out


def model_fit_limits():
    """k_mfit_record's grid and the observation records one pass of the fit's workspace holds (ctag_testkit_model_fit_limits).  Host only."""
    out = np.zeros(2, np.int32)
    n = load_library().ctag_testkit_model_fit_limits(out.ctypes.data_as(C.POINTER(C.c_int32)), 2)
    if n != 2:
        raise RuntimeError("ctag_testkit_model_fit_limits writes %d values" % n)
    return {"record_grid": int(out[0]), "pass_records": int(out[1])}


def rig_fit_limits():
    """k_rfit_record's grid and the observation records one pass of the rig assembly's workspace holds (ctag_testkit_rig_fit_limits).  Host only."""
    out = np.zeros(2, np.int32)
    n = load_library().ctag_testkit_rig_fit_limits(out.ctypes.data_as(C.POINTER(C.c_int32)), 2)
    if n != 2:
        raise RuntimeError("ctag_testkit_rig_fit_limits writes %d values" % n)
    return {"record_grid": int(out[0]), "pass_records": int(out[1])}


def camera_fit_limits():
    """k_cfit_record's grid and the observation records one pass of the camera set fit's workspace holds (ctag_testkit_camera_fit_limits).  Host only."""
    out = np.zeros(2, np.int32)
    n = load_library().ctag_testkit_camera_fit_limits(out.ctypes.data_as(C.POINTER(C.c_int32)), 2)
    if n != 2:
        raise RuntimeError("ctag_testkit_camera_fit_limits writes %d values" % n)
    return {"record_grid": int(out[0]), "pass_records": int(out[1])}


def intrinsics_fit_limits():
    """The grid of k_ifit_record / k_ifit_pose and the observation records one pass of the intrinsics fit's workspace holds
    (ctag_testkit_intrinsics_fit_limits).  Host only."""
    out = np.zeros(2, np.int32)
    n = load_library().ctag_testkit_intrinsics_fit_limits(out.ctypes.data_as(C.POINTER(C.c_int32)), 2)
    if n != 2:
        raise RuntimeError("ctag_testkit_intrinsics_fit_limits writes %d values" % n)
    return {"record_grid": int(out[0]), "pass_records": int(out[1])}


def synth_frame_host(state, frame_index, rows=1080, cols=1920, seed=SYNTH_SEED, markers=4):
    """Host rendering of synthetic frame `frame_index` (same code path as the device generator)."""
    L = load_library()
    state = np.ascontiguousarray(state, dtype=np.int32)
    img = np.zeros((rows, cols), np.uint8)
    truth = np.zeros(1, TRUTH_DT)
    st = L.ctag_synth_frame_host(state.ctypes.data_as(C.POINTER(C.c_int32)), state.shape[0], state.shape[1],
                                 img.ctypes.data, frame_index, rows, cols, img.strides[0], seed, markers,
                                 truth.ctypes.data)
    if st != 0:
        raise CtagError(st)
    return img, truth[0]


def synth3d_frame_host(state, frame_index, K, rows=2160, cols=3840, seed=SYNTH_SEED, markers=4):
    """Host rendering of frame `frame_index` of the 3-D scene (cylinders with planted poses, camera matrix K) -> (image, truth)."""
    L = load_library()
    state = np.ascontiguousarray(state, dtype=np.int32)
    img = np.zeros((rows, cols), np.uint8)
    truth = np.zeros(1, TRUTH3D_DT)
    K = np.asarray(K, np.float64)
    st = L.ctag_synth3d_frame_host(state.ctypes.data_as(C.POINTER(C.c_int32)), state.shape[0], state.shape[1], img.ctypes.data, frame_index,
                                   rows, cols, img.strides[0], seed, markers, K[0, 0], K[1, 1], K[0, 2], K[1, 2], truth.ctypes.data)
    if st != 0:
        raise CtagError(st, "ctag_synth3d_frame_host")
    return img, truth[0]


def synth3d_model(state):
    """3-D corner lists of the synthetic cylinders, one model per dictionary row (marker id = row) -> Model."""
    L = load_library()
    state = np.ascontiguousarray(state, dtype=np.int32)
    corners = np.zeros((state.shape[0], state.shape[1] * 8, 3), np.float32)
    st = L.ctag_synth3d_model(state.ctypes.data_as(C.POINTER(C.c_int32)), state.shape[0], state.shape[1], corners.ctypes.data)
    if st != 0:
        raise CtagError(st, "ctag_synth3d_model")
    return Model(ids=np.arange(state.shape[0], dtype=np.int32), corners=corners, model_size=state.shape[1]), corners


def synth_truth(state, frame_index, rows=1080, cols=1920, seed=SYNTH_SEED, markers=4):
    """Planted markers (dictionary rows, strip corners) of synthetic frame `frame_index`, without rendering."""
    L = load_library()
    state = np.ascontiguousarray(state, dtype=np.int32)
    truth = np.zeros(1, TRUTH_DT)
    st = L.ctag_synth_layout_truth(state.ctypes.data_as(C.POINTER(C.c_int32)), state.shape[0], state.shape[1], frame_index, rows,
                                   cols, seed, markers, truth.ctypes.data)
    if st != 0:
        raise CtagError(st)
    return truth[0]


def chunk_plan(rows, cols, nframes, adaptive_thresh=5, channels=1, corner_subpix=1, frames=0x10000, frame_stride=None, row_stride=None,
               fuse_mode=-1, wave_points=0, bgr_direct=1, expand_exact=0):
    """The kernel forms the library picks for a chunk (ctag_testkit_plan) as a dict over PLAN_FIELDS; the forms by name.  Host only.
    `frames` is an address (never read); the strides default to packed rows."""
    L = load_library()
    row_stride = cols * channels if row_stride is None else row_stride
    frame_stride = row_stride * rows if frame_stride is None else frame_stride
    out = np.zeros(len(PLAN_FIELDS), np.int32)
    n = L.ctag_testkit_plan(rows, cols, adaptive_thresh, nframes, channels, corner_subpix, frames, frame_stride, row_stride, fuse_mode, wave_points,
                            bgr_direct, expand_exact, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    if n != len(PLAN_FIELDS):
        raise RuntimeError("ctag_testkit_plan writes %d fields, PLAN_FIELDS names %d" % (n, len(PLAN_FIELDS)))
    plan = dict(zip(PLAN_FIELDS, (int(v) for v in out)))
    plan["dec"], plan["ccl"], plan["refine"] = DEC_FORMS[plan["dec"]], CCL_FORMS[plan["ccl"]], REFINE_FORMS[plan["refine"]]
    return plan


def welsch_limits():
    """The sizes at which the Welsch fit kernels change form (ctag_testkit_welsch_limits) as a dict over WELSCH_LIMITS.  Host only."""
    L = load_library()
    out = np.zeros(len(WELSCH_LIMITS), np.int32)
    n = L.ctag_testkit_welsch_limits(out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    if n != len(WELSCH_LIMITS):
        raise RuntimeError("ctag_testkit_welsch_limits writes %d values, WELSCH_LIMITS names %d" % (n, len(WELSCH_LIMITS)))
    return dict(zip(WELSCH_LIMITS, (int(v) for v in out)))


class Detector(ca.Detector):
    """The product's Detector plus the test kit's entry points on the same handle."""

    def __init__(self, state, feature_size, device=0, **kw):
        super().__init__(state, feature_size, device=device, **kw)
        self.T = load_library()

    def synth_frames_device(self, frames_ptr, first, n, rows, cols, row_stride, frame_stride, seed=SYNTH_SEED, markers=4):
        st = self.T.ctag_synth_frames_device(self.h, frames_ptr, first, n, rows, cols, row_stride, frame_stride, seed, markers)
        if st != 0:
            raise CtagError(st, "ctag_synth_frames_device")

    def synth3d_frames_device(self, frames_ptr, first, n, rows, cols, row_stride, frame_stride, K, seed=SYNTH_SEED, markers=4):
        K = np.asarray(K, np.float64)
        st = self.T.ctag_synth3d_frames_device(self.h, frames_ptr, first, n, rows, cols, row_stride, frame_stride, seed, markers,
                                               K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        if st != 0:
            raise CtagError(st, "ctag_synth3d_frames_device")

    def stall_stream(self, milliseconds):
        """A kernel that spins for `milliseconds` on the handle's stream: a late peer, as the gather's bounded waits see one."""
        st = self.T.ctag_testkit_stall_stream(self.h, int(milliseconds))
        if st != 0:
            raise CtagError(st, "ctag_testkit_stall_stream")

    def unpack_gathered(self, gathered_ptr, n_total, world, width, out_ptr):
        """ctag_gather_end's segment table + unpack kernels for a `world`-rank job on a caller-built gathered buffer."""
        self._gcheck(self.T.ctag_testkit_unpack_gathered(self.h, gathered_ptr, n_total, world, width, out_ptr), "ctag_testkit_unpack_gathered")

    def debug(self, frame, what):
        n = self.T.ctag_debug_fetch(self.h, frame, what, None, 0)
        if n < 0:
            raise CtagError(-1, "ctag_debug_fetch(%d)" % what)
        if what in (DBG_HALF, DBG_GRAY, DBG_MASK):
            a = np.zeros(n, np.uint8)
        elif what in (DBG_LABELS, DBG_CANDIDATES, DBG_LINES, DBG_LINE_POINTS, DBG_PACKS, DBG_PACKS1):
            a = np.zeros(n, np.int32)
        elif what == DBG_PREMARKERS:
            a = np.zeros(1, ca.RESULT_DT)
        else:
            a = np.zeros(n, np.float32)
        if n:
            got = self.T.ctag_debug_fetch(self.h, frame, what, a.ctypes.data, max(n, 1))
            if got < 0:
                raise CtagError(-2, "ctag_debug_fetch(%d)" % what)
        if what in (DBG_CANDIDATES, DBG_CAND_QUADS):
            return a.reshape(-1, 8)
        if what in (DBG_FEATURES0, DBG_FEATURES1, DBG_FEATURES2):
            return a.reshape(-1, 19)
        if what == DBG_PREMARKERS:
            return a[0]
        if what == DBG_LINE_POINTS:
            return a.reshape(-1, 2)
        if what == DBG_LINE_FITS:
            return a.reshape(-1, 4)
        return a

    def welsch_fit(self, frames, latency=0, welsch_gx=0, welsch_gs=0, tail_at_pool_end=False):
        """The Welsch fit stage alone (ctag_testkit_welsch_fit) on the workspace of the last chunk: `frames` is a list of frames, each a list
        of (n, 2) integer point clusters -> float32 [sum edges, 4] lines in input order.  Raises CtagError where the probe refuses the input."""
        clusters = [np.asarray(c, np.int32).reshape(-1, 2) for f in frames for c in f]
        edges = np.array([len(f) for f in frames], np.int32)
        counts = np.array([len(c) for c in clusters], np.int32)
        xy = np.ascontiguousarray(np.concatenate(clusters) if clusters else np.zeros((0, 2)), np.int32)
        lines = np.zeros((len(clusters), 4), np.float32)
        st = self.T.ctag_testkit_welsch_fit(self.h, len(frames), edges.ctypes.data, counts.ctypes.data, xy.ctypes.data, int(latency), int(welsch_gx),
                                            int(welsch_gs), int(bool(tail_at_pool_end)), lines.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_testkit_welsch_fit")
        return lines

    def refine_sums(self, nfeat, status, corners, n0):
        """edgeRefine's sums kernel alone (ctag_testkit_refine_sums) on the workspace of the last chunk: nfeat, status per frame; corners float32
        [sum nfeat, 16]; n0 float64 [sum 2 nfeat, 4, 128] -> float64 [sum 2 nfeat, 49], the first 49 doubles of every quad's block after the kernel."""
        nfeat = np.ascontiguousarray(nfeat, np.int32)
        status = np.ascontiguousarray(status, np.int32)
        nq = 2 * int(nfeat.sum())
        corners = np.ascontiguousarray(corners, np.float32).reshape(nq // 2, 16)
        n0 = np.ascontiguousarray(n0, np.float64).reshape(nq, 4, 128)
        sums = np.zeros((nq, 49), np.float64)
        st = self.T.ctag_testkit_refine_sums(self.h, len(nfeat), nfeat.ctypes.data, status.ctypes.data, corners.ctypes.data, n0.ctypes.data, sums.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_testkit_refine_sums")
        return sums

    def model_fit_system(self, results, poses, model, camera, model_index, lam, min_obs=2, pass_records=0):
        """The reduced system of the model reconstruction for one model at a given state (ctag_testkit_model_fit_system): host detection
        records, POSE_DT records over them, a Model -> dict of S [3P, 3P], g [3P], delta [3P], held [P] bool, bad_pivot bool."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == ca.RESULT_DT
        poses = np.ascontiguousarray(poses, ca.POSE_DT).reshape(-1)
        P = int(model.view()["size"]) * 8
        S, g, d = np.zeros((3 * P, 3 * P)), np.zeros(3 * P), np.zeros(3 * P)
        held = np.zeros(P, np.int32)
        bad = C.c_int32()
        st = self.T.ctag_testkit_model_fit_system(self.h, res.ctypes.data, len(res), poses.ctypes.data, len(poses), model.m, C.byref(camera),
                                                  int(model_index), float(lam), int(min_obs), int(pass_records), S.ctypes.data, g.ctypes.data,
                                                  d.ctypes.data, held.ctypes.data, C.byref(bad))
        if st != 0:
            raise CtagError(st, "ctag_testkit_model_fit_system")
        return {"S": S, "g": g, "delta": d, "held": held.astype(bool), "bad_pivot": bool(bad.value)}

    def rig_fit_system(self, results, rig_poses, model, rigs, camera, rig, lam, pass_records=0):
        """The reduced system of the rig assembly for one rig at a given state (ctag_testkit_rig_fit_system): host detection records, the
        RIG_POSE_DT records over them on `model` with `rigs` -> dict of S [N, N], g [N], delta [N] (N = 6 x the rig's models, the first
        model's rows being the dropped anchor's), bad_pivot bool."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == ca.RESULT_DT
        recs = np.ascontiguousarray(rig_poses, ca.RIG_POSE_DT).reshape(-1)
        assert len(recs) == len(res) * rigs.n_rigs
        S, g, d = np.zeros(96 * 96), np.zeros(96), np.zeros(96)
        n, bad = C.c_int32(), C.c_int32()
        st = self.T.ctag_testkit_rig_fit_system(self.h, res.ctypes.data, len(res), recs.ctypes.data, model.m, rigs.r, C.byref(camera), int(rig),
                                                float(lam), int(pass_records), S.ctypes.data, g.ctypes.data, d.ctypes.data, C.byref(n), C.byref(bad))
        if st != 0:
            raise CtagError(st, "ctag_testkit_rig_fit_system")
        N = int(n.value)
        return {"S": S[:N * N].reshape(N, N).copy(), "g": g[:N].copy(), "delta": d[:N].copy(), "bad_pivot": bool(bad.value)}

    def camera_fit_system(self, results, mv_poses, model, rigs, camera_set, anchor, lam, pass_records=0):
        """The reduced system of the camera set fit at a given state (ctag_testkit_camera_fit_system): host detection records [camera][frame],
        the MV_POSE_DT records over them under `camera_set` -> dict of S [N, N], g [N], delta [N] (N = 6 x the set's cameras, camera
        `anchor`'s rows dropped), bad_pivot bool."""
        res = np.ascontiguousarray(results)
        assert res.dtype == ca.RESULT_DT and res.ndim == 2 and res.shape[0] == camera_set.n
        recs = np.ascontiguousarray(mv_poses, ca.MV_POSE_DT).reshape(-1)
        assert len(recs) == res.shape[1] * rigs.n_rigs
        S, g, d = np.zeros(48 * 48), np.zeros(48), np.zeros(48)
        n, bad = C.c_int32(), C.c_int32()
        st = self.T.ctag_testkit_camera_fit_system(self.h, res.ctypes.data, res.shape[1], recs.ctypes.data, model.m, rigs.r, camera_set.s, int(anchor),
                                                   float(lam), int(pass_records), S.ctypes.data, g.ctypes.data, d.ctypes.data, C.byref(n), C.byref(bad))
        if st != 0:
            raise CtagError(st, "ctag_testkit_camera_fit_system")
        N = int(n.value)
        return {"S": S[:N * N].reshape(N, N).copy(), "g": g[:N].copy(), "delta": d[:N].copy(), "bad_pivot": bool(bad.value)}

    def intrinsics_fit_system(self, results, rig_poses, model, rigs, camera, lam, free_mask=0, tie_focal=0, pass_records=0):
        """The reduced system of the intrinsics fit at a given state (ctag_testkit_intrinsics_fit_system): host detection records, the
        RIG_POSE_DT records over them (the CTAG_POSE_OK ones are the observations, their rvec / tvec the view poses) and the camera ->
        dict of S [16, 16], g [16], delta [16], n_free, bad_pivot bool."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == ca.RESULT_DT
        recs = np.ascontiguousarray(rig_poses, ca.RIG_POSE_DT).reshape(-1)
        assert len(recs) == len(res) * rigs.n_rigs
        S, g, d = np.zeros((16, 16)), np.zeros(16), np.zeros(16)
        n, bad = C.c_int32(), C.c_int32()
        st = self.T.ctag_testkit_intrinsics_fit_system(self.h, res.ctypes.data, len(res), recs.ctypes.data, model.m, rigs.r, C.byref(camera), int(free_mask),
                                                       int(tie_focal), float(lam), int(pass_records), S.ctypes.data, g.ctypes.data, d.ctypes.data, C.byref(n),
                                                       C.byref(bad))
        if st != 0:
            raise CtagError(st, "ctag_testkit_intrinsics_fit_system")
        return {"S": S, "g": g, "delta": d, "n_free": int(n.value), "bad_pivot": bool(bad.value)}

    def intrinsics_fit_poses(self, results, rig_poses, model, rigs, camera):
        """Rule 4 of the intrinsics fit alone (ctag_testkit_intrinsics_fit_poses): every CTAG_POSE_OK record's view pose under `camera`,
        started from the record's own -> (RIG_POSE_DT records with rvec, tvec, cost replaced, usable bool)."""
        res = np.ascontiguousarray(results).reshape(-1)
        assert res.dtype == ca.RESULT_DT
        recs = np.ascontiguousarray(rig_poses, ca.RIG_POSE_DT).reshape(-1)
        assert len(recs) == len(res) * rigs.n_rigs
        out = np.zeros(len(recs), ca.RIG_POSE_DT)
        usable = C.c_int32()
        st = self.T.ctag_testkit_intrinsics_fit_poses(self.h, res.ctypes.data, len(res), recs.ctypes.data, model.m, rigs.r, C.byref(camera), out.ctypes.data,
                                                      C.byref(usable))
        if st != 0:
            raise CtagError(st, "ctag_testkit_intrinsics_fit_poses")
        return out, bool(usable.value)

    def dense_edge_probe(self, gray, segments, K, dist, rvec, tvec, samples_per_edge=8, search_px=3.0, min_contrast=8.0):
        """Edge search of the dense pose-refinement study on the device (ctag_testkit_dense_edge_probe): segments [n, 12]
        (a, b, opposite a, opposite b) -> dict of point [m, 2], normal [m, 2], offset [m] (NaN when dropped), keep [m] bool."""
        gray = np.asarray(gray, np.uint8)
        assert gray.ndim == 2 and gray.strides[1] == 1
        seg = np.ascontiguousarray(segments, np.float64).reshape(-1, 12)
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).ravel())
        d = np.zeros(14)
        dd = np.asarray(dist, np.float64).ravel()
        d[:dd.size] = dd
        rv, tv = np.ascontiguousarray(rvec, np.float64), np.ascontiguousarray(tvec, np.float64)
        m = seg.shape[0] * int(samples_per_edge)
        out = np.zeros((m, 5), np.float64)
        keep = np.zeros(m, np.int32)
        st = self.T.ctag_testkit_dense_edge_probe(self.h, gray.ctypes.data, gray.shape[0], gray.shape[1], gray.strides[0], seg.ctypes.data,
                                                  seg.shape[0], Kd.ctypes.data, d.ctypes.data, rv.ctypes.data, tv.ctypes.data,
                                                  int(samples_per_edge), float(search_px), float(min_contrast), out.ctypes.data,
                                                  keep.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_testkit_dense_edge_probe")
        return {"point": out[:, :2], "normal": out[:, 2:4], "offset": out[:, 4], "keep": keep.astype(bool)}

    def math(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float64)
        out = np.zeros_like(a)
        st = self.T.ctag_math_probe(self.h, op, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_math_probe")
        return out

    def wave(self, op, active, a=None, ia=None, block_threads=64):
        """One primitive of ctag_wave.h by itself (ctag_testkit_wave_probe): active uint64 [n_waves], a float64 / ia int64 [n_waves, 64] (zeros when
        left out) -> (out float64, iout int64), both [n_waves, 64]; a lane that was off keeps WAVE_SENTINEL_*.  Raises CtagError where the mask breaks
        the primitive's contract."""
        active = np.ascontiguousarray(active, np.uint64).reshape(-1)
        n = active.size
        a = np.ascontiguousarray(a if a is not None else np.zeros((n, 64)), np.float64).reshape(n, 64)
        ia = np.ascontiguousarray(ia if ia is not None else np.zeros((n, 64), np.int64), np.int64).reshape(n, 64)
        out, iout = np.zeros((n, 64), np.float64), np.zeros((n, 64), np.int64)
        st = self.T.ctag_testkit_wave_probe(self.h, int(op), int(block_threads), n, active.ctypes.data, a.ctypes.data, ia.ctypes.data, out.ctypes.data,
                                            iout.ctypes.data)
        if st != 0:
            raise CtagError(st, "ctag_testkit_wave_probe")
        return out, iout
