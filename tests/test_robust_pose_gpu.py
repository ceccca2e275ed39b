"""GPU tests of the robust refit (k_pose_robust.hip through the ctag_*_pose_robust_* entry points of include/ctag_pose.h): every record of
every case of tests/robust_shapes.py under every one of its option sets against the independent statement of tests/robust_statement.py
-- statuses, integer fields and inlier masks equal, evaluated fields within 16 x EVAL, final poses within 16 x max(LOOP, STOP), the
fields of a final pose against the statement's evaluation at that very pose -- and the mechanics of the calls: grid stride, capacity,
guard records, determinism, the one-frame calls, the Python wrappers, apply_robust into the covariance call, the C++ method, the
argument checks, log64 on the device.

The iteration count is held equal where max_iterations ends the loop (0, 1, 2) and where the loop runs into the cap of 50; a loop
that ends by PoseBA's own rules ends in steps whose acceptance the rounding of the cost decides (tests/test_robust_statement_cpu.py
measures it on the statement alone), and is held to its final pose."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_statement as cs
import cylindertag_amd as ca
import robust_shapes as shp
import robust_statement as rb
import testkit as tk
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, read_bmp_gray
from pose_testlib import read_camera_yml, read_model_file

pytestmark = pytest.mark.gpu

SZ = ca.ROBUST_POSE_DT.itemsize
SRC_DT = {"marker": ca.POSE_DT, "rig": ca.RIG_POSE_DT, "mv": ca.MV_POSE_DT}


@pytest.fixture(scope="module")
def env():
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    e = {"det": det, "cases": {c["name"]: c for c in shp.all_cases()}, "worst": [0.0, 0.0]}
    yield e
    print("device against the float64 statement: worst evaluated deviation %.2e (bar %.2e), worst pose distance %.2e (bar %.2e)"
          % (e["worst"][0], rb.EVAL_BAR, e["worst"][1], rb.POSE_BAR))
    det.close()


def _model(m):
    return ca.Model(ids=m["ids"], corners=m["corners"], model_size=m["size"])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _opts(o):
    return None if o is None else ca.robust_opts(o["loss"], o["max_iterations"], o["scale_px"], o["auto_k"], o["min_scale_px"])


def _padded_sources(case):
    """rig / mv calls take n_frames * n_rigs source records: the case's, padded with records without a pose."""
    n_frames = case["recs"].shape[-1]
    src = np.ascontiguousarray(case["sources"], SRC_DT[case["kind"]])
    n_rigs = -(-len(src) // n_frames)
    pad = np.zeros(n_frames * n_rigs - len(src), src.dtype)
    pad["status"] = 5
    return np.concatenate([src, pad]), n_rigs


def _run(env, case, opts, sources=None, capacity=None, guard=3):
    """One batch call on device copies of the case; returns the robust records (and checks the guard records on both sides)."""
    import torch
    det, kind = env["det"], case["kind"]
    M = _model(case["model"])
    o = _opts(opts)
    if kind == "marker":
        src = np.ascontiguousarray(case["sources"] if sources is None else sources, ca.POSE_DT)
        n_frames, n_rigs = len(case["recs"]), None
    else:
        src, n_rigs = _padded_sources(case)
        n_frames = case["recs"].shape[-1]
    n_out = len(src) if capacity is None else min(capacity, len(src))
    out = torch.full(((len(src) + 2 * guard) * SZ,), 0xA5, dtype=torch.uint8, device="cuda")
    d_src = _dev(src)
    cam = ca.make_camera(*case["cameras"][0])
    if kind == "marker":
        d_recs = _dev(case["recs"])
        offsets = np.zeros(n_frames + 1, np.int32)
        offsets[n_frames] = len(src)
        d_off = _dev(offsets)
        det.robust_pose_batch_device(d_recs.data_ptr(), n_frames, M, cam, d_off.data_ptr(), d_src.data_ptr(), len(src) if capacity is None else capacity,
                                     out.data_ptr() + guard * SZ, o)
    elif kind == "rig":
        d_recs = _dev(case["recs"])
        rigs = ca.Rigs(M, case["rig_of_model"], n_rigs)
        det.robust_rig_pose_batch_device(d_recs.data_ptr(), n_frames, M, rigs, cam, d_src.data_ptr(), out.data_ptr() + guard * SZ, o)
    else:
        d_recs = [_dev(case["recs"][c]) for c in range(len(case["cameras"]))]
        rigs = ca.Rigs(M, case["rig_of_model"], n_rigs)
        cams = ca.CameraSet([ca.make_camera(K, d) for K, d in case["cameras"]], case["camera_poses"])
        det.robust_mv_rig_pose_batch_device([t.data_ptr() for t in d_recs], n_frames, M, rigs, cams, d_src.data_ptr(), out.data_ptr() + guard * SZ, o)
    det.sync()
    raw = out.cpu().numpy()
    assert (raw[:guard * SZ] == 0xA5).all() and (raw[(guard + n_out) * SZ:] == 0xA5).all(), "bytes written outside the records"
    return raw[guard * SZ:(guard + n_out) * SZ].copy().view(ca.ROBUST_POSE_DT)


def _check(env, case, only=None):
    n = len(case["sources"])
    for name, o in shp.runs_of(case):
        if only is not None and name not in only:
            continue
        got = _run(env, case, o)
        assert (got["status"][n:] == rb.ROBUST_NO_POSE).all() and not got[n:].tobytes().strip(b"\x01\x00")  # the padding records
        want = shp.expected_of(case, o)
        if "expect" in case:
            assert [e["status"] for e in want] == case["expect"]
        we, wp = rb.check_robust_records(got[:n], want, case["sources"], shp.pparts_of(case), what="%s under %s" % (case["name"], name))
        moved = [int(G["iterations"]) for G, E in zip(got[:n], want) if E["status"] == 0]
        same = sum(int(G["iterations"]) == E["iterations"] for G, E in zip(got[:n], want) if E["status"] == 0)
        print("%s under %s: %d records, evaluated fields %.2e, poses %.2e, iterations %s (%d as the statement's)" % (case["name"], name, n, we, wp, moved[:12], same))
        env["worst"][0], env["worst"][1] = max(env["worst"][0], we), max(env["worst"][1], wp)


EVAL_RUNS = tuple(k for k, o in shp.OPTION_SETS.items() if o["max_iterations"] == 0) + ("edge inside", "edge outside")


@pytest.mark.parametrize("name", [c["name"] for c in shp.all_cases()])
def test_forms_without_the_loop(env, name):
    """max_iterations = 0 on every shape: the walk, the cached points, the median and the sums, without the loop behind them."""
    _check(env, env["cases"][name], EVAL_RUNS)


@pytest.mark.parametrize("name", [c["name"] for c in shp.all_cases() if "expect" not in c and c["name"] != "threshold edge"])
def test_records_against_the_statement(env, name):
    """Every other option set of the shape: both losses, given and automatic scales, max_iterations 1, 2 and 50."""
    _check(env, env["cases"][name], [k for k in env["cases"][name]["runs"] if k not in EVAL_RUNS])


@pytest.mark.parametrize("name", ["nan pixel", "rules", "rig rules", "mv rules"])
def test_rules(env, name):
    """CTAG_ROBUST_NO_POSE for every source status but OK, CTAG_ROBUST_BAD_RECORD for each of its causes (records that point outside
    their arrays are rejected, never read), CTAG_ROBUST_DEGENERATE for a NaN pixel; all other fields 0."""
    _check(env, env["cases"][name])


def test_weight_one_identity(env):
    """Huber with scale_px = 1e9: every weight is exactly 1, cost0 == cost_ls0 and cost == cost_ls bit for bit, every point an inlier."""
    case = env["cases"]["marker size 20 golden"]
    for name in ("weight one", "weight one eval"):
        G = _run(env, case, shp.OPTION_SETS[name])
        assert (G["status"] == 0).all() and (G["n_inliers"] == G["n_points"]).all()
        assert G["cost0"].tobytes() == G["cost_ls0"].tobytes() and G["cost"].tobytes() == G["cost_ls"].tobytes()
        assert (G["scale_px"] == 1e9).all() and (G["sigma_hat"] > 0).all()


def _scene(env):
    det = env["det"]
    M, cam = ca.Model(os.path.join(GOLDEN, "CTag_2f12c.model")), ca.load_camera(os.path.join(GOLDEN, "cameraParams.yml"))
    res = det.detect(read_bmp_gray(os.path.join(GOLDEN, "test.bmp")), 5, True, 5)
    return res, det.estimate_pose(res, M, cam), M, cam


def test_reference_scene_weight_one_stays_at_the_least_squares_pose(env):
    """test.bmp: detect, estimate_pose, robust_pose with scale_px = 1e9 -- real pose records, which ARE PoseBA's minimum, as the
    source: the refit's final pose lies within the pose bar of the source pose, its cost0 is the pose kernel's cost."""
    det = env["det"]
    res, poses, M, cam = _scene(env)
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    model = read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model"))
    case = {"kind": "marker", "name": "test.bmp", "recs": np.array([res]), "model": model, "cameras": [(K, dist)], "camera_poses": [shp.sh.ZERO_POSE],
            "sources": poses}
    got = det.robust_pose(res, poses, M, cam, _opts(shp.OPTION_SETS["weight one"]))
    assert (poses["status"] == 0).sum() >= 4
    worst = 0.0
    for w, (G, P) in enumerate(zip(got, poses)):
        assert int(G["status"]) == (rb.ROBUST_OK if P["status"] == 0 else rb.ROBUST_NO_POSE)
        if P["status"] != 0:
            continue
        assert abs(G["cost0"] - P["cost"]) <= 1e-9 * max(1.0, P["cost"]) and G["cost"] <= G["cost0"] and G["n_points"] == P["n_points"]
        x = np.concatenate([P["rvec"], P["tvec"]])
        H = rb.hessian_at(shp.pparts_of(case, np.longdouble)(w), x, np.longdouble(1e9), rb.HUBER)
        d = rb.pose_distance(np.concatenate([G["rvec"], G["tvec"]]), x, H)
        worst = max(worst, d)
        assert d <= rb.POSE_BAR, (w, d)
    print("test.bmp, weight one: the refit stays within %.2e pose sigmas of the pose kernel's pose (bar %.2e)" % (worst, rb.POSE_BAR))
    # the default refit against the statement, from the same real records
    o = rb.default_opts()
    got = det.robust_pose(res, poses, M, cam)
    assert got.tobytes() == _run(env, case, o).tobytes() == _run(env, case, None).tobytes()  # NULL opts: the defaults
    rb.check_robust_records(got, rb.expected_of(case, o), poses, shp.pparts_of(case), what="test.bmp")


def test_grid_stride_capacity_and_determinism(env):
    """More records than twice the launch grid in one call, tiled from the distinct records in a fixed permutation: every record has
    the bytes of its distinct source's record in a small call (the same record at many places of two batches).  capacity below the
    record count: the records past it are not written.  A second run and a smaller call after the larger one give the same bytes."""
    case = env["cases"]["marker size 20 golden"]
    distinct = np.ascontiguousarray(case["sources"], ca.POSE_DT).copy()
    bent = distinct[:4].copy()
    bent["status"][0], bent["frame"][1], bent["marker"][2], bent["n_points"][3] = 3, len(case["recs"]), 7, 9
    distinct = np.concatenate([distinct, bent])
    opts = shp.OPTION_SETS["cauchy auto"]
    small = _run(env, case, opts, sources=distinct)
    assert list(small["status"][-4:]) == [rb.ROBUST_NO_POSE, rb.ROBUST_BAD_RECORD, rb.ROBUST_BAD_RECORD, rb.ROBUST_BAD_RECORD] and (small["status"][:-4] == 0).all()
    n = 2 * shp.GRID + 37
    pick = np.concatenate([np.arange(len(distinct)), np.random.default_rng(5).integers(0, len(distinct), n - len(distinct))])
    big = _run(env, case, opts, sources=distinct[pick])
    assert len(big) == n and big.tobytes() == small[pick].tobytes()
    assert _run(env, case, opts, sources=distinct[pick]).tobytes() == big.tobytes()          # a second run
    assert _run(env, case, opts, sources=distinct).tobytes() == small.tobytes()              # a smaller call after the larger one
    cut = _run(env, case, opts, sources=distinct[pick], capacity=n - 5)                      # _run checks that the last 5 stay untouched
    assert len(cut) == n - 5 and cut.tobytes() == big[:n - 5].tobytes()
    assert len(_run(env, case, opts, sources=distinct, capacity=0)) == 0


def test_one_frame_calls_and_wrappers_give_the_batch_bytes(env):
    det = env["det"]
    opts = shp.OPTION_SETS["huber auto"]
    o = _opts(opts)
    case = env["cases"]["marker size 20 golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    batch = _run(env, case, opts)
    assert det.robust_pose(case["recs"][0], case["sources"][:2], M, cam, o).tobytes() == batch[:2].tobytes()
    assert det.robust_pose(case["recs"][0], case["sources"][:2], M, cam).tobytes() == _run(env, case, None)[:2].tobytes()
    assert _run(env, case, None).tobytes() == _run(env, case, rb.default_opts()).tobytes()
    case = env["cases"]["rig golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    rigs = ca.Rigs(M, case["rig_of_model"], 1)
    assert det.robust_rig_pose(case["recs"][0], case["sources"][:1], M, rigs, cam, o).tobytes() == _run(env, case, opts)[:1].tobytes()
    case = env["cases"]["mv three own cameras"]
    M = _model(case["model"])
    rigs = ca.Rigs(M, case["rig_of_model"], case["n_rigs"])
    cams = ca.CameraSet([ca.make_camera(K, d) for K, d in case["cameras"]], case["camera_poses"])
    got = det.robust_mv_rig_pose(case["recs"][:, 0], case["sources"][:case["n_rigs"]], M, rigs, cams, o)
    assert got.tobytes() == _run(env, case, opts)[:case["n_rigs"]].tobytes()


def test_apply_robust_feeds_the_covariance(env):
    """apply_robust puts the refitted poses into copies of the pose records; pose_cov of those is the covariance at the refitted pose:
    its recomputed cost is the refit's cost_ls, its worst point the refit's."""
    det = env["det"]
    case = env["cases"]["marker size 20 golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    w = case["outlier"][0]
    f = int(case["sources"][w]["frame"])
    src = np.ascontiguousarray(case["sources"][w:w + 2], ca.POSE_DT).copy()
    src["frame"] = 0
    src["status"][1] = 3
    R = det.robust_pose(case["recs"][f], src, M, cam)
    assert list(R["status"]) == [rb.ROBUST_OK, rb.ROBUST_NO_POSE]
    moved = ca.apply_robust(src, R)
    assert moved["rvec"][0].tobytes() == R["rvec"][0].tobytes() and moved["tvec"][0].tobytes() == R["tvec"][0].tobytes()
    assert moved[1].tobytes() == src[1].tobytes() and src["rvec"][0].tobytes() != R["rvec"][0].tobytes()
    for k in src.dtype.names:
        if k not in ("rvec", "tvec"):
            assert moved[k].tobytes() == src[k].tobytes()
    cov = det.pose_cov(case["recs"][f], moved, M, cam)
    assert cov["status"][0] == cs.COV_OK and cov["worst_point"][0] == R["worst_point"][0] == case["outlier"][1]
    assert abs(cov["cost"][0] - R["cost_ls"][0]) <= rb.EVAL_BAR * R["cost_ls"][0]
    assert abs(cov["max_residual_px"][0] - R["max_residual_px"][0]) <= rb.EVAL_BAR * R["max_residual_px"][0]
    with pytest.raises(ValueError):
        ca.apply_robust(src, R[:1])


def test_cpp_class_gives_the_c_abi_records(env):
    """CylinderTag::estimatePoseRobust on test.bmp (examples/ctag_classcheck.cpp, mode robust, doubles printed as hexadecimal floats):
    the fields of ctag_estimate_pose_robust's records for the markers that have a model, in estimatePose's order."""
    import subprocess
    from ctag_testlib import ROOT
    det = env["det"]
    exe = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_classcheck")
    files = [os.path.join(GOLDEN, f) for f in ("CTag_2f12c.marker", "test.bmp", "CTag_2f12c.model", "cameraParams.yml")]
    res, poses, M, cam = _scene(env)
    keep = poses["status"] != capi.POSE_NO_MODEL
    for cauchy, scale, cap in ((1, 0.0, 50), (0, 0.4, 3)):
        out = subprocess.run([exe, "robust"] + files + [str(cauchy), repr(scale), str(cap)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        want = det.robust_pose(res, poses, M, cam, ca.robust_opts(capi.LOSS_CAUCHY if cauchy else capi.LOSS_HUBER, cap, scale))[keep]
        lines = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("robust ")]
        assert len(lines) == len(want) >= 4
        for ln, W, P in zip(lines, want, poses[keep]):
            assert [int(v) for v in ln[:7]] == [int(P["model_index"])] + [int(W[k]) for k in ("status", "n_points", "n_inliers", "iterations", "loss", "worst_point")]
            got = np.array([float.fromhex(v) for v in ln[7:20]])
            ref = np.concatenate([[W[k] for k in ("scale_px", "sigma_hat", "cost_ls0", "cost_ls", "cost0", "cost", "max_residual_px")], W["rvec"], W["tvec"]])
            assert got.tobytes() == ref.tobytes()
            assert ln[20] == "".join(str(int(W["inlier_mask"][i >> 5]) >> (i & 31) & 1) for i in range(int(W["n_points"])))


def test_argument_rejections(env):
    import torch
    det, L = env["det"], capi.load_library()
    case = env["cases"]["marker size 20 golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + (1 << 15)  # zero records in, robust records out
    good = ca.robust_opts()
    assert (good.struct_size, good.loss, good.max_iterations, good.reserved, good.scale_px, good.auto_k, good.min_scale_px) == (C.sizeof(capi.RobustOptsC), 1, 50, 0, 0.0, 2.5, 0.05)

    def marker(h=det.h, res=p, n=1, m=M.m, c=C.byref(cam), off=p, poses=p, cap=1, o=None, out=q):
        return L.ctag_pose_robust_batch_device(h, res, n, m, c, off, poses, cap, o, out)
    assert marker() == 0
    for kw in ({"h": None}, {"res": None}, {"n": -1}, {"m": None}, {"off": None}, {"poses": None}, {"cap": -1}, {"out": None}):
        assert marker(**kw) == capi.ERR_ARG, kw
    bad_cam = ca.make_camera(case["cameras"][0][0], np.zeros(3, np.float32))
    assert marker(c=C.byref(bad_cam)) == capi.ERR_UNSUPPORTED and marker(c=None) == capi.ERR_UNSUPPORTED
    for field, value in (("struct_size", 32), ("loss", 2), ("loss", -1), ("max_iterations", -1), ("max_iterations", 51), ("scale_px", float("nan")),
                         ("scale_px", float("inf")), ("auto_k", float("nan")), ("min_scale_px", float("-inf")), ("auto_k", 0.0), ("auto_k", -1.0),
                         ("min_scale_px", 0.0)):
        o = ca.robust_opts()
        setattr(o, field, value)
        assert marker(o=C.byref(o)) == capi.ERR_ARG, (field, value)
        assert not rb.opts_ok(dict(rb.default_opts(), **{field: value})) or field == "struct_size"
    o = ca.robust_opts(scale_px=1.0, auto_k=0.0, min_scale_px=-1.0)  # a given scale: the automatic one's parameters are not judged
    assert marker(o=C.byref(o)) == 0
    rig = env["cases"]["rig golden"]
    MR = _model(rig["model"])
    rigs, other = ca.Rigs(MR, rig["rig_of_model"], 1), ca.Rigs(M, np.zeros(3, np.int32), 1)
    assert L.ctag_rig_pose_robust_batch_device(det.h, p, 1, MR.m, rigs.r, C.byref(cam), p, None, q) == 0
    assert L.ctag_rig_pose_robust_batch_device(det.h, p, 1, MR.m, other.r, C.byref(cam), p, None, q) == capi.ERR_ARG  # another model's rig set
    assert L.ctag_rig_pose_robust_batch_device(det.h, p, 1, MR.m, rigs.r, C.byref(cam), None, None, q) == capi.ERR_ARG
    assert L.ctag_rig_pose_robust_batch_device(det.h, p, 1, MR.m, rigs.r, C.byref(bad_cam), p, None, q) == capi.ERR_UNSUPPORTED
    cams = ca.CameraSet([cam, cam], [shp.sh.ZERO_POSE, shp.sh.ZERO_POSE])
    ptrs = (C.c_void_p * 2)(p, None)
    assert L.ctag_mv_rig_pose_robust_batch_device(det.h, ptrs, 1, MR.m, rigs.r, cams.s, p, None, q) == capi.ERR_ARG   # a camera without records
    ptrs = (C.c_void_p * 2)(p, p)
    assert L.ctag_mv_rig_pose_robust_batch_device(det.h, ptrs, 1, MR.m, rigs.r, cams.s, p, None, q) == 0
    assert L.ctag_mv_rig_pose_robust_batch_device(det.h, ptrs, 1, MR.m, rigs.r, None, p, None, q) == capi.ERR_ARG
    det.sync()


def test_log64_on_the_device(env):
    """ctm::log64 through the math probe: below 1 ulp from the true logarithm, and the bits of numpy's log wherever that is the
    correctly rounded value and log64 is too (more than nine in ten arguments)."""
    x = shp.log64_points()
    got = env["det"].math(tk.MATH_LOG64, x, np.zeros_like(x))
    worst = shp.log64_ulps(x, got)
    same = float((got == np.log(x)).mean())
    print("log64 on the device: worst %.3f ulp over %d arguments, %.1f %% the bits of the host's log" % (worst, len(x), 100 * same))
    assert worst < 1.0 and same > 0.9 and got[list(x).index(1.0)] == 0.0
