"""GPU tests of the pose covariance (k_pose_cov.hip through the ctag_*_pose_cov_* entry points of include/ctag_pose.h): every
record of every case of tests/cov_shapes.py against the independent statement of tests/cov_statement.py -- statuses and integer
fields exact, cost against the source record's, the other doubles within the statement's measured bar, cov symmetric bit for bit --
and the mechanics of the calls: grid stride, capacity, guard records, determinism, the one-frame calls, the argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_shapes as sh
import cov_statement as cs
import cylindertag_amd as ca
import testkit as tk
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, read_bmp_gray
from pose_testlib import read_camera_yml, read_model_file

pytestmark = pytest.mark.gpu

SZ = ca.POSE_COV_DT.itemsize
SRC_DT = {"marker": ca.POSE_DT, "rig": ca.RIG_POSE_DT, "mv": ca.MV_POSE_DT}
# param, sigma_px, outlier_k
OPTS = [(p, s, k) for p in (cs.TANGENT, cs.RVEC) for s in (0.0, 0.2) for k in (0.0, 3.0)]


@pytest.fixture(scope="module")
def env():
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    e = {"det": det, "cases": {c["name"]: c for c in sh.all_cases()}}
    yield e
    det.close()


def _model(m):
    return ca.Model(ids=m["ids"], corners=m["corners"], model_size=m["size"])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _padded_sources(case):
    """rig / mv calls take n_frames * n_rigs source records: the case's, padded with records without a pose."""
    n_frames = case["recs"].shape[-1]
    src = np.ascontiguousarray(case["sources"], SRC_DT[case["kind"]])
    n_rigs = -(-len(src) // n_frames)
    pad = np.zeros(n_frames * n_rigs - len(src), src.dtype)
    pad["status"] = 5
    return np.concatenate([src, pad]), n_rigs


def _run(env, case, opts, sources=None, capacity=None, guard=3):
    """One batch call on device copies of the case; returns the covariance records (and checks the guard records on both sides)."""
    import torch
    det, kind = env["det"], case["kind"]
    M = _model(case["model"])
    o = ca.cov_opts(*opts) if opts is not None else None
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
        det.pose_cov_batch_device(d_recs.data_ptr(), n_frames, M, cam, d_off.data_ptr(), d_src.data_ptr(), len(src) if capacity is None else capacity,
                                  out.data_ptr() + guard * SZ, o)
    elif kind == "rig":
        d_recs = _dev(case["recs"])
        rigs = ca.Rigs(M, case["rig_of_model"], n_rigs)
        det.rig_pose_cov_batch_device(d_recs.data_ptr(), n_frames, M, rigs, cam, d_src.data_ptr(), out.data_ptr() + guard * SZ, o)
    else:
        d_recs = [_dev(case["recs"][c]) for c in range(len(case["cameras"]))]
        rigs = ca.Rigs(M, case["rig_of_model"], n_rigs)
        cams = ca.CameraSet([ca.make_camera(K, d) for K, d in case["cameras"]], case["camera_poses"])
        det.mv_rig_pose_cov_batch_device([t.data_ptr() for t in d_recs], n_frames, M, rigs, cams, d_src.data_ptr(), out.data_ptr() + guard * SZ, o)
    det.sync()
    raw = out.cpu().numpy()
    assert (raw[:guard * SZ] == 0xA5).all() and (raw[(guard + n_out) * SZ:] == 0xA5).all(), "bytes written outside the records"
    return raw[guard * SZ:(guard + n_out) * SZ].copy().view(ca.POSE_COV_DT)


def _check(env, case, all_opts=OPTS):
    worst = 0.0
    n = len(case["sources"])
    for opts in all_opts:
        got = _run(env, case, opts)
        assert (got["status"][n:] == cs.COV_NO_POSE).all() and not got[n:].tobytes().strip(b"\x01\x00")  # the padding records
        want = sh.expected_of(case, dict(param=opts[0], sigma_px=opts[1], outlier_k=opts[2]))
        if "expect" in case:
            assert [e["status"] for e in want] == case["expect"]
        worst = max(worst, cs.check_cov_records(got[:n], want, case["sources"], what="%s %s" % (case["name"], opts)))
    print("%s: %d records x %d option sets, worst deviation %.2e (bar %.2e)" % (case["name"], n, len(all_opts), worst, cs.BAR))
    return worst


@pytest.mark.parametrize("name", ["marker size 20 golden", "marker size 12 n_dist8", "marker size 16 n_dist12"])
def test_marker_records_against_the_statement(env, name):
    """Per-marker point counts 4 8 60 64 68 96 160, three cameras, both parametrisations, sigma_px 0 and 0.2, outlier_k 0 and 3."""
    case = env["cases"][name]
    _check(env, case)
    if case["outlier"]:
        w, i = case["outlier"]
        for opts in ((cs.TANGENT, 0.2, 3.0), (cs.RVEC, 0.0, 3.0)):
            G = _run(env, case, opts)[w]
            assert G["status"] == 0 and G["worst_point"] == i and G["n_outliers"] >= 1 and G["max_residual_px"] > 4.0
        assert _run(env, case, (cs.TANGENT, 0.2, 0.0))[w]["n_outliers"] == 0


@pytest.mark.parametrize("name", ["rig golden", "rig n_dist12"])
def test_rig_records_against_the_statement(env, name):
    """Rig point counts 164 256 796 800."""
    _check(env, env["cases"][name])


@pytest.mark.parametrize("name", ["mv 8 + 8", "mv three own cameras", "mv eight cameras", "mv virtual split"])
def test_mv_records_against_the_statement(env, name):
    _check(env, env["cases"][name], OPTS[::3] + OPTS[1:2])


def test_virtual_split_gives_the_bytes_of_the_rig_covariance(env):
    """Three equal cameras at the reference that share out a rig record's markers: Rc P + tc is P bit for bit, the sums run over the
    same points in the same order."""
    rig, split = env["cases"]["rig golden"], env["cases"]["mv virtual split"]
    for opts in ((cs.TANGENT, 0.0, 3.0), (cs.RVEC, 0.2, 3.0)):
        a, b = _run(env, rig, opts), _run(env, split, opts)
        assert (a["status"] == 0).all() and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["rules", "rig rules", "mv rules"])
def test_rules(env, name):
    """CTAG_COV_NO_POSE for every source status but OK, CTAG_COV_BAD_RECORD for each of its causes (records that point outside
    their arrays are rejected, never read), CTAG_COV_SINGULAR for four coincident points and for a collinear set; all other fields 0."""
    case = env["cases"][name]
    _check(env, case, [(cs.TANGENT, 0.0, 3.0), (cs.RVEC, 0.2, 3.0)])


def test_grid_stride_capacity_and_determinism(env):
    """More records than twice the launch grid in one call, tiled from the distinct records in a fixed permutation: every record has
    the bytes of its distinct source's record in a small call.  capacity below the record count: the records past it are not
    written.  A second run and a smaller call after the larger one give the same bytes."""
    case = env["cases"]["marker size 20 golden"]
    distinct = np.ascontiguousarray(case["sources"], ca.POSE_DT).copy()
    bent = distinct[:4].copy()
    bent["status"][0], bent["frame"][1], bent["marker"][2], bent["n_points"][3] = 3, len(case["recs"]), 7, 9
    distinct = np.concatenate([distinct, bent])
    opts = (cs.TANGENT, 0.0, 3.0)
    small = _run(env, case, opts, sources=distinct)
    assert list(small["status"][-4:]) == [cs.COV_NO_POSE, cs.COV_BAD_RECORD, cs.COV_BAD_RECORD, cs.COV_BAD_RECORD] and (small["status"][:-4] == 0).all()
    n = 2 * sh.GRID + 37
    pick = np.concatenate([np.arange(len(distinct)), np.random.default_rng(5).integers(0, len(distinct), n - len(distinct))])
    big = _run(env, case, opts, sources=distinct[pick])
    assert len(big) == n and big.tobytes() == small[pick].tobytes()
    assert _run(env, case, opts, sources=distinct[pick]).tobytes() == big.tobytes()          # a second run
    assert _run(env, case, opts, sources=distinct).tobytes() == small.tobytes()              # a smaller call after the larger one
    cut = _run(env, case, opts, sources=distinct[pick], capacity=n - 5)                      # _run checks that the last 5 stay untouched
    assert len(cut) == n - 5 and cut.tobytes() == big[:n - 5].tobytes()
    assert len(_run(env, case, opts, sources=distinct, capacity=0)) == 0


def test_one_frame_calls_give_the_batch_bytes(env):
    det = env["det"]
    opts = (cs.RVEC, 0.2, 3.0)
    o = ca.cov_opts(*opts)
    case = env["cases"]["marker size 20 golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    batch = _run(env, case, opts)
    got = det.pose_cov(case["recs"][0], case["sources"][:2], M, cam, o)
    assert got.tobytes() == batch[:2].tobytes()
    assert det.pose_cov(case["recs"][0], case["sources"][:2], M, cam).tobytes() == _run(env, case, None)[:2].tobytes()  # NULL opts: the defaults
    assert _run(env, case, None).tobytes() == _run(env, case, (cs.TANGENT, 0.0, 3.0)).tobytes()
    case = env["cases"]["rig golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    rigs = ca.Rigs(M, case["rig_of_model"], 1)
    assert det.rig_pose_cov(case["recs"][0], case["sources"][:1], M, rigs, cam, o).tobytes() == _run(env, case, opts)[:1].tobytes()
    case = env["cases"]["mv three own cameras"]
    M = _model(case["model"])
    rigs = ca.Rigs(M, case["rig_of_model"], case["n_rigs"])
    cams = ca.CameraSet([ca.make_camera(K, d) for K, d in case["cameras"]], case["camera_poses"])
    got = det.mv_rig_pose_cov(case["recs"][:, 0], case["sources"][:case["n_rigs"]], M, rigs, cams, o)
    assert got.tobytes() == _run(env, case, opts)[:case["n_rigs"]].tobytes()


def test_argument_rejections(env):
    import torch
    det, L = env["det"], capi.load_library()
    case = env["cases"]["marker size 20 golden"]
    M, cam = _model(case["model"]), ca.make_camera(*case["cameras"][0])
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + (1 << 15)  # zero records in, covariance records out
    good = ca.cov_opts()
    assert (good.struct_size, good.param, good.sigma_px, good.outlier_k) == (C.sizeof(capi.CovOptsC), 0, 0.0, 3.0)

    def marker(h=det.h, res=p, n=1, m=M.m, c=C.byref(cam), off=p, poses=p, cap=1, o=None, out=q):
        return L.ctag_pose_cov_batch_device(h, res, n, m, c, off, poses, cap, o, out)
    assert marker() == 0
    for kw in ({"h": None}, {"res": None}, {"n": -1}, {"m": None}, {"off": None}, {"poses": None}, {"cap": -1}, {"out": None}):
        assert marker(**kw) == capi.ERR_ARG, kw
    bad_cam = ca.make_camera(case["cameras"][0][0], np.zeros(3, np.float32))
    assert marker(c=C.byref(bad_cam)) == capi.ERR_UNSUPPORTED and marker(c=None) == capi.ERR_UNSUPPORTED
    for field, value in (("struct_size", 16), ("param", 2), ("param", -1), ("sigma_px", float("nan")), ("sigma_px", float("inf")),
                         ("outlier_k", float("nan")), ("outlier_k", float("-inf"))):
        o = ca.cov_opts()
        setattr(o, field, value)
        assert marker(o=C.byref(o)) == capi.ERR_ARG, field
    rig = env["cases"]["rig golden"]
    MR = _model(rig["model"])
    rigs, other = ca.Rigs(MR, rig["rig_of_model"], 1), ca.Rigs(M, np.zeros(3, np.int32), 1)
    assert L.ctag_rig_pose_cov_batch_device(det.h, p, 1, MR.m, rigs.r, C.byref(cam), p, None, q) == 0
    assert L.ctag_rig_pose_cov_batch_device(det.h, p, 1, MR.m, other.r, C.byref(cam), p, None, q) == capi.ERR_ARG  # another model's rig set
    assert L.ctag_rig_pose_cov_batch_device(det.h, p, 1, MR.m, rigs.r, C.byref(cam), None, None, q) == capi.ERR_ARG
    assert L.ctag_rig_pose_cov_batch_device(det.h, p, 1, MR.m, rigs.r, C.byref(bad_cam), p, None, q) == capi.ERR_UNSUPPORTED
    cams = ca.CameraSet([cam, cam], [sh.ZERO_POSE, sh.ZERO_POSE])
    ptrs = (C.c_void_p * 2)(p, None)
    assert L.ctag_mv_rig_pose_cov_batch_device(det.h, ptrs, 1, MR.m, rigs.r, cams.s, p, None, q) == capi.ERR_ARG   # a camera without records
    ptrs = (C.c_void_p * 2)(p, p)
    assert L.ctag_mv_rig_pose_cov_batch_device(det.h, ptrs, 1, MR.m, rigs.r, cams.s, p, None, q) == 0
    assert L.ctag_mv_rig_pose_cov_batch_device(det.h, ptrs, 1, MR.m, rigs.r, None, p, None, q) == capi.ERR_ARG
    det.sync()


def test_reference_scene_through_the_wrappers(env):
    """test.bmp: detect, estimate_pose, pose_cov -- real pose records as the source.  The records equal the C ABI's batch call and
    the statement; the recomputed cost is the pose kernel's."""
    det = env["det"]
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    model = read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model"))
    M, cam = ca.Model(os.path.join(GOLDEN, "CTag_2f12c.model")), ca.load_camera(os.path.join(GOLDEN, "cameraParams.yml"))
    res = det.detect(read_bmp_gray(os.path.join(GOLDEN, "test.bmp")), 5, True, 5)
    poses = det.estimate_pose(res, M, cam)
    assert (poses["status"] == 0).sum() >= 4
    case = {"kind": "marker", "name": "test.bmp", "recs": np.array([res]), "model": model, "cameras": [(K, dist)], "camera_poses": [sh.ZERO_POSE],
            "sources": poses}
    for opts in ((cs.TANGENT, 0.0, 3.0), (cs.RVEC, 0.3, 3.0)):
        got = det.pose_cov(res, poses, M, cam, ca.cov_opts(*opts))
        assert got.tobytes() == _run(env, case, opts).tobytes()
        want = sh.expected_of(case, dict(param=opts[0], sigma_px=opts[1], outlier_k=opts[2]))
        assert [e["status"] for e in want] == [cs.COV_OK if s == 0 else cs.COV_NO_POSE for s in poses["status"]]
        cs.check_cov_records(got, want, poses, what="test.bmp")


def test_cpp_class_gives_the_c_abi_records(env):
    """CylinderTag::estimatePoseCovariance on test.bmp (examples/ctag_classcheck.cpp, mode cov, doubles printed as hexadecimal
    floats): the fields of ctag_estimate_pose_cov's records for the markers that have a model, in estimatePose's order."""
    import subprocess
    from ctag_testlib import ROOT
    det = env["det"]
    exe = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_classcheck")
    files = [os.path.join(GOLDEN, f) for f in ("CTag_2f12c.marker", "test.bmp", "CTag_2f12c.model", "cameraParams.yml")]
    M, cam = ca.Model(files[2]), ca.load_camera(files[3])
    res = det.detect(read_bmp_gray(files[1]), 5, True, 5)
    poses = det.estimate_pose(res, M, cam)
    keep = poses["status"] != capi.POSE_NO_MODEL
    for tangent, sigma in ((1, 0.0), (0, 0.25)):
        out = subprocess.run([exe, "cov"] + files + [str(tangent), repr(sigma)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        want = det.pose_cov(res, poses, M, cam, ca.cov_opts(cs.TANGENT if tangent else cs.RVEC, sigma, 3.0))[keep]
        lines = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("cov ")]
        assert len(lines) == len(want) >= 4
        for ln, W, P in zip(lines, want, poses[keep]):
            assert [int(v) for v in ln[:6]] == [int(P["model_index"])] + [int(W[k]) for k in ("status", "n_points", "dof", "worst_point", "n_outliers")]
            got = np.array([float.fromhex(v) for v in ln[6:]])
            ref = np.concatenate([[W[k] for k in ("cost", "sigma2_hat", "sigma2_used", "max_residual_px", "min_pivot")], W["cov"].ravel()])
            assert got.tobytes() == ref.tobytes()
