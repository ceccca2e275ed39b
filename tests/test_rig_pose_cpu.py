"""CPU tests of the rig pose (include/ctag_pose.h: one pose per rig of markers): the record layout against the C header, the
rig composition of tests/rig_testlib.py against planted poses and scipy, the accuracy gain over per-marker poses, and the host
side of the C ABI (argument checks, no CPU fallback)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cylindertag_amd as ca
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, ROOT
from pose_testlib import PoseOracle, make_camera, make_model_view, project, read_camera_yml, read_model_file, rodrigues
from rig_testlib import RIG_POSE_DT, compose_rig_poses, rig_study, rot_err_deg, stacked_rig_model, synth_rig_frame

MODEL_PATH = os.path.join(GOLDEN, "CTag_2f12c.model")
CAM_PATH = os.path.join(GOLDEN, "cameraParams.yml")


@pytest.fixture(scope="module")
def env():
    K, dist = read_camera_yml(CAM_PATH)
    rig = stacked_rig_model(read_model_file(MODEL_PATH), 3, 70.0)
    return {"K": K, "dist": dist, "rig": rig, "po": PoseOracle(), "cam": make_camera(K, dist), "mv": make_model_view(rig)}


def test_rig_record_layout_matches_header():
    fields = ["status", "rig", "frame", "n_members", "n_excluded", "n_points", "iterations", "reserved", "member_mask", "rvec", "tvec",
              "rvec0", "tvec0", "cost0", "cost"]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ctag_pose.h\"\nint main(){printf(\"%zu %d %d\", sizeof(ctag_rig_pose_rec), " \
          "CTAG_POSE_NOT_SEEN, CTAG_RIG_MAX_POINTS);" + "".join(' printf(" %%zu", offsetof(ctag_rig_pose_rec, %s));' % f for f in fields) + "}"
    exe = os.path.join(ROOT, "cylindertag_amd", "_build", "rig_layout")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[:3] == [160, capi.POSE_NOT_SEEN, capi.RIG_MAX_POINTS] == [160, 5, 800]
    assert got[3:] == [ca.RIG_POSE_DT.fields[f][1] for f in fields]
    assert ca.RIG_POSE_DT == RIG_POSE_DT and ca.RIG_POSE_DT.itemsize == 160
    assert {"ctag_rigs_create", "ctag_rigs_free", "ctag_rig_pose_batch_device", "ctag_estimate_rig_pose"} <= set(capi.POSE_EXPORTS)


def test_rig_composition_recovers_planted_poses_and_is_a_scipy_minimum(env):
    """Noise-free frames: the planted rig pose comes back.  Noisy frames: the composition's final pose is the minimum of the
    reprojection residual over the concatenated undistorted points as scipy.optimize.least_squares sees it."""
    from scipy.optimize import least_squares
    K, dist, rig, po, cam, mv = env["K"], env["dist"], env["rig"], env["po"], env["cam"], env["mv"]
    rng = np.random.default_rng(3)
    K64 = K.astype(np.float64)
    d = np.zeros(5)
    d[:dist.size] = dist[:5]
    for f in range(12):
        noise = 0.0 if f < 6 else 0.3
        res, truth = synth_rig_frame(rng, rig, [[0, 1, 2]], K, dist, noise)
        R = compose_rig_poses(po, res, mv, cam, np.zeros(3, np.int32), 1, f)[0]
        assert R["status"] == 0 and R["n_members"] == 3 and R["n_excluded"] == 0 and R["member_mask"][0] == 7 and R["frame"] == f
        rv, tv = truth[0]
        if noise == 0.0:
            assert rot_err_deg(R["rvec"], rv) < 2e-3 and np.linalg.norm(R["tvec"] - tv) < 2e-2, f
            continue
        # the concatenated correspondences restated in numpy (all features inner: corners 0 1 4 5 2 3 6 7, no end skip)
        img, X = [], []
        for k in range(int(res["n_markers"])):
            M = res["markers"][k]
            mi = int(np.nonzero(rig["ids"] == M["marker_id"])[0][0])
            for F in res["features"][M["first_feature"]:M["first_feature"] + M["n_features"]]:
                for c in (0, 1, 4, 5, 2, 3, 6, 7):
                    img.append(F["corners"][2 * c:2 * c + 2])
                    X.append(rig["corners"][mi][F["pos"] * 8 + c])
        img, X = np.array(img, np.float32).astype(np.float64), np.array(X, np.float32).astype(np.float64)
        assert len(X) == R["n_points"]
        xn = (img - K64[[0, 1], [2, 2]]) / K64[[0, 1], [0, 1]]
        x = xn.copy()
        for _ in range(5):
            r2 = (x ** 2).sum(1)
            icd = 1.0 / (1 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2)
            dx = 2 * d[2] * x[:, 0] * x[:, 1] + d[3] * (r2 + 2 * x[:, 0] ** 2)
            dy = d[2] * (r2 + 2 * x[:, 1] ** 2) + 2 * d[3] * x[:, 0] * x[:, 1]
            x = np.stack([(xn[:, 0] - dx) * icd, (xn[:, 1] - dy) * icd], 1)
        obs = (x * K64[[0, 1], [0, 1]] + K64[[0, 1], [2, 2]]).astype(np.float32).astype(np.float64)

        def resid(q):
            P = X @ rodrigues(q[:3]).T + q[3:]
            return np.concatenate([K64[0, 0] * P[:, 0] / P[:, 2] + K64[0, 2] - obs[:, 0], K64[1, 1] * P[:, 1] / P[:, 2] + K64[1, 2] - obs[:, 1]])

        mine = np.concatenate([R["rvec"], R["tvec"]])
        assert abs(0.5 * (resid(mine) ** 2).sum() - R["cost"]) < 1e-9 * max(1.0, R["cost"])
        near = least_squares(resid, mine + np.array([1e-3, -1e-3, 1e-3, 1.0, -1.0, 1.0]), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                             x_scale="jac")
        assert abs(R["cost"] - near.cost) < 1e-9 * max(1.0, near.cost), (R["cost"], near.cost)
        assert np.abs(rodrigues(R["rvec"]) - rodrigues(near.x[:3])).max() < 1e-6
        assert np.abs(R["tvec"] - near.x[3:]).max() < 1e-4 * np.linalg.norm(R["tvec"])
        assert rot_err_deg(R["rvec"], rv) < 0.2


def test_rig_accuracy_beats_per_marker_poses(env):
    """tools/rig_study.py at 0.2 px (seed 7, fewer frames): the rig's median rotation and translation errors are at least 2x below
    the per-marker medians (measured about 4x over 300 frames)."""
    s = rig_study(env["po"], env["rig"], env["K"], env["dist"], env["cam"], env["mv"], n_frames=120, noise_px=0.2, seed=7)
    (mr, mt), (rr, rt) = s["marker"], s["rig"]
    assert len(rr) == 120 and len(mr) >= 300
    assert np.median(mr) >= 2 * np.median(rr), (np.median(mr), np.median(rr))
    assert np.median(mt) >= 2 * np.median(rt), (np.median(mt), np.median(rt))


def test_rigs_create_checks_arguments_and_rig_calls_have_no_fallback():
    L = capi.load_library()
    model = ca.Model(MODEL_PATH)  # host-only object: no GPU needed
    good = np.array([0, 0, 1, -1, 1, 0], np.int32)
    i32 = C.POINTER(C.c_int32)
    r = C.c_void_p()
    assert L.ctag_rigs_create(model.m, good.ctypes.data_as(i32), 2, C.byref(r)) == 0 and r.value
    L.ctag_rigs_free(r)
    L.ctag_rigs_free(None)  # harmless
    for bad, n_rigs in ((np.array([0, 0, 2, -1, 1, 0], np.int32), 2), (np.array([0, -2, 1, -1, 1, 0], np.int32), 2), (good, 0), (good, -1)):
        r = C.c_void_p()
        assert L.ctag_rigs_create(model.m, bad.ctypes.data_as(i32), n_rigs, C.byref(r)) == capi.ERR_ARG and not r.value
    assert L.ctag_rigs_create(None, good.ctypes.data_as(i32), 2, C.byref(r)) == capi.ERR_ARG
    assert L.ctag_rigs_create(model.m, None, 2, C.byref(r)) == capi.ERR_ARG
    assert L.ctag_rigs_create(model.m, good.ctypes.data_as(i32), 2, None) == capi.ERR_ARG
    with pytest.raises(ca.CtagError):
        ca.Rigs(model, [0, 0, 7, -1, 1, 0], n_rigs=2)
    rigs = ca.Rigs(model, good)
    assert rigs.n_rigs == 2
    cam = ca.load_camera(CAM_PATH)
    res = np.zeros(1, ca.RESULT_DT)
    out = np.full(2, 0x5a, np.uint8).repeat(ca.RIG_POSE_DT.itemsize)
    # a null handle is an argument error; there is no host implementation to fall back to
    assert L.ctag_estimate_rig_pose(None, res.ctypes.data, model.m, rigs.r, C.byref(cam), out.ctypes.data) == capi.ERR_ARG
    assert L.ctag_rig_pose_batch_device(None, res.ctypes.data, 1, model.m, rigs.r, C.byref(cam), out.ctypes.data) == capi.ERR_ARG
    assert (out == 0x5a).all()
    rigs.close()
    model.close()
