"""CPU tests of the numpy statement of the dense edge-based pose refinement (tests/dense_testlib.py): its derivatives,
camera model and edge search against independent checks, its behaviour at a known pose, and the accuracy study behind
docs/history.md ("Dense pose refinement: measured before building").  No GPU."""
import os

import numpy as np
import pytest

import dense_testlib as dt
import testkit as tk
from ctag_testlib import GOLDEN, RESULT_DT
from pose_testlib import POSE_DT, project, read_camera_yml, rodrigues


def _rotvec(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w * (th / (2 * np.sin(th))) if th > 1e-12 else 0.5 * w


@pytest.fixture(scope="module")
def scene():
    state, fs, model, K = dt.synth_scene()
    return {"state": state, "model": model, "K": K, "cam": dt.Cam(K, np.zeros(5))}


def _marker_segments(model, row):
    C = model["corners"][row].astype(np.float64)
    segs = [(C[p * 8 + a], C[p * 8 + b], C[p * 8 + oa], C[p * 8 + ob]) for p in range(model["size"]) for a, b, oa, ob in dt.SIDES]
    s = np.array(segs)
    return s[:, 0], s[:, 1], s[:, 2], s[:, 3]


def test_rotation_derivatives_match_finite_differences():
    rng = np.random.default_rng(1)
    for scale in (1e-14, 1e-3, 0.5, 2.5):
        r = rng.normal(size=3) * scale
        R, dR = dt.rot_and_derivs(r)
        assert np.abs(R - rodrigues(r)).max() < 1e-14
        for k in range(3):
            e = np.zeros(3)
            e[k] = 1e-6
            num = (rodrigues(r + e) - rodrigues(r - e)) / 2e-6
            assert np.abs(dR[k] - num).max() < 1e-8, (scale, k)


def test_residual_jacobians_match_finite_differences(scene):
    """Analytic Jacobians of the corner residuals and of the signed edge distances."""
    rng = np.random.default_rng(2)
    a, b, _, _ = _marker_segments(scene["model"], 3)
    Xc = scene["model"]["corners"][3][:40].astype(np.float64)
    r0, t0 = np.array([0.3, -0.2, 0.1]), np.array([10.0, -5.0, 600.0])
    obs = dt.pinhole_and_jac(scene["cam"], rodrigues(r0), dt.rot_and_derivs(r0)[1], t0, Xc)[0] + rng.normal(0, 0.5, (40, 2))
    y = dt.pinhole_and_jac(scene["cam"], rodrigues(r0), dt.rot_and_derivs(r0)[1], t0, a)[0] + rng.normal(0, 1.0, (a.shape[0], 2))
    rc, e, Jc, Je = dt._terms(scene["cam"], r0, t0, Xc, obs, a, b, y, True, dt.DEFAULTS)
    x0 = np.concatenate([r0, t0])
    for k in range(6):
        h = 1e-7 if k < 3 else 1e-4
        xp, xm = x0.copy(), x0.copy()
        xp[k] += h
        xm[k] -= h
        rp, ep, _, _ = dt._terms(scene["cam"], xp[:3], xp[3:], Xc, obs, a, b, y, False, dt.DEFAULTS)
        rm, em, _, _ = dt._terms(scene["cam"], xm[:3], xm[3:], Xc, obs, a, b, y, False, dt.DEFAULTS)
        assert np.allclose(Jc[:, k], (rp - rm) / (2 * h), rtol=1e-5, atol=1e-5 * np.abs(Jc[:, k]).max()), k
        assert np.allclose(Je[:, k], (ep - em) / (2 * h), rtol=1e-5, atol=1e-5 * np.abs(Je[:, k]).max()), k


def test_camera_model_and_undistortion_against_the_reference_camera():
    """project_full agrees with pose_testlib.project (k1 k2 p1 p2 k3), and undistort_px maps it back to the pinhole pixel."""
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    cam = dt.Cam(K, dist)
    rng = np.random.default_rng(3)
    X = np.column_stack([rng.uniform(-60, 60, 300), rng.uniform(-40, 40, 300), rng.uniform(500, 900, 300)])
    uv = dt.project_full(cam, np.eye(3), np.zeros(3), X)
    assert np.allclose(uv, project(K, dist, np.zeros(3), np.zeros(3), X), atol=1e-9)
    pin = dt.project_full(dt.Cam(K, np.zeros(5)), np.eye(3), np.zeros(3), X)
    assert np.abs(dt.undistort_px(cam, uv) - pin).max() < 2e-3


def test_edge_search_is_unbiased_at_the_planted_pose(scene):
    """At the planted pose every long side's found offset is centred on 0 (the sub-pixel estimator's spread is what is left),
    the normals point from the black quad to the paper, and the search drops nothing inside a clean frame."""
    offs = []
    for f in (0, 1):
        img, truth = tk.synth3d_frame_host(scene["state"], f, dt.K_PLANTED, rows=dt.ROWS, cols=dt.COLS)
        for k in range(truth["n_markers"]):
            R, t = truth["R"][k].reshape(3, 3), truth["t"][k]
            segs = _marker_segments(scene["model"], int(truth["dict_row"][k]))
            s = dt.search_edges(img, scene["cam"], _rotvec(R), t, *segs, dt.DEFAULTS)
            assert s["keep"].mean() > 0.95
            P, n = s["point"][s["keep"]], s["normal"][s["keep"]]
            dark = dt.bilinear(img, P[:, 0] - 2 * n[:, 0], P[:, 1] - 2 * n[:, 1])
            bright = dt.bilinear(img, P[:, 0] + 2 * n[:, 0], P[:, 1] + 2 * n[:, 1])
            assert np.median(bright - dark) > 100
            offs.append(s["offset"][s["keep"]])
    o = np.concatenate(offs)
    assert abs(np.median(o)) < 0.02 and np.median(np.abs(o)) < 0.12 and np.abs(o).max() < 0.5, (np.median(o), np.abs(o).max())


def test_a_pose_at_the_truth_stays_there(scene):
    """A record already at the planted pose, whose corners are the exact projections of the model, on a noise-free frame:
    the refinement keeps the translation to 1e-4 of the distance but turns the pose by up to ~0.02 degrees (0.003 - 0.018 on
    frame 0's four markers), more than the 0.01 degrees a refinement that improves on PoseBA would have to stay within: the
    minimum of the edge term is not at the truth even where the found edges are unbiased on average (docs/history.md)."""
    img, truth = tk.synth3d_frame_host(scene["state"], 0, dt.K_PLANTED, rows=dt.ROWS, cols=dt.COLS)
    res = np.zeros(1, RESULT_DT)[0]
    moved = []
    for k in range(truth["n_markers"]):
        row = int(truth["dict_row"][k])
        R, t = truth["R"][k].reshape(3, 3), truth["t"][k]
        rv = _rotvec(R)
        size = scene["model"]["size"]
        res["markers"][0] = (row, 0, size, size)
        res["features"]["pos"][:size] = np.arange(size)
        rec = np.zeros(1, POSE_DT)[0]
        rec["rvec"], rec["tvec"] = rv, t
        Xc = scene["model"]["corners"][row].astype(np.float64)
        obs = dt.pinhole_and_jac(scene["cam"], R, dt.rot_and_derivs(rv)[1], t, Xc)[0].astype(np.float32)
        r1, t1, info = dt.refine_record(img, scene["cam"], res, rec, scene["model"]["corners"][row], size, Xc, obs)
        assert info["status"] in (dt.DENSE_OK, dt.DENSE_REJECTED) and info["n_kept"] > 0.95 * info["n_samples"]
        ang = np.degrees(np.arccos(np.clip((np.trace(rodrigues(r1).T @ R) - 1) / 2, -1, 1)))
        moved.append(ang)
        assert np.linalg.norm(t1 - t) < 1e-4 * np.linalg.norm(t)
    assert max(moved) < 0.03, moved


def test_statuses_and_pass_through(scene):
    """A record that is not CTAG_POSE_OK is skipped and returned unchanged; a frame without edges keeps the input pose
    (too few samples)."""
    size = scene["model"]["size"]
    res = np.zeros(1, RESULT_DT)[0]
    res["markers"][0] = (2, 0, size, size)
    res["features"]["pos"][:size] = np.arange(size)
    rec = np.zeros(1, POSE_DT)[0]
    rec["rvec"], rec["tvec"] = [0.1, 0.2, 0.3], [5.0, 3.0, 700.0]
    Xc = scene["model"]["corners"][2].astype(np.float64)
    obs = np.zeros((Xc.shape[0], 2), np.float32)
    flat = np.full((dt.ROWS, dt.COLS), 128, np.uint8)
    for status, want in ((1, dt.DENSE_SKIPPED), (0, dt.DENSE_FEW_SAMPLES)):
        rec["status"] = status
        r, t, info = dt.refine_record(flat, scene["cam"], res, rec, scene["model"]["corners"][2], size, Xc, obs)
        assert info["status"] == want and np.array_equal(r, rec["rvec"]) and np.array_equal(t, rec["tvec"])
    assert info["n_kept"] == 0 and info["n_samples"] == size * 4 * 8


def test_measured_accuracy_against_planted_poses():
    """The study of docs/history.md on a small slice (12 frames each): with the default parameters the dense pose has a lower
    median translation error than PoseBA on clean and on degraded frames, and a higher median rotation error -- which is why
    the refinement was not built into the product (the gate of the issue: at least as good on clean frames, better on
    degraded ones, in both measures)."""
    for degraded in (False, True):
        E, st = dt.run(12, degraded=degraded)
        assert E.shape[0] >= 40 and (st == dt.DENSE_OK).mean() > 0.95
        med = np.median(E, 0)
        assert med[3] < med[1], (degraded, med)
        assert med[2] > med[0], (degraded, med)
