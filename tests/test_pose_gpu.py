"""GPU parity of the pose back end (k_pose.hip through the C ABI of include/ctag_pose.h) against the CPU oracle.

Floating point (FP64): the stated bar is |rvec diff| <= 1e-9 rad and |tvec diff| <= 1e-9 * max(1, |tvec|) with equal
status / model index / point count.  The kernel accumulates every sum in the oracle's order and shares its
deterministic math header, so the records are in fact required to be byte-identical here; the tolerance is the
fallback bar should a toolchain change break bit-equality (the assertion message then says which one failed)."""
import os

import numpy as np
import pytest

import cylindertag_amd as ca
import testkit as tk
from ctag_testlib import GOLDEN, read_bmp_gray
from pose_testlib import PoseOracle, make_camera, make_model_view, read_camera_yml, read_model_file, synth_pose_results

pytestmark = pytest.mark.gpu

MODEL_PATH = os.path.join(GOLDEN, "CTag_2f12c.model")
CAM_PATH = os.path.join(GOLDEN, "cameraParams.yml")


@pytest.fixture(scope="module")
def env():
    K, dist = read_camera_yml(CAM_PATH)
    model = read_model_file(MODEL_PATH)
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    e = {"K": K, "dist": dist, "model": model, "cam_o": make_camera(K, dist), "mv": make_model_view(model),
         "po": PoseOracle(), "det": det, "M": ca.Model(MODEL_PATH), "cam": ca.load_camera(CAM_PATH)}
    yield e
    det.close()


def assert_pose_parity(got, want, what):
    assert len(got) == len(want), what
    for k in ("status", "model_index", "frame", "marker", "n_points"):
        assert np.array_equal(got[k], want[k]), (what, k)
    ok = want["status"] == 0
    for k in ("rvec", "rvec0"):
        assert np.abs(got[k][ok] - want[k][ok]).max(initial=0) <= 1e-9, (what, k)
    for k in ("tvec", "tvec0"):
        scale = np.maximum(1.0, np.abs(want[k][ok]).max(axis=1, initial=0))[:, None]
        assert (np.abs(got[k][ok] - want[k][ok]) / scale).max(initial=0) <= 1e-9, (what, k)
    assert got.tobytes() == want.tobytes(), "%s: within tolerance but not byte-identical" % what


def test_reference_scene_pose_parity(env):
    """test.bmp -> HIP detect -> HIP pose == oracle pose of the same records; sub-pixel reprojection RMS."""
    res = env["det"].detect(read_bmp_gray(os.path.join(GOLDEN, "test.bmp")), 5, True, 5)
    got = env["det"].estimate_pose(res, env["M"], env["cam"])
    want = env["po"].pose_frame(res, env["mv"], env["cam_o"])
    assert_pose_parity(got, want, "test.bmp")
    assert [int(p["model_index"]) for p in got] == [5, 0, 1, 3, 2]
    for p in got:
        assert np.sqrt(2 * p["cost"] / p["n_points"]) < 0.6


def test_batch_pose_parity_device_records(env):
    """512 frames of synthetic detection records in HBM (random poses of the reference's models, every branch of the
    correspondence builder, markers without a model, markers of 4 to 56 points) through ctag_pose_batch_device.  Larger
    markers, up to the 160 points of the large form, are in test_pose_forms_gpu.py."""
    import torch
    recs, truth = synth_pose_results(env["model"], env["K"], env["dist"], 512, 1)
    d = torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1)).cuda()
    off = torch.zeros(len(recs) + 1, dtype=torch.int32, device="cuda")
    cap = int(recs["n_markers"].sum())
    poses = torch.zeros(max(cap, 1) * ca.POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    env["det"].pose_batch_device(d.data_ptr(), len(recs), env["M"], env["cam"], off.data_ptr(), poses.data_ptr(), cap)
    env["det"].sync()
    offs = off.cpu().numpy()
    assert offs[0] == 0 and offs[-1] == cap and np.array_equal(np.diff(offs), recs["n_markers"])
    P = poses.cpu().numpy().view(ca.POSE_DT)[:cap]
    for f in range(len(recs)):
        want = env["po"].pose_frame(recs[f], env["mv"], env["cam_o"], f)
        assert_pose_parity(P[offs[f]:offs[f + 1]], want, "frame %d" % f)
    assert {0, 1} <= set(int(s) for s in P["status"])
    good = [np.abs(P[offs[f] + k]["tvec"] - tv).max() for f in range(len(recs)) for k, (mi, rv, tv) in enumerate(truth[f])
            if P[offs[f] + k]["status"] == 0 and P[offs[f] + k]["n_points"] >= 16]
    assert np.median(good) < 1.0  # millimetres at 0.2 px noise


def test_pose_edge_cases(env):
    """Frames without markers, failed frames, capacity smaller than the batch, bad feature positions."""
    import torch
    recs, _ = synth_pose_results(env["model"], env["K"], env["dist"], 16, 5)
    recs[3]["status"] = 1           # CTAG_NO_CORNER frame: no pose records
    recs[4]["n_markers"] = 0
    recs[5]["features"][0]["pos"] = 12   # outside the model
    d = torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1)).cuda()
    off = torch.zeros(len(recs) + 1, dtype=torch.int32, device="cuda")
    need = int(sum(r["n_markers"] for r in recs if r["status"] == 0))
    for cap in (need, max(need - 3, 1)):
        poses = torch.zeros(need * ca.POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
        env["det"].pose_batch_device(d.data_ptr(), len(recs), env["M"], env["cam"], off.data_ptr(), poses.data_ptr(), cap)
        env["det"].sync()
        offs = off.cpu().numpy()
        assert offs[-1] == need and offs[4] == offs[3] and offs[5] == offs[4]
        P = poses.cpu().numpy().view(ca.POSE_DT)
        want = np.concatenate([env["po"].pose_frame(recs[f], env["mv"], env["cam_o"], f) for f in range(len(recs))])
        assert P[:cap].tobytes() == want[:cap].tobytes()
        assert not P[cap:need].view(np.uint8).any()  # surplus not computed
    # single-frame host entry point on a frame whose status is not OK: no records, no error
    assert len(env["det"].estimate_pose(recs[3], env["M"], env["cam"])) == 0


def test_cpp_estimate_pose_demo(env):
    """The C++ host layer with the reference's call sequence (main.cpp:31-40): CylinderTag marker(...); loadModel; loadCamera;
    detect; estimatePose -- the printed poses equal the oracle's for every marker that has a model, in order, with
    PoseInfo::markerID = model index."""
    import subprocess
    from ctag_testlib import ROOT
    exe = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_demo")
    out = subprocess.check_output([exe, os.path.join(GOLDEN, "CTag_2f12c.marker"), os.path.join(GOLDEN, "test.bmp"), "5", "1", "5",
                                   MODEL_PATH, CAM_PATH], timeout=120).decode()
    lines = [l.split() for l in out.splitlines() if l.startswith("pose ")]
    res = env["det"].detect(read_bmp_gray(os.path.join(GOLDEN, "test.bmp")), 5, True, 5)
    want = [p for p in env["po"].pose_frame(res, env["mv"], env["cam_o"]) if p["status"] != ca.capi.POSE_NO_MODEL]
    assert "poses %d" % len(want) in out and len(lines) == len(want) == 5
    for l, p in zip(lines, want):
        assert int(l[1]) == p["model_index"]
        assert [float(v) for v in l[3:6]] == list(p["rvec"]) and [float(v) for v in l[7:10]] == list(p["tvec"])


def test_config5_4k_detect_plus_pose_known_answers(env):
    """BASELINE config 5 end to end on the GPU at 3840x2160: ray-cast cylinders with planted poses (rendered on the device,
    identical to the host rendering), detect(img,5,true,5), ctag_pose_batch_device with the objects' 3-D corner lists --
    pose records byte-identical to the CPU pose oracle on the oracle's detection records, and the planted poses recovered."""
    import torch
    from ctag_testlib import Oracle
    from pose_testlib import rodrigues
    det = env["det"]
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    rows, cols, n = 2160, 3840, 6
    K = np.array([[5200.0, 0, 1920.0], [0, 5200.0, 1080.0], [0, 0, 1]])
    M, corners = tk.synth3d_model(state)
    ids = np.arange(state.shape[0], dtype=np.int32)
    mv = make_model_view({"ids": ids, "size": state.shape[1], "base": np.zeros((len(ids), 3), np.float32),
                          "axis": np.zeros((len(ids), 3), np.float32), "corners": corners})
    cam_c, cam_o = ca.make_camera(K, np.zeros(5)), make_camera(K, np.zeros(5))
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    det.synth3d_frames_device(frames.data_ptr(), 0, n, rows, cols, cols, rows * cols, K)
    host0, truth0 = tk.synth3d_frame_host(state, 0, K)
    assert (frames[0].cpu().numpy() == host0).all()
    res = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    det.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, res.data_ptr(), 5, True, 5)
    off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    poses = torch.zeros(n * 8 * ca.POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    det.pose_batch_device(res.data_ptr(), n, M, cam_c, off.data_ptr(), poses.data_ptr(), n * 8)
    det.sync()
    recs = np.frombuffer(res.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    offs = off.cpu().numpy()
    P = np.frombuffer(poses.cpu().numpy().tobytes(), dtype=ca.POSE_DT)[:offs[-1]]
    orc = Oracle()
    for f in (0, n - 1):  # detection parity at 4K on two frames (the oracle takes ~1 s per 4K frame)
        want = orc.detect_fast(frames[f].cpu().numpy(), state, fs)
        assert recs[f].tobytes() == want.tobytes(), "4K detection record %d" % f
    want_p = np.concatenate([env["po"].pose_frame(recs[f], mv, cam_o, f) for f in range(n)])
    assert_pose_parity(P, want_p, "config 5 poses")
    assert P.tobytes() == want_p.tobytes()
    nposes = 0
    for f in range(n):
        img_f, truth = (host0, truth0) if f == 0 else tk.synth3d_frame_host(state, f, K)  # the planted poses (and the host rendering)
        assert (frames[f].cpu().numpy() == img_f).all()
        planted = sorted(int(x) for x in truth["dict_row"][:truth["n_markers"]])
        found = sorted(int(m["marker_id"]) for m in recs[f]["markers"][:recs[f]["n_markers"]])
        assert set(found) <= set(planted) and len(found) >= len(planted) - 1, f
        for p in P[offs[f]:offs[f + 1]]:
            assert p["status"] == 0
            k = [i for i in range(truth["n_markers"]) if truth["dict_row"][i] == ids[p["model_index"]]][0]
            R, Rt = rodrigues(p["rvec"]), truth["R"][k].reshape(3, 3)
            ang = np.degrees(np.arccos(np.clip((np.trace(R.T @ Rt) - 1) / 2, -1, 1)))
            rel = np.linalg.norm(p["tvec"] - truth["t"][k]) / np.linalg.norm(truth["t"][k])
            assert ang < 0.1 and rel < 5e-4 and np.sqrt(2 * p["cost"] / p["n_points"]) < 0.3, (f, ang, rel)
            nposes += 1
    assert nposes >= 4 * n - 4
