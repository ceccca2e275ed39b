"""The edge search of the dense pose-refinement study on the device (ctag_testkit_dense_edge_probe, include/ctag_testkit.h)
against the numpy statement of tests/dense_testlib.py, sample by sample: same keep decision, same found offset.  Poses and
segments come from the CPU oracles (detect + pose oracle), so only the search itself runs on the GPU."""
import os

import numpy as np
import pytest

import cylindertag_amd as ca
import dense_testlib as dt
import testkit as tk
from ctag_testlib import GOLDEN, Oracle, read_bmp_gray, read_marker_file
from pose_testlib import PoseOracle, make_camera, make_model_view, read_camera_yml, read_model_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    d = tk.Detector(state, fs, device=0)
    yield d
    d.close()


def _segments(res, rec, corners, size):
    a, b, oa, ob = dt.record_segments(res, rec, corners, size)
    return np.concatenate([a, b, oa, ob], 1)


def _compare(det, img, K, dist, res, poses, model, params, tally):
    cam = dt.Cam(K, dist)
    for p in poses:
        if p["status"] != 0:
            continue
        seg = _segments(res, p, model["corners"][p["model_index"]], model["size"])
        if seg.shape[0] == 0:
            continue
        want = dt.search_edges(img, cam, p["rvec"], p["tvec"], seg[:, 0:3], seg[:, 3:6], seg[:, 6:9], seg[:, 9:12], params)
        got = det.dense_edge_probe(img, seg, np.asarray(K, np.float32), np.asarray(dist, np.float32), p["rvec"], p["tvec"],
                                   params["samples_per_edge"], params["search_px"], params["min_contrast"])
        fin = np.isfinite(want["point"]).all(1)
        assert np.array_equal(fin, np.isfinite(got["point"]).all(1))
        assert np.abs(got["point"][fin] - want["point"][fin]).max(initial=0) < 1e-6
        assert np.abs(got["normal"][fin] - want["normal"][fin]).max(initial=0) < 1e-9
        both = got["keep"] & want["keep"]
        same = (got["keep"] == want["keep"])
        same[both] &= np.abs(got["offset"][both] - want["offset"][both]) < 1e-3
        assert np.isnan(got["offset"][~got["keep"]]).all()
        tally["n"] += same.size
        tally["same"] += int(same.sum())
        tally["kept"] += int(got["keep"].sum())


def test_probe_matches_numpy_on_the_reference_scene(det):
    """test.bmp with CTag_2f12c.model and cameraParams.yml (five distortion terms), at the PoseBA poses."""
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    model = read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model"))
    state, fs = read_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    img = read_bmp_gray(os.path.join(GOLDEN, "test.bmp"))
    res = Oracle().detect_fast(img, state, fs, 5, True, 5)
    poses = PoseOracle().pose_frame(res, make_model_view(model), make_camera(K, dist))
    assert (poses["status"] == 0).sum() == 5
    tally = {"n": 0, "same": 0, "kept": 0}
    for params in (dt.DEFAULTS, dict(dt.DEFAULTS, samples_per_edge=5, search_px=2.25, min_contrast=3.0)):
        _compare(det, img, K, dist, res, poses, model, params, tally)
    assert tally["kept"] > 0.5 * tally["n"]
    assert tally["same"] >= 0.995 * tally["n"], tally


@pytest.mark.parametrize("degraded", [False, True])
def test_probe_matches_numpy_on_synthetic_3d_frames(det, degraded):
    """64 ray-cast frames with planted poses (clean, then blurred and noisy), at the PoseBA poses of the CPU oracles."""
    state, fs, model, K = dt.synth_scene()
    orc, po = Oracle(), PoseOracle()
    mv, cam = make_model_view(model), make_camera(K, np.zeros(5))
    tally = {"n": 0, "same": 0, "kept": 0}
    for f in range(64):
        img, _ = tk.synth3d_frame_host(state, f, dt.K_PLANTED, rows=dt.ROWS, cols=dt.COLS)
        if degraded:
            img = dt.degrade(img, 1000 + f)
        res = orc.detect_fast(img, state, fs)
        if res["status"] != 0:
            continue
        _compare(det, img, K, np.zeros(5), res, po.pose_frame(res, mv, cam), model, dt.DEFAULTS, tally)
    assert tally["n"] > 40000 and tally["kept"] > 0.8 * tally["n"]
    assert tally["same"] >= 0.995 * tally["n"], tally


def test_probe_padded_stride_and_frame_border(det):
    """A padded row stride reads the same pixels; a pose whose samples run off the frame drops them all."""
    state, fs, model, K = dt.synth_scene()
    img, truth = tk.synth3d_frame_host(state, 0, dt.K_PLANTED, rows=dt.ROWS, cols=dt.COLS)
    R = truth["R"][0].reshape(3, 3)
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    rv = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * th / (2 * np.sin(th))
    C = model["corners"][int(truth["dict_row"][0])].astype(np.float64)
    seg = np.array([np.concatenate([C[p * 8 + a], C[p * 8 + b], C[p * 8 + oa], C[p * 8 + ob]])
                    for p in range(model["size"]) for a, b, oa, ob in dt.SIDES])
    base = det.dense_edge_probe(img, seg, K, np.zeros(5), rv, truth["t"][0])
    padded = np.full((img.shape[0], img.shape[1] + 77), 255, np.uint8)
    padded[:, :img.shape[1]] = img
    got = det.dense_edge_probe(padded[:, :img.shape[1]], seg, K, np.zeros(5), rv, truth["t"][0])
    assert np.array_equal(got["keep"], base["keep"]) and base["keep"].mean() > 0.95
    assert np.array_equal(got["offset"][got["keep"]], base["offset"][base["keep"]])
    off = det.dense_edge_probe(img, seg, K, np.zeros(5), rv, truth["t"][0] + np.array([1e4, 0, 0]))
    assert not off["keep"].any() and np.isnan(off["offset"]).all()


def test_probe_argument_checks(det):
    img = np.zeros((64, 64), np.uint8)
    seg = np.zeros((1, 12))
    K = np.array([[100.0, 0, 32], [0, 100, 32], [0, 0, 1]])
    for kw in ({"samples_per_edge": 0}, {"samples_per_edge": 65}, {"search_px": 8.25}, {"search_px": 0.3}, {"search_px": 1.1},
               {"min_contrast": -1.0}):
        with pytest.raises(ca.CtagError):
            det.dense_edge_probe(img, seg, K, np.zeros(5), np.zeros(3), np.array([0, 0, 100.0]), **kw)
    with pytest.raises(ca.CtagError):
        det.dense_edge_probe(np.zeros((1, 64), np.uint8), seg, K, np.zeros(5), np.zeros(3), np.array([0, 0, 100.0]))
