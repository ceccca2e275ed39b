"""GPU overlay of CylinderTag::drawAxis (k_draw.hip through ctag_draw_axis / ctag_draw_axis_batch_device of
include/ctag_pose.h) against the sequential numpy painter of tests/draw_testlib.py: every check is byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

import cylindertag_amd as ca
from cylindertag_amd import capi
import testkit as tk
import draw_testlib as D
from ctag_testlib import GOLDEN, ROOT, read_bmp_gray
from pose_testlib import read_camera_yml, read_model_file, synth_pose_results

pytestmark = pytest.mark.gpu

MODEL_PATH = os.path.join(GOLDEN, "CTag_2f12c.model")
CAM_PATH = os.path.join(GOLDEN, "cameraParams.yml")
DEMO = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_demo")


@pytest.fixture(scope="module")
def env():
    K, dist = read_camera_yml(CAM_PATH)
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    e = {"K": K, "dist": dist, "model": read_model_file(MODEL_PATH), "det": det, "M": ca.Model(MODEL_PATH),
         "cam": ca.load_camera(CAM_PATH)}
    yield e
    det.close()


def records_from_truth(recs, truth, first_frame=0):
    """Pose records (ctag_pose_batch_device's layout: one per marker, in marker order) with the synthetic ground-truth poses."""
    out = []
    for f, tf in enumerate(truth):
        for k, (mi, rv, tv) in enumerate(tf):
            p = np.zeros(1, ca.POSE_DT)[0]
            p["status"] = capi.POSE_OK if mi >= 0 else capi.POSE_NO_MODEL
            p["model_index"] = mi
            p["frame"] = first_frame + f
            p["marker"] = k
            p["rvec"], p["tvec"] = rv, tv
            out.append(p)
    return np.array(out, ca.POSE_DT)


def offsets_of(P, n):
    off = np.zeros(n + 1, np.int32)
    for f in range(n):
        off[f + 1] = off[f] + int((P["frame"] == f).sum())
    return off


def gray3(g):
    return np.repeat(g[:, :, None], 3, axis=2)


def test_reference_scene_detect_pose_draw(env):
    """test.bmp -> detect -> estimate_pose -> draw_axis (axisLength 30 as main.cpp:41) == the painter; pixels outside every
    primitive's box are gray x 3."""
    g = read_bmp_gray(os.path.join(GOLDEN, "test.bmp"))
    res = np.asarray(env["det"].detect(g, 5, True, 5)).reshape(1)
    poses = env["det"].estimate_pose(res, env["M"], env["cam"])
    assert len(poses) == 5 and (poses["status"] == 0).all()
    got = env["det"].draw_axis(g, res, poses, env["M"], env["cam"], 30)
    want = D.draw_axis(g, res[0], poses, env["model"], env["K"], env["dist"], 30)
    assert got.tobytes() == want.tobytes()
    assert (got != gray3(g)).any()
    inside = np.zeros(g.shape, bool)
    for p in poses:
        pos = D.record_positions(res[0], p, env["model"])
        uv = D.project_points(D.model_points(env["model"], int(p["model_index"]), pos, 30), p["rvec"], p["tvec"], env["K"], env["dist"])
        pts = [D.to_point(q) for q in uv]
        base = pts[-4]
        for q in pts[:-5] + [base]:
            inside[max(q[1] - 9, 0):q[1] + 10, max(q[0] - 9, 0):q[0] + 10] = True
        for end in pts[-3:]:
            ends = [base, end] + D.arrow_tips(base, end)
            xs, ys = [e[0] for e in ends], [e[1] for e in ends]
            inside[max(min(ys) - 8, 0):max(ys) + 9, max(min(xs) - 8, 0):max(xs) + 9] = True
    assert (got[~inside] == gray3(g)[~inside]).all()


# (n_dist, axis_length) of the eight groups of 32 frames: every distortion model, arrows short, usual and leaving the frame
GROUPS = [(0, 5), (5, 30), (8, 300), (14, 30), (14, 300), (5, 5), (0, 300), (8, 30)]


def camera_for(K, dist, n_dist, rng):
    d = np.zeros(14, np.float32)
    d[:5] = dist[:5]
    if n_dist >= 8:
        d[5:8] = rng.normal(0, 0.5, 3)
    if n_dist >= 14:
        d[8:12] = rng.normal(0, 0.005, 4)
    return d[:n_dist]


def test_batch_device_synthetic_frames(env):
    """256 synthetic frames (random poses, up to 5 markers; NO_MODEL and BAD_POS records; a marker behind the camera; 0/5/8/14
    distortion terms; axis lengths 5/30/300) through ctag_draw_axis_batch_device == the painter; the first frames of each
    group through the host call give the same bytes."""
    import torch
    rows, cols = 600, 960
    rng = np.random.default_rng(7)
    K = env["K"].copy()
    K[0, 2], K[1, 2] = 480.0, 300.0
    for gi, (nd, L) in enumerate(GROUPS):
        dist = camera_for(env["K"], env["dist"], nd, rng)
        cam = ca.make_camera(K, dist)
        recs, truth = synth_pose_results(env["model"], K, env["dist"], 32, 100 + gi)
        P = records_from_truth(recs, truth)
        if gi == 2:  # a marker behind the camera
            P[0]["tvec"] = -P[0]["tvec"]
        if gi == 3 and len(P) > 2:
            P[1]["status"] = capi.POSE_BAD_POS
            recs[P[2]["frame"]]["features"][recs[P[2]["frame"]]["markers"][P[2]["marker"]]["first_feature"]]["pos"] = 12  # outside the model
        frames = rng.integers(0, 256, (32, rows, cols), dtype=np.uint8)
        off = offsets_of(P, 32)
        d_fr = torch.from_numpy(frames).cuda()
        d_res = torch.from_numpy(recs.view(np.uint8).reshape(32, -1)).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_p = torch.from_numpy(P.view(np.uint8).copy()).cuda() if len(P) else torch.zeros(1, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((32, rows, cols * 3), dtype=torch.uint8, device="cuda")
        env["det"].draw_axis_batch_device(d_fr.data_ptr(), 32, rows, cols, cols, rows * cols, d_res.data_ptr(), d_off.data_ptr(),
                                          d_p.data_ptr(), len(P), env["M"], cam, L, d_out.data_ptr(), cols * 3, rows * cols * 3)
        env["det"].sync()
        out = d_out.cpu().numpy().reshape(32, rows, cols, 3)
        for f in range(32):
            want = D.draw_axis(frames[f], recs[f], P[off[f]:off[f + 1]], env["model"], K, dist, L, frame=f)
            assert out[f].tobytes() == want.tobytes(), "group %d frame %d" % (gi, f)
            if f < 4:
                Pf = P[off[f]:off[f + 1]].copy()
                Pf["frame"] = 0
                host = env["det"].draw_axis(frames[f], recs[f], Pf, env["M"], cam, L)
                assert host.tobytes() == out[f].tobytes(), "group %d frame %d: host call" % (gi, f)


def two_overlapping(env):
    g = read_bmp_gray(os.path.join(GOLDEN, "test.bmp"))
    res = np.asarray(env["det"].detect(g, 5, True, 5)).reshape(1)
    poses = env["det"].estimate_pose(res, env["M"], env["cam"])
    a = poses[0].copy()
    b = poses[0].copy()  # the same marker under a pose a few millimetres and degrees away: the two overlays overlap
    b["tvec"] = a["tvec"] + np.array([3.0, 2.0, 0.0])
    b["rvec"] = a["rvec"] + np.array([0.0, 0.05, 0.1])
    return g, res, a, b


def test_overlapping_markers_record_order(env):
    g, res, a, b = two_overlapping(env)
    ab = env["det"].draw_axis(g, res, np.array([a, b]), env["M"], env["cam"], 30)
    ba = env["det"].draw_axis(g, res, np.array([b, a]), env["M"], env["cam"], 30)
    assert ab.tobytes() != ba.tobytes()
    assert ab.tobytes() == D.draw_axis(g, res[0], np.array([a, b]), env["model"], env["K"], env["dist"], 30).tobytes()
    assert ba.tobytes() == D.draw_axis(g, res[0], np.array([b, a]), env["model"], env["K"], env["dist"], 30).tobytes()


def test_padded_and_odd_strides(env):
    """Host call with an odd input stride and a padded output view; batch call with padded device strides: the pixels equal
    the painter, the padding bytes are untouched."""
    import torch
    g, res, a, b = two_overlapping(env)
    rows, cols = g.shape
    want = D.draw_axis(g, res[0], np.array([a, b]), env["model"], env["K"], env["dist"], 30)
    wide = np.zeros((rows, cols + 5), np.uint8)
    wide[:, 3:3 + cols] = g
    buf = np.full((rows, 3 * cols + 7), 0xAB, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (rows, cols, 3), (buf.strides[0], 3, 1))
    env["det"].draw_axis(wide[:, 3:3 + cols], res, np.array([a, b]), env["M"], env["cam"], 30, out=view)
    assert np.array_equal(buf[:, :3 * cols].reshape(rows, cols, 3), want)
    assert (buf[:, 3 * cols:] == 0xAB).all()
    # device: two frames, input rows 1923 bytes apart, output rows 3*cols + 13, frames a further 29 bytes apart
    rs, ors = cols + 3, 3 * cols + 13
    fs, ofs = rs * rows + 11, ors * rows + 29
    src = np.zeros(2 * fs, np.uint8)
    for f in range(2):
        src[f * fs:f * fs + rs * rows].reshape(rows, rs)[:, :cols] = g
    P = np.array([a, b, a, b])
    P["frame"] = [0, 0, 1, 1]
    d_src = torch.from_numpy(src).cuda()
    d_res = torch.from_numpy(np.concatenate([res, res]).view(np.uint8).reshape(2, -1)).cuda()
    d_off = torch.from_numpy(np.array([0, 2, 4], np.int32)).cuda()
    d_p = torch.from_numpy(P.view(np.uint8).copy()).cuda()
    d_out = torch.full((2 * ofs,), 0xCD, dtype=torch.uint8, device="cuda")
    env["det"].draw_axis_batch_device(d_src.data_ptr(), 2, rows, cols, rs, fs, d_res.data_ptr(), d_off.data_ptr(), d_p.data_ptr(), 4,
                                      env["M"], env["cam"], 30, d_out.data_ptr(), ors, ofs)
    env["det"].sync()
    o = d_out.cpu().numpy()
    for f in range(2):
        fr = o[f * ofs:f * ofs + ors * rows].reshape(rows, ors)
        assert np.array_equal(fr[:, :3 * cols].reshape(rows, cols, 3), want)
        assert (fr[:, 3 * cols:] == 0xCD).all()
    assert (o[ors * rows:ofs] == 0xCD).all() and (o[ofs + ors * rows:] == 0xCD).all()


def test_records_pointing_nowhere_draw_nothing(env):
    """Frame, marker and model index out of range, a frame whose status is not OK, records past `capacity`: the call returns
    normally and the output is gray x 3."""
    import torch
    g, res, a, b = two_overlapping(env)
    bad = np.array([a, a, a, a, a])
    bad[0]["frame"] = 5
    bad[1]["marker"] = 99
    bad[2]["marker"] = -1
    bad[3]["model_index"] = 77
    bad[4]["model_index"] = -3
    out = env["det"].draw_axis(g, res, bad, env["M"], env["cam"], 30)
    assert np.array_equal(out, gray3(g))
    failed = res.copy()
    failed["status"] = 1
    assert np.array_equal(env["det"].draw_axis(g, failed, np.array([a]), env["M"], env["cam"], 30), gray3(g))
    # batch: offsets that run past capacity and backwards
    rows, cols = g.shape
    d_g = torch.from_numpy(np.stack([g, g])).cuda()
    d_res = torch.from_numpy(np.concatenate([res, res]).view(np.uint8).reshape(2, -1)).cuda()
    d_off = torch.from_numpy(np.array([1, 1000, -5], np.int32)).cuda()
    P = np.array([a, a])
    P["frame"] = 0
    d_p = torch.from_numpy(P.view(np.uint8).copy()).cuda()
    d_out = torch.zeros((2, rows, cols * 3), dtype=torch.uint8, device="cuda")
    env["det"].draw_axis_batch_device(d_g.data_ptr(), 2, rows, cols, cols, rows * cols, d_res.data_ptr(), d_off.data_ptr(), d_p.data_ptr(), 1,
                                      env["M"], env["cam"], 30, d_out.data_ptr(), cols * 3, rows * cols * 3)
    env["det"].sync()
    o = d_out.cpu().numpy().reshape(2, rows, cols, 3)
    assert np.array_equal(o[0], gray3(g)) and np.array_equal(o[1], gray3(g))  # record 1 lies past capacity 1
    with pytest.raises(ca.CtagError):
        env["det"].draw_axis(g, res, np.array([a]), env["M"], env["cam"], -1)


def write_model(path, model, keep):
    with open(path, "w") as f:
        f.write("%d %d\n" % (len(keep), model["size"]))
        for i in keep:
            f.write("%d\n%.9g %.9g %.9g\n%.9g %.9g %.9g\n" % ((model["ids"][i],) + tuple(model["base"][i]) + tuple(model["axis"][i])))
            for c in range(model["size"] * 8):
                f.write("%d %.9g %.9g %.9g\n" % ((c,) + tuple(model["corners"][i, c])))


def test_cpp_class_pairing_and_demo_bmp(env, tmp_path):
    """ctag_demo (detect -> estimatePose -> drawAxis(30) -> BMP) with a model list that lacks the model of test.bmp's second
    marker: the C++ class pairs pose[i] with markers[i] as the reference does (after the erase), and the BMP equals draw_axis's
    bytes for records built that way, and the painter's."""
    from PIL import Image
    model = env["model"]
    keep = [i for i in range(len(model["ids"])) if i != 0]  # model 0 belongs to test.bmp's second marker
    mpath = str(tmp_path / "five.model")
    write_model(mpath, model, keep)
    sub = read_model_file(mpath)
    out_bmp = str(tmp_path / "annotated.bmp")
    p = subprocess.run([DEMO, os.path.join(GOLDEN, "CTag_2f12c.marker"), os.path.join(GOLDEN, "test.bmp"), "5", "1", "5", mpath, CAM_PATH,
                        out_bmp], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    poses = [(int(m.group(1)), [float(v) for v in m.group(2).split()], [float(v) for v in m.group(3).split()])
             for m in re.finditer(r"pose (-?\d+) rvec (\S+ \S+ \S+) tvec (\S+ \S+ \S+)", p.stdout)]
    assert len(poses) == 4
    g = read_bmp_gray(os.path.join(GOLDEN, "test.bmp"))
    res = np.asarray(env["det"].detect(g, 5, True, 5)).reshape(1)
    assert int(res[0]["n_markers"]) == 5
    P = np.zeros(4, ca.POSE_DT)
    for i, (mi, rv, tv) in enumerate(poses):
        P[i]["model_index"], P[i]["marker"], P[i]["rvec"], P[i]["tvec"] = mi, i, rv, tv
    got = np.asarray(Image.open(out_bmp).convert("RGB"))[:, :, ::-1]  # the file stores channel 0 first (as blue)
    M = ca.Model(mpath)
    want = env["det"].draw_axis(g, res, P, M, env["cam"], 30)
    assert got.tobytes() == want.tobytes()
    assert want.tobytes() == D.draw_axis(g, res[0], P, sub, env["K"], env["dist"], 30).tobytes()
    # the pairing is by position: record 1 draws pose 1 (the third marker's) on marker 1, unlike the per-marker records
    own = env["det"].estimate_pose(res, M, env["cam"])
    assert own[1]["status"] == capi.POSE_NO_MODEL
    assert env["det"].draw_axis(g, res, own, M, env["cam"], 30).tobytes() != want.tobytes()
