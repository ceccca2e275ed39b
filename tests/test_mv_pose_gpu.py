"""GPU tests of the multi-view rig pose (k_mv_pose.hip through ctag_mv_rig_pose_batch_device / ctag_estimate_mv_rig_pose of
include/ctag_pose.h).  Where every camera has the same intrinsics and a zero pose the whole record is pinned byte for byte to the
unmodified pose oracle (EPnP + PoseBA on the start camera's points, PoseBA again over the concatenation of all cameras' points);
with real camera poses every record is checked against the statement of tests/mv_statement.py and scipy's minimum."""
import os
import subprocess

import numpy as np
import pytest

import cylindertag_amd as ca
import mv_statement as ms
import testkit as tk
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, ROOT, RESULT_DT, read_bmp_gray
from mv_testlib import synth_mv_instant
from pose_testlib import PoseOracle, make_camera, make_model_view, planar_model, read_camera_yml, read_model_file, test_cameras
from rig_testlib import add_marker, compose_rig_poses, cylinder_model, random_pose, stacked_rig_model

pytestmark = pytest.mark.gpu

MODEL_PATH = os.path.join(GOLDEN, "CTag_2f12c.model")
CAM_PATH = os.path.join(GOLDEN, "cameraParams.yml")
ZERO = (np.zeros(3), np.zeros(3))
SZ = ca.MV_POSE_DT.itemsize
STAGE1 = (("rvec_epnp", "rvec0"), ("tvec_epnp", "tvec0"), ("rvec_cam", "rvec"), ("tvec_cam", "tvec"), ("cost_cam0", "cost0"),
          ("cost_cam", "cost"), ("iterations_cam", "iterations"))


@pytest.fixture(scope="module")
def env():
    K, dist = read_camera_yml(CAM_PATH)
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    golden = read_model_file(MODEL_PATH)
    a = stacked_rig_model(golden, 3, 70.0, src=0, ids=[0, 1, 5])
    b = stacked_rig_model(golden, 2, 80.0, src=5, ids=[17, 21])
    two = {"ids": np.array([0, 1, 5, 17, 21], np.int32), "size": 12, "base": np.concatenate([a["base"], b["base"]]),
           "axis": np.concatenate([a["axis"], b["axis"]]), "corners": np.concatenate([a["corners"], b["corners"]])}
    e = {"K": K, "dist": dist, "po": PoseOracle(), "det": det, "golden": golden, "rig": stacked_rig_model(golden, 3, 70.0), "two": two,
         "big": cylinder_model(6, 20)}
    yield e
    det.close()


def _model(m):
    return ca.Model(ids=m["ids"], corners=m["corners"], model_size=m["size"], base=m["base"], axis=m["axis"])


def _camera_set(cameras, poses):
    return ca.CameraSet([ca.make_camera(K, d) for K, d in cameras], poses)


def _batch(env, recs, M, rigs, cs, guard=4):
    """ctag_mv_rig_pose_batch_device on device copies of recs[c][f]; returns the n_frames * n_rigs records and checks the guard
    records before and after them."""
    import torch
    recs = np.asarray(recs)
    n_frames = recs.shape[1]
    d = [torch.from_numpy(np.ascontiguousarray(recs[c]).view(np.uint8).reshape(n_frames, -1)).cuda() for c in range(recs.shape[0])]
    n_out = n_frames * rigs.n_rigs
    out = torch.full(((n_out + 2 * guard) * SZ,), 0xA5, dtype=torch.uint8, device="cuda")
    env["det"].mv_rig_pose_batch_device([t.data_ptr() for t in d], n_frames, M, rigs, cs, out.data_ptr() + guard * SZ)
    env["det"].sync()
    raw = out.cpu().numpy()
    assert (raw[:guard * SZ] == 0xA5).all() and (raw[(guard + n_out) * SZ:] == 0xA5).all(), "bytes written outside n_frames * n_rigs records"
    return raw[guard * SZ:(guard + n_out) * SZ].copy().view(ca.MV_POSE_DT)


def _ring(env, n, seed, centre=None):
    """n cameras with their own intrinsics and coefficient counts (0, 5, 8, 12) on a ring round the rig, 25-50 degrees apart,
    each shifted."""
    rng = np.random.default_rng(seed)
    tc = test_cameras()
    cameras = []
    for c in range(n):
        K = env["K"].copy()
        s = 0.85 + 0.05 * c
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K[0, 0] * s, K[1, 1] * (s + 0.01), K[0, 2] + 11 * c, K[1, 2] - 7 * c
        cameras.append((K, tc[("n_dist0", "n_dist5", "n_dist8", "n_dist12")[c % 4]]))
    step = {2: 50.0, 3: 40.0}.get(n, 360.0 / n)
    angles = [(c - (n - 1) / 2.0) * step + rng.uniform(-5, 5) + 3.0 for c in range(n)]
    centre = env["rig"]["corners"].reshape(-1, 3).astype(np.float64).mean(0) if centre is None else centre
    # about a metre away: the rig stays within |x/z| < 0.15 of every optical axis, where the five undistortion steps converge below
    # float32's pixel rounding for all four coefficient sets (a noise-free pixel then is noise-free for its own camera too)
    return cameras, ms.ring_poses(centre, angles, shifts=rng.normal(0, 1, (n, 3)) * np.array([30.0, 20.0, 40.0]) + np.array([0.0, 0.0, 500.0]))


def _virtual_expected(env, inst, model, camera, rig_of_model, n_rigs, frame=0):
    """Records of one instant whose cameras all are `camera` at the reference: the header by the statement, stage 1 the pose
    oracle's EPnP + PoseBA over the start camera's points, stage 2 its PoseBA over the concatenation from (rvec_cam, tvec_cam)."""
    po, cam_o = env["po"], make_camera(*camera)
    out = np.zeros(n_rigs, ms.MV_POSE_DT)
    for g in range(n_rigs):
        H, per = ms.expected_header(inst, model, rig_of_model, g, frame)
        out[g] = H
        if H["status"] != 0:
            continue
        R, sc = out[g], int(H["start_camera"])
        st, r0, t0 = po.epnp(cam_o, per[sc][1], per[sc][2])
        if st != 0:
            R["status"] = st
            continue
        it1, r1, t1, c0, c1 = po.ba(cam_o, per[sc][1], per[sc][2], r0, t0)
        R["rvec_epnp"], R["tvec_epnp"], R["rvec_cam"], R["tvec_cam"], R["cost_cam0"], R["cost_cam"], R["iterations_cam"] = r0, t0, r1, t1, c0, c1, it1
        R["rvec_start"], R["tvec_start"] = r1, t1
        if int(H["n_points"]) == len(per[sc][1]):
            R["rvec"], R["tvec"], R["cost0"], R["cost"] = r1, t1, c1, c1
            continue
        it, r, t, a, b = po.ba(cam_o, np.concatenate([p[1] for p in per]), np.concatenate([p[2] for p in per]), r1, t1)
        R["iterations"], R["rvec"], R["tvec"], R["cost0"], R["cost"] = it, r, t, a, b
    return out


def test_one_contributing_camera(env):
    """Two cameras, camera 1 away from the reference, only camera 1 sees the rig: stage 1 is camera 1's own rig record, stage 2 is
    not run, and the pose is that record's moved into the reference frame."""
    rig, cam = env["rig"], (env["K"], env["dist"])
    cameras = [cam, cam]
    poses = ms.ring_poses(rig["corners"].reshape(-1, 3).astype(np.float64).mean(0), (0, 35), shifts=[(0, 0, 0), (25, -15, 60)])
    assert not np.any(poses[0][0]) and not np.any(poses[0][1]) and np.any(poses[1][0])
    rng = np.random.default_rng(31)
    M, cs = _model(rig), _camera_set(cameras, poses)
    rigs = ca.Rigs(M, np.zeros(3, np.int32))
    frames = [synth_mv_instant(rng, rig, [[0, 1, 2]], cameras, poses, 0.2, show=lambda c, g, mem: mem if c == 1 else [])[0] for _ in range(3)]
    recs = np.array(frames).T.copy()  # [camera][frame]
    got = _batch(env, recs, M, rigs, cs)
    for f, P in enumerate(got):
        want = compose_rig_poses(env["po"], recs[1][f], make_model_view(rig), make_camera(*cam), np.zeros(3, np.int32), 1)[0]
        assert want["status"] == 0 and P["status"] == 0 and P["start_camera"] == 1 and P["n_cameras"] == 1 and P["n_points"] == want["n_points"]
        for mine, theirs in STAGE1:
            assert P[mine].tobytes() == want[theirs].tobytes(), (f, mine)
        assert P["member_mask"][1].tobytes() == want["member_mask"].tobytes() and not P["member_mask"][0].any()
        assert P["iterations"] == 0 and P["cost0"] == P["cost"] == P["cost_cam"]
        rs, ts = ms.to_reference(P["rvec_cam"], P["tvec_cam"], poses[1])
        print("frame %d: move differs from numpy's by %.3g (rvec) %.3g (tvec)" % (f, np.abs(P["rvec"] - rs).max(), np.abs(P["tvec"] - ts).max()))
        assert np.abs(P["rvec"] - rs).max() <= 1e-12 and np.abs(P["tvec"] - ts).max() <= 1e-12
    assert ms.check_mv_records(got, recs, rig, np.zeros(3, np.int32), 1, cameras, poses) == (3, 3)


# (model index, first position, features, id pattern) per camera: the smallest problem (two cameras x one 4-point feature), the
# last size of the one-wave kernel, the first of the 256-thread kernel, and the bound with a sixth member excluded in the last camera
SPLITS = {8: [[(0, 5, 1, (5, -1))], [(1, 9, 1, (5, -1))], []],
          160: [[(0, 0, 12, (3, 4))], [(1, 0, 8, (3, 4))], []],
          168: [[(0, 0, 12, (3, 4))], [(1, 0, 9, (3, 4))], []],
          # the loop edges of the 256-thread kernel: next to the list switch at 160, and to 256, 512 and 800
          164: [[(0, 0, 12, (3, 4))], [(1, 0, 8, (3, 4)), (2, 5, 1, (5, -1))], []],
          256: [[(0, 0, 20, (3, 4))], [(1, 0, 12, (3, 4))], []],
          260: [[(0, 0, 20, (3, 4))], [(1, 0, 12, (3, 4)), (2, 5, 1, (5, -1))], []],
          512: [[(0, 0, 20, (3, 4)), (1, 0, 20, (3, 4))], [(2, 0, 20, (3, 4)), (3, 0, 4, (3, 4))], []],
          516: [[(0, 0, 20, (3, 4)), (1, 0, 20, (3, 4))], [(2, 0, 20, (3, 4)), (3, 0, 4, (3, 4)), (4, 5, 1, (5, -1))], []],
          796: [[(0, 0, 20, (3, 4)), (1, 0, 20, (3, 4))], [(2, 0, 20, (3, 4)), (3, 0, 20, (3, 4))], [(4, 0, 19, (3, 4)), (5, 5, 1, (5, -1))]],
          800: [[(0, 0, 20, (3, 4)), (1, 0, 20, (3, 4))], [(2, 0, 20, (3, 4)), (3, 0, 20, (3, 4))], [(4, 0, 20, (3, 4)), (5, 3, 2, (3, 4))]]}


def _split_instant(env, rng, camera, split, noise=0.2):
    """One synthetic rig frame of the model_size 20 model whose markers are dealt out to three records."""
    model = env["big"]
    rv, tv = random_pose(rng, model["corners"].reshape(-1, 3).astype(np.float64).mean(0), rot_sigma=0.1)
    recs = np.zeros(3, RESULT_DT)
    for c, deal in enumerate(split):
        for mi, p0, nf, pat in deal:
            X = model["corners"][mi].astype(np.float64)
            pts = ms.project_camera(camera, ZERO, rv, tv, X) + rng.normal(0, noise, (X.shape[0], 2))
            add_marker(recs[c], int(model["ids"][mi]), mi, model, pts, p0, nf, [pat], rng)
    return recs


@pytest.mark.parametrize("cam_name", ["n_dist5", "n_dist8", "n_dist12"])
@pytest.mark.parametrize("n_points", sorted(SPLITS))
def test_virtual_split_is_the_pose_oracle(env, n_points, cam_name):
    """Three cameras with equal intrinsics at the reference: every byte of the record is the pose oracle's."""
    camera = (env["K"], test_cameras()[cam_name])
    model, rig_of_model = env["big"], np.zeros(6, np.int32)
    rng = np.random.default_rng(40 + n_points)
    inst = _split_instant(env, rng, camera, SPLITS[n_points])
    M = _model(model)
    got = _batch(env, inst.reshape(3, 1), M, ca.Rigs(M, rig_of_model), _camera_set([camera] * 3, [ZERO] * 3))[0]
    want = _virtual_expected(env, inst, model, camera, rig_of_model, 1)[0]
    assert want["status"] == 0 and want["n_points"] == n_points and want["n_cameras"] == (2 if n_points < 796 else 3) and want["iterations"] > 0
    assert want["n_excluded"] == (1 if n_points == 800 else 0) and want["start_camera"] == 0
    for k in ca.MV_POSE_DT.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    own = compose_rig_poses(env["po"], inst[0], make_model_view(model), make_camera(*camera), rig_of_model, 1)[0]  # the start camera's own rig record
    for mine, theirs in STAGE1:
        assert got[mine].tobytes() == own[theirs].tobytes(), mine
    assert got["rvec_start"].tobytes() == got["rvec_cam"].tobytes() and got["tvec_start"].tobytes() == got["tvec_cam"].tobytes()


@pytest.mark.parametrize("noise", [0.0, 0.2])
@pytest.mark.parametrize("n_cameras", [2, 3, 8])
def test_real_multi_view_against_the_statement(env, n_cameras, noise):
    """Cameras with their own poses, intrinsics and coefficient counts, two rigs: every record against the statement and scipy's
    minimum (check_mv_records); noise-free input returns the planted poses within the same bars."""
    model, rig_of_model = env["two"], np.array([0, 0, 0, 1, 1], np.int32)
    cameras, poses = _ring(env, n_cameras, 50 + n_cameras)
    rng = np.random.default_rng(60 + n_cameras)
    frames, planted = [], []
    for f in range(4):
        r, truth = synth_mv_instant(rng, model, [[0, 1, 2], [3, 4]], cameras, poses, noise, feats=(2, 4) if n_cameras == 8 else (2, 5))
        frames.append(r)
        planted.append(truth)
    recs = np.array(frames).T.copy()
    M = _model(model)
    got = _batch(env, recs, M, ca.Rigs(M, rig_of_model), _camera_set(cameras, poses))
    assert (got["status"] == 0).all() and (got["n_points"] >= 16).all() and (got["n_cameras"] == n_cameras).all() and (got["iterations"] > 0).all()
    ok, checked = ms.check_mv_records(got, recs, model, rig_of_model, 2, cameras, poses, planted=planted if noise == 0.0 else None)
    print(ms.last_stats)
    assert ok == checked == 8  # no OK record is left out of the minimum check


def test_rules_and_statuses(env):
    """The start camera's tie, a failed camera beside two good ones, all cameras failed, duplicates and rejected members per
    camera, TOO_FEW; and a planar model: DEGENERATE with zero pose fields."""
    rig, rig_of_model = env["rig"], np.zeros(3, np.int32)
    cameras, poses = _ring(env, 3, 71)
    rng = np.random.default_rng(72)
    full = lambda **kw: synth_mv_instant(rng, rig, [[0, 1, 2]], cameras, poses, 0.2, **kw)[0]  # noqa: E731
    tie = full(feats=(3, 3), show=lambda c, g, mem: mem if c > 0 else mem[:1])
    failed = full()
    failed[1]["status"] = 2  # CTAG_NO_FEATURE
    dark = full()
    dark["status"] = [1, 2, 2]
    dup = full(feats=(2, 3))
    dup[0]["markers"][3] = dup[0]["markers"][1]  # camera 0: marker 1 once more
    dup[0]["n_markers"] = 4
    k = int(dup[1]["markers"][2]["first_feature"])
    dup[1]["features"][k]["pos"] = 12  # camera 1: a member whose feature lies outside the model
    few = full(show=lambda c, g, mem: mem[:1] if c == 2 else [])
    few[2]["markers"][0]["n_features"] = 0
    recs = np.array([tie, failed, dark, dup, few]).T.copy()
    M = _model(rig)
    rigs, cs = ca.Rigs(M, rig_of_model), _camera_set(cameras, poses)
    got = _batch(env, recs, M, rigs, cs)
    assert [int(s) for s in got["status"]] == [0, 0, ms.NOT_SEEN, 0, ms.TOO_FEW]
    assert list(got[0]["points_of_camera"][:3]) == [24, 72, 72] and got[0]["start_camera"] == 1
    assert got[1]["points_of_camera"][1] == 0 and got[1]["n_cameras"] == 2 and not got[1]["member_mask"][1].any()
    assert got[3]["n_excluded"] == 2 and got[3]["n_members"] == 8 and got[3]["n_cameras"] == 3
    assert got[4]["n_members"] == 1 and got[4]["n_points"] == 0 and got[4]["start_camera"] == 0
    assert ms.check_mv_records(got, recs, rig, rig_of_model, 1, cameras, poses) == (3, 3)
    flat = planar_model(rig)
    got = _batch(env, recs, _model(flat), rigs, cs)
    assert [int(s) for s in got["status"]] == [ms.DEGENERATE, ms.DEGENERATE, ms.NOT_SEEN, ms.DEGENERATE, ms.TOO_FEW]
    assert ms.check_mv_records(got, recs, flat, rig_of_model, 1, cameras, poses, degenerate=lambda f, g: True) == (0, 0)


def test_batch_equals_single_instant_calls_and_the_raw_abi(env):
    model, rig_of_model = env["two"], np.array([0, 0, 0, 1, 1], np.int32)
    cameras, poses = _ring(env, 3, 81)
    rng = np.random.default_rng(82)
    frames = [synth_mv_instant(rng, model, [[0, 1, 2], [3, 4]], cameras, poses, 0.2, show=lambda c, g, mem: [m for m in mem if rng.random() < 0.7])[0]
              for _ in range(12)]
    frames[5]["status"] = 1
    frames[7][2]["status"] = 2
    recs = np.array(frames).T.copy()
    M = _model(model)
    rigs, cs = ca.Rigs(M, rig_of_model), _camera_set(cameras, poses)
    got = _batch(env, recs, M, rigs, cs, guard=16)
    assert {0, ms.NOT_SEEN} <= set(int(s) for s in got["status"])
    L = capi.load_library()
    for f in range(12):
        one = env["det"].estimate_mv_rig_pose(recs[:, f], M, rigs, cs)
        one["frame"] = f  # the single-instant call numbers its frame 0
        assert one.tobytes() == got[2 * f:2 * f + 2].tobytes(), f
        raw = np.zeros(2, ca.MV_POSE_DT)
        inst = np.ascontiguousarray(recs[:, f])
        assert L.ctag_estimate_mv_rig_pose(env["det"].h, inst.ctypes.data, M.m, rigs.r, cs.s, raw.ctypes.data) == 0
        raw["frame"] = f
        assert raw.tobytes() == one.tobytes()


def test_more_items_than_either_grid(env):
    """About 4800 eight-point items and 390 items of 168 points in one call, failed and pointless instants among them: both
    solve kernels walk their list with a stride and reuse their LDS image after items that leave early.  Equal cameras at the
    reference, so every record is the pose oracle's."""
    camera = (env["K"], env["dist"])
    model, rig_of_model = env["big"], np.zeros(6, np.int32)
    rng = np.random.default_rng(91)
    kinds = []
    for i in range(30 + 13):
        inst = _split_instant(env, rng, camera, SPLITS[8 if i < 30 else 168])[:2]
        if i % 10 == 3:
            inst["status"] = 1                       # NOT_SEEN
        elif i % 10 == 6:
            inst[0]["markers"][0]["n_features"] = 0  # camera 1 starts and is alone: no stage 2
            if i % 20 == 16:
                inst[1]["markers"][0]["n_features"] = 0  # TOO_FEW
        elif i % 10 == 8:
            inst[1]["status"] = 2                    # camera 0 alone
        kinds.append((inst, _virtual_expected(env, inst, model, camera, rig_of_model, 1)[0]))
    order = [f % 30 for f in range(4800)] + [30 + f % 13 for f in range(390)]
    order = [order[i] for i in np.random.default_rng(92).permutation(len(order))]
    recs = np.array([kinds[k][0] for k in order]).T.copy()
    want = np.array([kinds[k][1] for k in order])
    want["frame"] = np.arange(len(order))
    assert {0, ms.NOT_SEEN, ms.TOO_FEW} <= set(int(s) for s in want["status"])
    solved = want["status"] != ms.NOT_SEEN
    solved &= want["status"] != ms.TOO_FEW
    assert (solved & (want["n_points"] <= 160)).sum() > 4096 and (solved & (want["n_points"] > 160)).sum() > 256  # more than either grid
    assert (want["iterations"] > 0).sum() > 3000 and ((want["status"] == 0) & (want["iterations"] == 0)).sum() > 500
    M = _model(model)
    got = _batch(env, recs, M, ca.Rigs(M, rig_of_model), _camera_set([camera] * 2, [ZERO] * 2))
    bad = [f for f in range(len(order)) if got[f].tobytes() != want[f].tobytes()]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])


def test_argument_rejections(env):
    rig = env["rig"]
    cam = ca.make_camera(env["K"], env["dist"])
    M = _model(rig)
    rigs = ca.Rigs(M, np.zeros(3, np.int32))
    for n in (0, 9):
        with pytest.raises(ca.CtagError) as e:
            ca.CameraSet([cam] * n, [ZERO] * n)
        assert e.value.status == capi.ERR_ARG
    tilted = ca.make_camera(env["K"], np.r_[test_cameras()["n_dist12"], 0.01, 0.0])
    with pytest.raises(ca.CtagError) as e:
        ca.CameraSet([cam, tilted], [ZERO] * 2)
    assert e.value.status == capi.ERR_UNSUPPORTED
    with pytest.raises(ca.CtagError) as e:
        ca.CameraSet([cam, cam], [ZERO, ((0, 0, 0), (0, np.nan, 0))])
    assert e.value.status == capi.ERR_ARG
    import torch
    cs = ca.CameraSet([cam, cam], [ZERO, ((0, 0.4, 0), (100, 0, 0))])
    d = torch.zeros(2 * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * SZ,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(ca.CtagError) as e:  # a null entry in the pointer array
        env["det"].mv_rig_pose_batch_device([d.data_ptr(), None], 1, M, rigs, cs, out.data_ptr())
    assert e.value.status == capi.ERR_ARG
    other = _model(env["two"])
    with pytest.raises(ca.CtagError) as e:  # a rig set made for a model of another size
        env["det"].mv_rig_pose_batch_device([d.data_ptr(), d.data_ptr() + RESULT_DT.itemsize], 1, other, rigs, cs, out.data_ptr())
    assert e.value.status == capi.ERR_ARG
    env["det"].sync()
    assert (out.cpu().numpy() == 0xA5).all()
    env["det"].mv_rig_pose_batch_device([d.data_ptr(), d.data_ptr() + RESULT_DT.itemsize], 0, M, rigs, cs, out.data_ptr())  # no frames: nothing written
    env["det"].sync()
    assert (out.cpu().numpy() == 0xA5).all()


DRIVER = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "CylinderTag.h"
#include "ctag_io.h"
int main(int argc, char** argv) {  // marker bmp model camera n_cameras rig_of_model...
    try {
        CylinderTag tag(argv[1]);
        const ctag_host::GrayImage g = ctag_host::read_bmp_gray(argv[2]);
        std::vector<MarkerInfo> markers;
        tag.detect(ctag_host::Mat(g.rows, g.cols, g.px.data()), markers, 5, true, 5);
        std::vector<ModelInfo> model;
        CamInfo cam;
        tag.loadModel(argv[3], model);
        tag.loadCamera(argv[4], cam);
        const int nc = std::stoi(argv[5]);
        std::vector<int> rig;
        for (int i = 6; i < argc; i++) rig.push_back(std::stoi(argv[i]));
        // camera c sees the first n - c markers, from a pose a little off the reference
        std::vector<std::vector<MarkerInfo>> lists;
        std::vector<CamInfo> cams;
        std::vector<ViewPose> views;
        for (int c = 0; c < nc; c++) {
            lists.emplace_back(markers.begin(), markers.end() - (c < (int)markers.size() ? c : 0));
            cams.push_back(cam);
            ViewPose v;
            v.rvec[1] = 0.002 * c;
            v.tvec[0] = 0.5 * c;
            views.push_back(v);
        }
        std::vector<RigPoseInfo> pose;
        tag.estimateMultiViewRigPose(lists, model, rig, cams, views, pose);
        for (const RigPoseInfo& p : pose) {
            std::printf("rig %d", p.rigID);
            for (int i = 0; i < 3; i++) std::printf(" %.17g", p.rvec[i]);
            for (int i = 0; i < 3; i++) std::printf(" %.17g", p.tvec[i]);
            std::printf(" members");
            for (const auto& m : p.viewMembers) std::printf(" %d:%d", m.first, m.second);
            std::printf("\n");
        }
    } catch (const std::string& e) {
        std::printf("error %s", e.c_str());
        return 1;
    }
    return 0;
}
"""


def test_cpp_class_estimate_multi_view_rig_pose_equals_the_c_abi(env, tmp_path):
    build = os.path.join(ROOT, "cylindertag_amd", "_build")
    exe = str(tmp_path / "mv_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-x", "c++", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cylindertag_amd", "csrc"),
                    "-o", exe, "-", "-L" + build, "-lcylindertag", "-lctag_hip", "-Wl,-rpath," + build], input=DRIVER.encode(), check=True, timeout=300)
    det = env["det"]
    M, cam = ca.Model(MODEL_PATH), ca.load_camera(CAM_PATH)
    res = det.detect(read_bmp_gray(os.path.join(GOLDEN, "test.bmp")), 5, True, 5)
    nm = int(res["n_markers"])
    assert nm == 5
    for nc, rig_of_model in ((2, [0, 0, 0, 0, 0, 0]), (3, [1, -1, 0, 1, -1, 0]), (1, [0, 1, 2, 3, 4, 5])):
        out = subprocess.check_output([exe, os.path.join(GOLDEN, "CTag_2f12c.marker"), os.path.join(GOLDEN, "test.bmp"), MODEL_PATH, CAM_PATH, str(nc)] +
                                      [str(v) for v in rig_of_model], timeout=120).decode()
        recs = np.zeros(nc, ca.RESULT_DT)
        for c in range(nc):
            recs[c] = res
            recs[c]["n_markers"] = nm - c  # the features of the dropped markers stay in the record, unused
        cs = ca.CameraSet([cam] * nc, [((0, 0.002 * c, 0), (0.5 * c, 0, 0)) for c in range(nc)])
        got_recs = det.estimate_mv_rig_pose(recs, M, ca.Rigs(M, rig_of_model), cs)
        want = []
        for R in got_recs:
            if R["status"] == ca.capi.POSE_NOT_SEEN:
                continue  # erased
            assert R["status"] == 0
            mem = ["%d:%d" % (c, k) for c in range(nc) for k in range(100) if (int(R["member_mask"][c][k >> 5]) >> (k & 31)) & 1]
            want.append("rig %d %s %s members %s" % (R["rig"], " ".join("%.17g" % v for v in R["rvec"]), " ".join("%.17g" % v for v in R["tvec"]), " ".join(mem)))
        got = [l.strip() for l in out.splitlines() if l.startswith("rig ")]
        assert [" ".join(l.split()) for l in got] == [" ".join(l.split()) for l in want] and got, (rig_of_model, out)
