"""GPU parity of the rig pose (k_rig_pose.hip through ctag_rig_pose_batch_device / ctag_estimate_rig_pose of include/ctag_pose.h):
every record byte-identical to the rig composition of tests/rig_testlib.py (the unmodified pose oracle's correspondence builder,
EPnP and PoseBA over the members' concatenated points), on test.bmp, on synthetic record batches and at the 800-point bound."""
import os
import subprocess

import numpy as np
import pytest

import cylindertag_amd as ca
import testkit as tk
from ctag_testlib import GOLDEN, ROOT, RESULT_DT, read_bmp_gray
from pose_testlib import PoseOracle, make_camera, make_model_view, project, read_camera_yml, read_model_file
from rig_testlib import (add_marker, compose_rig_poses, cylinder_model, random_pose, rot_err_deg, stacked_rig_model, synth_rig_frame)

pytestmark = pytest.mark.gpu

MODEL_PATH = os.path.join(GOLDEN, "CTag_2f12c.model")
CAM_PATH = os.path.join(GOLDEN, "cameraParams.yml")
POSE_FIELDS = ("n_points", "iterations", "rvec", "tvec", "rvec0", "tvec0", "cost0", "cost")


@pytest.fixture(scope="module")
def env():
    K, dist = read_camera_yml(CAM_PATH)
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    e = {"K": K, "dist": dist, "model": read_model_file(MODEL_PATH), "cam_o": make_camera(K, dist), "po": PoseOracle(), "det": det,
         "M": ca.Model(MODEL_PATH), "cam": ca.load_camera(CAM_PATH), "res": det.detect(read_bmp_gray(os.path.join(GOLDEN, "test.bmp")), 5, True, 5)}
    e["mv"] = make_model_view(e["model"])
    yield e
    det.close()


def _model(m):
    return ca.Model(ids=m["ids"], corners=m["corners"], model_size=m["size"], base=m["base"], axis=m["axis"])


def _batch(env, recs, M, rigs, guard=4):
    """ctag_rig_pose_batch_device on device copies of recs; returns the n_frames*n_rigs records, checking the guard records after them."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1)).cuda()
    n_out = len(recs) * rigs.n_rigs
    out = torch.full(((n_out + guard) * ca.RIG_POSE_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    env["det"].rig_pose_batch_device(d.data_ptr(), len(recs), M, rigs, env["cam"], out.data_ptr())
    env["det"].sync()
    raw = out.cpu().numpy()
    assert (raw[n_out * ca.RIG_POSE_DT.itemsize:] == 0xA5).all(), "bytes written past n_frames * n_rigs records"
    return raw[:n_out * ca.RIG_POSE_DT.itemsize].view(ca.RIG_POSE_DT)


def _want(env, recs, mv, rig_of_model, n_rigs):
    return np.concatenate([compose_rig_poses(env["po"], recs[f], mv, env["cam_o"], rig_of_model, n_rigs, f) for f in range(len(recs))])


def test_reference_scene_each_model_its_own_rig(env):
    """test.bmp: with every model a rig of its own, each seen rig carries that marker's ctag_pose_rec pose bytes; model 21 is not seen."""
    det, M, res = env["det"], env["M"], env["res"]
    rigs = ca.Rigs(M, np.arange(6))
    got = det.estimate_rig_pose(res, M, rigs, env["cam"])
    assert got.tobytes() == compose_rig_poses(env["po"], res, env["mv"], env["cam_o"], np.arange(6), 6).tobytes()
    poses = det.estimate_pose(res, M, env["cam"])
    seen = set()
    for k, p in enumerate(poses):
        if p["status"] != ca.capi.POSE_OK:
            continue
        g = int(p["model_index"])
        seen.add(g)
        R = got[g]
        assert R["status"] == 0 and R["n_members"] == 1 and R["n_excluded"] == 0 and R["member_mask"][0] == 1 << k
        for f in POSE_FIELDS:
            assert R[f].tobytes() == p[f].tobytes(), (g, f)
    assert seen == {0, 1, 2, 3, 5}
    assert int(env["model"]["ids"][4]) == 21 and got[4]["status"] == ca.capi.POSE_NOT_SEEN and got[4]["n_members"] == 0


def test_reference_scene_all_models_one_rig(env):
    det, M, res = env["det"], env["M"], env["res"]
    rigs = ca.Rigs(M, np.zeros(6, np.int32))
    got = det.estimate_rig_pose(res, M, rigs, env["cam"])
    want = compose_rig_poses(env["po"], res, env["mv"], env["cam_o"], np.zeros(6, np.int32), 1)
    assert got.tobytes() == want.tobytes()
    assert got[0]["status"] == 0 and got[0]["n_members"] == 5 and got[0]["n_points"] == sum(
        int(p["n_points"]) for p in det.estimate_pose(res, M, env["cam"]))


def _synthetic_batch(env, n_frames, seed):
    """Six models: models 0-2 three stacked copies of CTag_2f12c's model 0 (rig 0), 3-4 two stacked copies of its model 2 (rig 1),
    5 in no rig.  Frames mix both rigs, markers outside the rigs, unknown ids, duplicated markers, members the builder rejects,
    members without points, frames that are not CTAG_OK and empty frames."""
    K, dist = env["K"], env["dist"]
    a = stacked_rig_model(env["model"], 3, 70.0, src=0, ids=[0, 1, 5])
    b = stacked_rig_model(env["model"], 2, 80.0, src=2, ids=[17, 21])
    model = {"ids": np.array([0, 1, 5, 17, 21, 23], np.int32), "size": 12, "base": np.concatenate([a["base"], b["base"], env["model"]["base"][4:5]]),
             "axis": np.concatenate([a["axis"], b["axis"], env["model"]["axis"][4:5]]),
             "corners": np.concatenate([a["corners"], b["corners"], env["model"]["corners"][4:5]])}
    rig_of_model = np.array([0, 0, 0, 1, 1, -1], np.int32)
    rng = np.random.default_rng(seed)
    patterns = [(3, 3), (3, 4), (2, 4), (1, 4), (5, -1), (0, 0), (6, 7), (7, 4)]
    recs = np.zeros(n_frames, RESULT_DT)
    truth = []
    for f in range(n_frames):
        kind = f % 8
        show = lambda g, mem: [m for m in mem if rng.random() < 0.75] or [mem[0]]  # noqa: E731
        r, tr = synth_rig_frame(rng, model, [[0, 1, 2], [3, 4]], K, dist, 0.2, feats=(1, 6),
                                patterns=patterns if kind == 7 else [(3, 4)], show=show)
        if kind == 3:  # the model outside every rig, and an unknown id
            rv, tv = random_pose(rng, model["corners"][5].mean(0))
            add_marker(r, 23, 5, model, project(K, dist, rv, tv, model["corners"][5].astype(np.float64)), 2, 3, [(3, 4)], rng)
            add_marker(r, 40, -1, model, project(K, dist, rv, tv, model["corners"][5].astype(np.float64)), 0, 2, [(3, 4)], rng)
        elif kind == 4 and r["n_markers"] > 0:  # a duplicate of an earlier marker (same id, same features)
            m = int(r["n_markers"])
            r["markers"][m] = r["markers"][int(rng.integers(0, m))]
            r["n_markers"] = m + 1
        elif kind == 5 and r["n_markers"] > 0:  # a member whose feature lies outside the model
            M = r["markers"][int(rng.integers(0, int(r["n_markers"])))]
            r["features"][int(M["first_feature"]) + int(rng.integers(0, int(M["n_features"])))]["pos"] = 12
        elif kind == 6 and r["n_markers"] > 0:  # a member without points (no features): n < 4 when it is the rig's only member
            r["markers"][int(rng.integers(0, int(r["n_markers"])))]["n_features"] = 0
        elif kind == 1:
            r["status"] = 1
        elif kind == 2:
            r["n_markers"] = 0
        recs[f] = r
        truth.append(tr)
    return model, rig_of_model, recs, truth


def test_synthetic_batch_parity(env):
    model, rig_of_model, recs, truth = _synthetic_batch(env, 512, 11)
    M, mv = _model(model), make_model_view(model)
    rigs = ca.Rigs(M, rig_of_model)
    got = _batch(env, recs, M, rigs)
    want = _want(env, recs, mv, rig_of_model, 2)
    for f in range(len(recs)):
        assert got[2 * f:2 * f + 2].tobytes() == want[2 * f:2 * f + 2].tobytes(), "frame %d" % f
    st = got["status"]
    assert {0, 2, 5} <= set(int(s) for s in st), set(st)  # OK, TOO_FEW and NOT_SEEN all occur
    assert (got["n_excluded"] > 0).sum() >= 32 and (got["n_members"] >= 2).sum() >= 200
    assert all(got[2 * f]["status"] == got[2 * f + 1]["status"] == 5 for f in range(1, 512, 8))  # not CTAG_OK
    both = [f for f in range(0, 512, 8) if got[2 * f]["status"] == 0 and got[2 * f + 1]["status"] == 0]
    assert len(both) >= 48  # two rigs posed in one frame
    err_t, err_r = [], []
    for f in range(0, 512, 8):  # plain frames: the planted poses come back
        for g in range(2):
            R = got[2 * f + g]
            if R["status"] == 0 and R["n_points"] >= 32:
                err_r.append(rot_err_deg(R["rvec"], truth[f][g][0]))
                err_t.append(np.linalg.norm(R["tvec"] - truth[f][g][1]))
    assert len(err_t) >= 80 and np.median(err_r) < 0.1 and np.median(err_t) < 1.0, (np.median(err_r), np.median(err_t))


@pytest.mark.parametrize("name", ["n_dist8", "n_dist12"])
def test_synthetic_batch_parity_rational_and_thin_prism_cameras(env, name):
    """The synthetic batch under the 8- and 12-coefficient cameras of pose_testlib.test_cameras(): k_rig_pose.hip shares
    undistort_normalised and pose_solve with k_pose.hip, whose k[5..11] terms the golden camera leaves at zero."""
    from pose_testlib import test_cameras
    dist = test_cameras()[name]
    e = dict(env, dist=dist, cam=ca.make_camera(env["K"], dist), cam_o=make_camera(env["K"], dist))
    assert e["cam"].n_dist == len(dist) == int(name[6:]) and e["cam"].dist[len(dist) - 1] != 0
    model, rig_of_model, recs, _ = _synthetic_batch(e, 64, 13)
    M, mv = _model(model), make_model_view(model)
    got = _batch(e, recs, M, ca.Rigs(M, rig_of_model))
    want = _want(e, recs, mv, rig_of_model, 2)
    for f in range(len(recs)):
        assert got[2 * f:2 * f + 2].tobytes() == want[2 * f:2 * f + 2].tobytes(), "frame %d" % f
    assert (got["status"] == 0).sum() >= 40 and (got["n_members"] >= 2).sum() >= 20
    # and not the golden camera's records: the extra terms reach the kernel
    plain = _batch(env, recs, M, ca.Rigs(M, rig_of_model))
    ok = (got["status"] == 0) & (plain["status"] == 0)
    assert np.median(np.abs(got["tvec"][ok] - plain["tvec"][ok]).max(axis=1)) > 1e-3  # millimetres


def test_batch_equals_single_frame_calls(env):
    model, rig_of_model, recs, _ = _synthetic_batch(env, 48, 12)
    M = _model(model)
    rigs = ca.Rigs(M, rig_of_model)
    got = _batch(env, recs, M, rigs, guard=16)
    for f in range(len(recs)):
        one = env["det"].estimate_rig_pose(recs[f], M, rigs, env["cam"])
        one["frame"] = f  # the single-frame call numbers its frame 0
        assert one.tobytes() == got[2 * f:2 * f + 2].tobytes(), f
    other = _model({k: (v[:5] if k != "size" else v) for k, v in model.items()})
    with pytest.raises(ca.CtagError):  # a rig set made for a model of another size
        env["det"].estimate_rig_pose(recs[0], other, rigs, env["cam"])


def test_upper_bound_800_points(env):
    """model_size 20 (160 points per marker): five members of 20 inner features fill a frame's 100 features, n = 800; a hand-built
    frame whose six markers share one feature range excludes the sixth at the bound; members of 160 and 168 points on the two paths."""
    K, dist = env["K"], env["dist"]
    model = cylinder_model(6, 20)
    M, mv = _model(model), make_model_view(model)
    rig_of_model = np.zeros(6, np.int32)
    rigs = ca.Rigs(M, rig_of_model)
    rng = np.random.default_rng(5)
    recs = np.zeros(4, RESULT_DT)
    rv, tv = random_pose(rng, model["corners"].reshape(-1, 3).astype(np.float64).mean(0), rot_sigma=0.1)
    pts = [project(K, dist, rv, tv, model["corners"][m].astype(np.float64)) + rng.normal(0, 0.2, (160, 2)) for m in range(6)]
    for m in range(5):
        add_marker(recs[0], m, m, model, pts[m], 0, 20, [(3, 4)], rng)
    add_marker(recs[1], 0, 0, model, pts[0], 0, 20, [(3, 4)], rng)
    for m in range(1, 6):  # overlapping feature ranges: every marker points at features 0..19
        recs[1]["markers"][m] = (m, 0, 20, 20)
    recs[1]["n_markers"] = 6
    add_marker(recs[2], 2, 2, model, pts[2], 0, 20, [(3, 4)], rng)          # 160 points: the one-wave path
    add_marker(recs[3], 1, 1, model, pts[1], 0, 20, [(3, 4)], rng)          # 160 + 8 points: the 256-thread path
    add_marker(recs[3], 4, 4, model, pts[4], 7, 1, [(3, 4)], rng)
    got = _batch(env, recs, M, rigs)
    want = _want(env, recs, mv, rig_of_model, 1)
    assert got.tobytes() == want.tobytes()
    assert [int(v) for v in got["n_points"]] == [800, 800, 160, 168] and list(got["status"]) == [0, 0, 0, 0]
    assert got[1]["n_members"] == 5 and got[1]["n_excluded"] == 1 and got[1]["member_mask"][0] == 0x1F
    # a thin cylinder (radius 25 mm) 1.5 m away at 0.2 px noise
    assert rot_err_deg(got[0]["rvec"], rv) < 0.5 and np.linalg.norm(got[0]["tvec"] - tv) < 7.5  # mm: 0.5 % of the distance


DRIVER = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "CylinderTag.h"
#include "ctag_io.h"
int main(int argc, char** argv) {  // marker bmp model camera rig_of_model...
    try {
        CylinderTag tag(argv[1]);
        const ctag_host::GrayImage g = ctag_host::read_bmp_gray(argv[2]);
        std::vector<MarkerInfo> markers;
        tag.detect(ctag_host::Mat(g.rows, g.cols, g.px.data()), markers, 5, true, 5);
        std::vector<ModelInfo> model;
        CamInfo cam;
        tag.loadModel(argv[3], model);
        tag.loadCamera(argv[4], cam);
        std::vector<int> rig;
        for (int i = 5; i < argc; i++) rig.push_back(std::stoi(argv[i]));
        std::vector<RigPoseInfo> pose;
        tag.estimateRigPose(markers, model, rig, cam, pose);
        for (const RigPoseInfo& p : pose) {
            std::printf("rig %d", p.rigID);
            for (int i = 0; i < 3; i++) std::printf(" %.17g", p.rvec[i]);
            for (int i = 0; i < 3; i++) std::printf(" %.17g", p.tvec[i]);
            std::printf(" members");
            for (int k : p.members) std::printf(" %d", k);
            std::printf("\n");
        }
    } catch (const std::string& e) {
        std::printf("error %s", e.c_str());
        return 1;
    }
    return 0;
}
"""


def test_cpp_class_estimate_rig_pose_equals_the_c_abi(env, tmp_path):
    build = os.path.join(ROOT, "cylindertag_amd", "_build")
    exe = str(tmp_path / "rig_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-x", "c++", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cylindertag_amd", "csrc"),
                    "-o", exe, "-", "-L" + build, "-lcylindertag", "-lctag_hip", "-Wl,-rpath," + build], input=DRIVER.encode(), check=True, timeout=300)
    det, M, res = env["det"], env["M"], env["res"]
    for rig_of_model in ([0, 1, 2, 3, 4, 5], [0, 0, 0, 0, 0, 0], [1, -1, 0, 1, -1, 0]):
        out = subprocess.check_output([exe, os.path.join(GOLDEN, "CTag_2f12c.marker"), os.path.join(GOLDEN, "test.bmp"), MODEL_PATH, CAM_PATH] +
                                      [str(v) for v in rig_of_model], timeout=120).decode()
        recs = det.estimate_rig_pose(res, M, ca.Rigs(M, rig_of_model), env["cam"])
        want = []
        for R in recs:
            if R["status"] == ca.capi.POSE_NOT_SEEN:
                continue  # erased
            assert R["status"] == 0
            mem = [k for k in range(100) if (int(R["member_mask"][k >> 5]) >> (k & 31)) & 1]
            want.append("rig %d %s %s members %s" % (R["rig"], " ".join("%.17g" % v for v in R["rvec"]), " ".join("%.17g" % v for v in R["tvec"]),
                                                      " ".join(str(k) for k in mem)))
        got = [l.strip() for l in out.splitlines() if l.startswith("rig ")]
        assert [" ".join(l.split()) for l in got] == [" ".join(l.split()) for l in want], (rig_of_model, out)
        assert len(got) == len(set(v for v in rig_of_model if v >= 0) - ({4} if rig_of_model == [0, 1, 2, 3, 4, 5] else set()))
