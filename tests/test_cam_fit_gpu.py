"""GPU tests of the camera set fit through the public calls (Detector.fit_camera_set / fit_camera_set_device): every case of
tests/cam_fit_shapes.py is fitted once and the result is held to rules 1-6 of include/ctag_pose.h and to the independent statement's
joint minimum (tests/cam_fit_statement.py)."""
import ctypes as C

import numpy as np
import pytest

import cam_fit_shapes as sh
import cam_fit_statement as cf
import cylindertag_amd as ca
from cam_fit_testlib import TIGHT, Detectors, device_mv_poses, device_rig_records, input_of, observation_cost, state_of
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu
SMALL = [n for n in sh.NAMES if not n.startswith("e")]   # the joint minimum of (e) is (a)'s, 572 records of it


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "fit": {}}
    yield e
    e["dets"].close()


def _fit(env, name, **kw):
    """The case fitted once (host entry) and shared: (case, detector, Model, Rigs, cameras, (CameraSet | None, stat, cam_stats))."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in env["fit"]:
        b = sh.case(name)
        det = env["dets"].of(b)
        M, rigs, cams = input_of(b)
        opts = dict(min_items=b["min_items"], rel_tol=TIGHT)
        opts.update(kw)
        env["fit"][key] = (b, det, M, rigs, cams, det.fit_camera_set(b["recs"], M, rigs, cams, **opts))
    return env["fit"][key]


def _mv_under(b, det, M, rigs, placed, cam_stats):
    """The public multi-view call on the placed cameras under the set cam_stats describes."""
    cs = ca.CameraSet([ca.make_camera(*b["cameras"][c]) for c in placed], [(cam_stats[c]["rvec"], cam_stats[c]["tvec"]) for c in placed])
    return device_mv_poses(det, np.ascontiguousarray(b["recs"][placed]), M, rigs, cs)


@pytest.mark.parametrize("name", sh.NAMES)
def test_result_obeys_the_rules(env, name):
    """Rules 2-3 from the statistics: anchor, tree, counts, unplaced cameras and their status; the observation set; stat.cost and
    cost_init are the sums of the public multi-view call's record costs under the returned and the initial set, byte for byte."""
    b, det, M, rigs, cams, (cs, stat, cam_stats) = _fit(env, name)
    A = sh.assembled(name)
    init, placed = A["init"], A["init"]["placed"]
    n_cam = len(b["cameras"])
    assert stat["status"] == 0 and stat["anchor"] == init["anchor"] and stat["n_placed"] == len(placed) and stat["n_unplaced"] == n_cam - len(placed)
    assert stat["reserved"] == 0 and (cs is None) == (len(placed) < n_cam)
    for c in range(n_cam):
        st = cam_stats[c]
        assert st["reserved"] == 0
        if c not in placed or c == init["anchor"]:
            assert st["status"] == (0 if c in placed else capi.POSE_NOT_SEEN) and st["parent"] == -1 and st["n_items_with_parent"] == 0
            assert not st["rvec"].any() and not st["tvec"].any()
        else:
            assert st["status"] == 0 and st["parent"] == init["parent"][c] and st["n_items_with_parent"] == init["n_with_parent"][c]
    mvp = _mv_under(b, det, M, rigs, placed, cam_stats)
    stat0, cam_stats0 = _fit(env, name, max_rounds=0)[5][1:]
    mvp0 = _mv_under(b, det, M, rigs, placed, cam_stats0)
    items = [w for w in range(len(mvp0)) if mvp0[w]["status"] == 0 and mvp0[w]["n_cameras"] >= 2]
    O = cf.Observations(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], placed, ok_of=lambda w: mvp0[w]["status"] == 0)
    assert O.items == items and stat["n_records"] == len(items) and stat["n_points"] == sum(O.n_points)
    for k, c in enumerate(placed):
        assert cam_stats[c]["n_records"] == sum(1 for pts in O.points_of_camera if pts[k]) and cam_stats[c]["n_points"] == sum(pts[k] for pts in O.points_of_camera)
    assert 1 <= stat["rounds"] <= 30 and stat["cost"] <= stat["cost_init"]
    assert stat["cost_init"] == observation_cost(mvp0, items) == stat0["cost_init"] == stat0["cost"] and stat0["rounds"] == 0
    assert stat["cost"] == observation_cost(mvp, items), "stat.cost is not the cost of the returned set"
    assert stat["rms_px"] == np.sqrt(2.0 * stat["cost"] / stat["n_points"])
    print("%s: %d records, %d rounds, cost %.6g -> %.6g, rms %.3g px, lambda %.3g" % (name, len(items), stat["rounds"], stat["cost_init"], stat["cost"], stat["rms_px"],
                                                                                       stat["lambda"]))


@pytest.mark.parametrize("name", sh.NAMES)
def test_max_rounds_0_returns_the_initial_assembly(env, name):
    """Rule 2 as the statement has it, on the device's own per-camera rig records (rule 1: whichever minimum EPnP + PoseBA ended in; the
    statement's minimum from the planted start is printed beside it)."""
    b, det, M, rigs, cams, (_, stat0, cam_stats0) = _fit(env, name, max_rounds=0)
    A = sh.assembled(name)
    rr = device_rig_records(det, b, M, rigs, cams)
    init = cf.initial_assembly(rr, len(cams), b["recs"].shape[1] * b["n_rigs"], b["min_items"])
    assert init["anchor"] == A["init"]["anchor"] and init["parent"] == A["init"]["parent"] and (init["counts"] == A["init"]["counts"]).all()
    placed = init["placed"]
    got = state_of(cam_stats0, placed)
    d = sh.set_distance(*got, np.array([init["T"][c][0] for c in placed]), np.array([init["T"][c][1] for c in placed]))
    far = sh.set_distance(*got, A["R0"], A["t0"])
    print("%s: the device's initial assembly lies %.2e rad %.2e from rule 2 on its own rig records, %.2e rad %.2e from the statement's minima" % ((name,) + d + far))
    assert sh.within_bar(d)


@pytest.mark.parametrize("name", SMALL)
def test_poses_against_the_joint_minimum(env, name):
    """Every placed camera within cf.POSE_BAR of the statement's joint minimum over camera poses and rig poses."""
    cam_stats = _fit(env, name)[5][2]
    ref = sh.joint_reference(name)
    d = sh.set_distance(*state_of(cam_stats, sh.assembled(name)["init"]["placed"]), ref["R"], ref["t"])
    print("%s: %.2e rad %.2e from the joint minimum (bar %.2e %.2e)" % ((name,) + d + cf.POSE_BAR))
    assert sh.within_bar(d), d


@pytest.mark.parametrize("name", [n for n in sh.NAMES if n.endswith("noise-free")])
def test_noise_free_cases_recover_the_planted_poses(env, name):
    b, cam_stats = sh.case(name), _fit(env, name)[5][2]
    init = sh.assembled(name)["init"]
    d = sh.set_distance(*state_of(cam_stats, init["placed"]), *sh.planted_set(b, init["placed"], init["anchor"]))
    print("%s: %.2e rad %.2e from the planted set (bar %.2e %.2e)" % ((name,) + d + cf.POSE_BAR))
    assert sh.within_bar(d), d


@pytest.mark.parametrize("name", ["b 0.1 px", "d 0.1 px"])
def test_the_defaults_end_no_further_from_the_minimum_than_the_start(env, name):
    b, det, M, rigs, cams, (cs, tight, cam_stats) = _fit(env, name)
    _, stat, cam_stats_default = det.fit_camera_set(b["recs"], M, rigs, cams, min_items=b["min_items"])
    A, ref = sh.assembled(name), sh.joint_reference(name)
    placed = A["init"]["placed"]
    d = sh.set_distance(*state_of(cam_stats_default, placed), ref["R"], ref["t"])
    d0 = sh.set_distance(A["R0"], A["t0"], ref["R"], ref["t"])
    print("%s: defaults (rel_tol %g) %d rounds, cost %.6f, %.2e rad %.2e from the joint minimum (start %.2e %.2e); rel_tol %g: %d rounds, cost %.6f"
          % (name, ca.camera_fit_opts().rel_tol, stat["rounds"], stat["cost"], d[0], d[1], d0[0], d0[1], TIGHT, tight["rounds"], tight["cost"]))
    assert abs(ca.camera_fit_opts().rel_tol - 4 * cf.REL_TOL_ULP) <= 1e-3 * ca.camera_fit_opts().rel_tol
    assert d[0] <= d0[0] and d[1] <= d0[1]
    assert 1 <= stat["rounds"] <= 30 and stat["cost"] <= stat["cost_init"] == tight["cost_init"]


def test_an_unplaced_camera_gives_no_set(env):
    b, det, M, rigs, cams, (cs, stat, cam_stats) = _fit(env, "c 0.1 px")
    assert cs is None and stat["n_unplaced"] == 1 and cam_stats[0]["status"] == capi.POSE_NOT_SEEN and stat["anchor"] == 1
    # no pair shares min_items items: no anchor, every camera unplaced, the call still succeeds
    cs2, stat2, cam2 = det.fit_camera_set(b["recs"], M, rigs, cams, min_items=1000)
    assert cs2 is None and stat2["status"] == capi.POSE_NOT_SEEN and stat2["anchor"] == -1 and stat2["n_unplaced"] == len(cams)
    assert (cam2["status"] == capi.POSE_NOT_SEEN).all() and not cam2["rvec"].any() and not cam2["tvec"].any()


def test_camera_set_get_round_trip(env):
    b, det, M, rigs, cams, (cs, stat, cam_stats) = _fit(env, "b 0.1 px")
    poses = cs.poses()
    assert len(poses) == cs.n == len(cams)
    for c, (rv, tv) in enumerate(poses):
        assert rv.tobytes() == cam_stats[c]["rvec"].tobytes() and tv.tobytes() == cam_stats[c]["tvec"].tobytes()
    for got, want in zip(cs.cameras(), cams):
        assert bytes(got) == bytes(want)
    again = ca.CameraSet(cs.cameras(), poses)
    assert all(a[0].tobytes() == p[0].tobytes() and a[1].tobytes() == p[1].tobytes() for a, p in zip(again.poses(), poses))
    n = C.c_int()
    assert det.L.ctag_camera_set_get(cs.s, C.byref(n), None, None) == 0 and n.value == len(cams)
    assert det.L.ctag_camera_set_get(None, C.byref(n), None, None) == capi.ERR_ARG and det.L.ctag_camera_set_get(cs.s, None, None, None) == capi.ERR_ARG


def test_last_ms_by_kind():
    """ctag_camera_fit_last_ms: four kinds, all zero without CTAG_OPT_TIMING, all positive with it after a call that took rounds."""
    import testkit as tk
    b = sh.case("a 0.1 px")
    M, rigs, cams = input_of(b)
    for timing in (0, 1):
        det = tk.Detector(b["state"], 2, device=0)
        try:
            det.set_option(capi.OPT_TIMING, timing)
            _, stat, _ = det.fit_camera_set(b["recs"], M, rigs, cams, min_items=b["min_items"], rel_tol=TIGHT)
            ms = det.camera_fit_last_ms()
            assert list(ms) == ["rig_pose", "mv_pose", "record", "solve"] and stat["rounds"] >= 1
            assert all(v > 0.0 for v in ms.values()) if timing else not any(ms.values()), ms
        finally:
            det.close()


def _c_call(det, fn, res, n_cam, n_frames, M, rigs, cams, opts, n_stats=8):
    arr = (capi.CameraC * n_cam)(*cams[:n_cam]) if cams is not None else None
    stat, cam_stats = np.zeros(1, ca.CAMERA_FIT_STAT_DT), np.zeros(n_stats, ca.CAMERA_FIT_CAM_STAT_DT)
    out = C.c_void_p()
    st = fn(det.h, res, n_cam, n_frames, M.m if M is not None else None, rigs.r if rigs is not None else None, arr,
            C.byref(opts) if opts is not None else None, C.byref(out), stat.ctypes.data, cam_stats.ctypes.data)
    return st, out, stat, cam_stats


@pytest.mark.parametrize("name", ["b 0.1 px", "c 0.1 px"])
def test_two_calls_both_entries_and_the_c_abi_return_the_same_bytes(env, name):
    import torch
    b, det, M, rigs, cams, (cs, stat, cam_stats) = _fit(env, name)
    kw = dict(min_items=b["min_items"], rel_tol=TIGHT)
    again = det.fit_camera_set(b["recs"], M, rigs, cams, **kw)
    d = [torch.from_numpy(np.ascontiguousarray(b["recs"][c]).view(np.uint8).reshape(-1)).cuda() for c in range(len(cams))]
    dev = det.fit_camera_set_device([t.data_ptr() for t in d], b["recs"].shape[1], M, rigs, cams, **kw)
    recs = np.ascontiguousarray(b["recs"])
    st, out, cstat, ccam = _c_call(det, det.L.ctag_camera_fit, recs.ctypes.data, len(cams), recs.shape[1], M, rigs, cams, ca.camera_fit_opts(**kw))
    assert st == 0 and bool(out.value) == (cs is not None)
    c_set = ca.CameraSet._adopt(out) if out.value else None
    for o_set, o_stat, o_cam in (again, dev, (c_set, cstat[0], ccam[:len(cams)])):
        assert o_stat.tobytes() == stat.tobytes() and o_cam.tobytes() == cam_stats.tobytes()
        assert (o_set is None) == (cs is None)
        if cs is not None:
            assert all(a[0].tobytes() == p[0].tobytes() and a[1].tobytes() == p[1].tobytes() for a, p in zip(o_set.poses(), cs.poses()))


def test_rejections(env):
    """Rule 6, each on its own."""
    b = sh.case("a noise-free")
    det = env["dets"].of(b)
    M, rigs, cams = input_of(b)
    L = det.L
    recs = np.ascontiguousarray(b["recs"])
    n = recs.shape[1]

    def call(fn=L.ctag_camera_fit, res=recs.ctypes.data, n_cam=2, n_frames=n, m=M, r=rigs, c=cams, opts=None):
        return _c_call(det, fn, res, n_cam, n_frames, m, r, c, opts)[0]

    for bad in (dict(max_rounds=-1), dict(min_items=0), dict(min_points=0), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda_max=0.0), dict(rel_tol=0.0),
                dict(lambda0=float("nan"))):
        assert call(opts=ca.camera_fit_opts(**bad)) == capi.ERR_ARG, bad
    for null in (dict(res=None), dict(m=None), dict(r=None), dict(c=None), dict(n_frames=0)):
        assert call(**null) == capi.ERR_ARG, null
    assert call(n_cam=1) == capi.ERR_ARG
    nine = [cams[0]] * 9
    assert _c_call(det, L.ctag_camera_fit, recs.ctypes.data, 9, 1, M, rigs, nine, None, n_stats=9)[0] == capi.ERR_ARG
    other = sh.case("c noise-free")                      # rigs made for 4 models against a model of 2
    Mo, ro, _ = input_of(other)
    assert call(r=ro) == capi.ERR_ARG
    wide = sh.case("d noise-free")                       # 20 columns against a handle of 12
    Mw, rw, _ = input_of(wide)
    assert call(m=Mw, r=rw) == capi.ERR_ARG
    K = b["cameras"][0][0]
    tilted = ca.make_camera(K, np.float32([0] * 12 + [0.1, 0]))
    assert call(c=[cams[0], tilted]) == capi.ERR_UNSUPPORTED
    ptrs = (C.c_void_p * 2)(None, None)
    assert call(fn=L.ctag_camera_fit_device, res=ptrs) == capi.ERR_ARG
    assert call(fn=L.ctag_camera_fit_device, res=None) == capi.ERR_ARG
    assert call() == 0
