"""GPU tests of the rig assembly through the public calls (Detector.fit_rigs / fit_rigs_device): every batch of
tests/rig_fit_shapes.py is assembled once and the result is held to rules 1-7 of include/ctag_pose.h and to the independent
statement's joint minimum (tests/rig_fit_statement.py)."""
import ctypes as C

import numpy as np
import pytest

import cylindertag_amd as ca
import pose_statement as ps
import rig_fit_shapes as sh
import rig_fit_statement as rf
from cylindertag_amd import capi
from rig_fit_testlib import Detectors, device_poses, device_rig_poses, input_of, marker_costs, model_of, observation_cost

pytestmark = pytest.mark.gpu
# The default rel_tol stops a rig once a round gains less than float32 rounding of the model costs (4 x rf.REL_TOL_F32); on the 0.1 px
# batches that is a few thousandths of a millimetre before the minimum.  The tests below ask for the minimum itself: the loop runs on
# until lambda_max or max_rounds ends it.  test_the_default_tolerance_stops_earlier_at_a_cost_no_lower runs the defaults.
TIGHT = 1e-9


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "fit": {}}
    yield e
    e["dets"].close()


def _fit(env, name, max_rounds=None):
    """The batch assembled once (host entry) and shared: (batch, detector, camera, Model in, Rigs in, result tuple, its view)."""
    key = (name, max_rounds)
    if key not in env["fit"]:
        b = sh.batch(name)
        det, cam = env["dets"].of(b), ca.make_camera(b["K"], b["dist"])
        M, rigs = input_of(b)
        kw = {} if max_rounds is None else {"max_rounds": max_rounds}
        out = det.fit_rigs(b["recs"], M, rigs, cam, ca.rig_fit_opts(min_frames=b["min_frames"], rel_tol=TIGHT, **kw))
        env["fit"][key] = (b, det, cam, M, rigs, out, out[0].view())
    return env["fit"][key]


@pytest.mark.parametrize("name", sh.NAMES)
def test_per_marker_poses_are_not_mirrored(env, name):
    """The initialisation's basin (rule 2): every counted per-marker pose of the device has a cost near the planted pose's."""
    b = sh.batch(name)
    det, cam = env["dets"].of(b), ca.make_camera(b["K"], b["dist"])
    poses = device_poses(det, b["recs"], input_of(b)[0], cam)
    off = ps.offsets_of(b["recs"])
    counted = rf.counted_markers(b["recs"], b["model"], ok_of=lambda f, k: poses[off[f] + k]["status"] == 0)
    assert counted == sh.assembled(name)["counted"]
    sh.check_no_mirror(b, counted, marker_costs(b, poses, counted))


@pytest.mark.parametrize("name", sh.NAMES)
def test_result_obeys_the_rules(env, name):
    """Rules 2-4 from the statistics: the tree, the anchor, the counts, unplaced models and their status; the anchor's and unplaced
    models' bytes are the input's; cost / cost_init are the sums of the public rig call's record costs on the returned model and on
    the initial assembly, byte for byte; cost <= cost_init; rms_px; rvec / tvec reproduce the returned corners."""
    b, det, cam, M, rigs, (R, rig_stats, model_stats, placed), view = _fit(env, name)
    A = sh.assembled(name)
    m_in = b["model"]
    assert view["ids"].tobytes() == m_in["ids"].tobytes() and view["size"] == m_in["size"] and view["corners"].dtype == np.float32
    assert (placed == A["rig_placed"]).all()
    for m, st in enumerate(model_stats):
        rig = A["rigs"].get(int(b["rig_of_model"][m]))
        assert st["rig"] == b["rig_of_model"][m] and st["reserved"] == 0
        anchor = rig is not None and rig["anchor"] == m
        if A["rig_placed"][m] < 0 or anchor:
            for k in ("corners", "base", "axis"):
                assert view[k][m].tobytes() == m_in[k][m].tobytes(), (k, m)
            assert not st["rvec"].any() and not st["tvec"].any() and st["parent"] == -1 and st["n_frames_with_parent"] == 0
            assert st["status"] == (0 if anchor else capi.POSE_NOT_SEEN)
        else:
            assert st["status"] == 0 and st["parent"] == rig["parent"][m] and st["n_frames_with_parent"] == rig["n_with_parent"][m]
            Rm = ps.rodrigues(st["rvec"])
            for k, t in (("corners", st["tvec"]), ("base", st["tvec"]), ("axis", 0.0)):
                want = m_in[k][m].astype(np.float64) @ Rm.T + t
                assert np.abs(view[k][m] - want).max() <= rf.F32_SPACING_MM, (k, m)
        assert st["n_records"] == sum(o is not None and m in o["models"] for o in A["obs"])
    rigs_out = ca.Rigs(R, placed, b["n_rigs"])
    poses = device_rig_poses(det, b["recs"], R, rigs_out, cam)
    R0, stats0 = _fit(env, name, 0)[5][:2]
    poses0 = device_rig_poses(det, b["recs"], R0, rigs_out, cam)
    for g, st in enumerate(rig_stats):
        rig = A["rigs"][g]
        assert st["anchor"] == rig["anchor"] and st["n_placed"] == len(rig["placed"]) and st["n_unplaced"] == len(sh.members_of(b, g)) - len(rig["placed"])
        assert st["status"] == (0 if rig["anchor"] >= 0 else capi.POSE_NOT_SEEN) and st["reserved"] == 0
        mine = [o for o in A["obs"] if o is not None and o["rig"] == g]
        assert [o["w"] for o in mine] == [w for w in range(len(poses0)) if poses0[w]["rig"] == g and poses0[w]["status"] == 0 and poses0[w]["n_members"] >= 2]
        assert st["n_records"] == len(mine) and st["n_points"] == sum(len(o["ids"]) for o in mine)
        if not mine:
            continue
        assert 1 <= st["rounds"] <= 30 and st["cost"] <= st["cost_init"]
        assert st["cost_init"] == observation_cost(poses0, A["obs"], g) == stats0[g]["cost_init"] == stats0[g]["cost"]
        assert st["cost"] == observation_cost(poses, A["obs"], g), "stats.cost is not the cost of the returned model"
        assert st["rms_px"] == np.sqrt(2.0 * st["cost"] / st["n_points"])
        print("%s rig %d: %d records, %d rounds, cost %.6g -> %.6g, rms %.3g px, lambda %.3g" % (name, g, len(mine), st["rounds"], st["cost_init"], st["cost"],
                                                                                                 st["rms_px"], st["lambda"]))


@pytest.mark.parametrize("name", sh.NAMES)
def test_max_rounds_0_returns_the_initial_assembly(env, name):
    b, det, cam, M, rigs, (R0, rig_stats, model_stats, placed), view = _fit(env, name, 0)
    A = sh.assembled(name)
    assert not rig_stats["rounds"].any() and (rig_stats["cost"] == rig_stats["cost_init"]).all()
    placed_models = [m for m in range(len(placed)) if placed[m] >= 0]
    d = sh.corner_distance(view["corners"], A["X0"], placed_models)
    print("%s: the device's initial assembly lies %.2e mm from the statement's" % (name, d))
    assert d <= rf.CORNER_BAR_MM


@pytest.mark.parametrize("name", sh.NAMES)
def test_corners_against_the_joint_minimum(env, name):
    """The placed corners of every rig within 16 x the float32 spacing of the statement's joint minimum over transforms and rig
    poses (rf.CORNER_BAR_MM)."""
    b, det, cam, M, rigs, (R, rig_stats, model_stats, placed), view = _fit(env, name)
    A = sh.assembled(name)
    for g, ref in sh.joint_reference(name).items():
        d = sh.corner_distance(view["corners"], ref["X"], A["rigs"][g]["placed"])
        print("%s rig %d: %.2e mm from the joint minimum (bar %.2e); cost %.6g, the statement's %.6g" % (name, g, d, rf.CORNER_BAR_MM, rig_stats[g]["cost"], ref["cost"]))
        assert d <= rf.CORNER_BAR_MM, (name, g, d)


@pytest.mark.parametrize("name", [n for n in sh.NAMES if sh.batch(n)["claims"].get("recover")])
def test_noise_free_batches_recover_the_planted_layout(env, name):
    b, det, cam, M, rigs, (R, rig_stats, model_stats, placed), view = _fit(env, name)
    A = sh.assembled(name)
    for g, rig in A["rigs"].items():
        if rig["anchor"] < 0:
            continue
        want = rf.layout(b["model"]["corners"], sh.planted_layout(b, g, rig["anchor"], rig["placed"]), round_float=False)
        d = sh.corner_distance(view["corners"], want, rig["placed"])
        print("%s rig %d: %.2e mm from the planted layout (bar %.2e)" % (name, g, d, rf.CORNER_BAR_MM))
        assert d <= rf.CORNER_BAR_MM


@pytest.mark.parametrize("name", [sh.NAMES[1], sh.NAMES[2]])
def test_two_calls_and_both_entries_return_the_same_bytes(env, name):
    import torch
    b, det, cam, M, rigs, (R, rig_stats, model_stats, placed), view = _fit(env, name)
    opts = ca.rig_fit_opts(min_frames=b["min_frames"], rel_tol=TIGHT)
    again = det.fit_rigs(b["recs"], M, rigs, cam, opts)
    d_recs = torch.from_numpy(np.ascontiguousarray(b["recs"]).view(np.uint8).reshape(-1)).cuda()
    dev = det.fit_rigs_device(d_recs.data_ptr(), len(b["recs"]), M, rigs, cam, opts)
    for other in (again, dev):
        v = other[0].view()
        assert all(v[k].tobytes() == view[k].tobytes() for k in ("ids", "base", "axis", "corners"))
        assert other[1].tobytes() == rig_stats.tobytes() and other[2].tobytes() == model_stats.tobytes() and (other[3] == placed).all()


@pytest.mark.parametrize("name", [sh.NAMES[1], sh.NAMES[3]])
def test_the_default_tolerance_stops_earlier_at_a_cost_no_lower(env, name):
    b, det, cam, M, rigs, (R, rig_stats, model_stats, placed), view = _fit(env, name)
    out = det.fit_rigs(b["recs"], M, rigs, cam, ca.rig_fit_opts(min_frames=b["min_frames"]))
    st = out[1][0]
    assert abs(ca.rig_fit_opts().rel_tol - 4 * rf.REL_TOL_F32) <= 1e-3 * ca.rig_fit_opts().rel_tol
    ref = sh.joint_reference(name)[0]
    rig_placed = sh.assembled(name)["rigs"][0]["placed"]
    d = sh.corner_distance(out[0].view()["corners"], ref["X"], rig_placed)
    print("%s: defaults %d rounds, cost %.6f, %.2e mm from the joint minimum; rel_tol %g: %d rounds, cost %.6f" % (name, st["rounds"], st["cost"], d, TIGHT,
                                                                                                              rig_stats[0]["rounds"], rig_stats[0]["cost"]))
    # a default call stops short of the minimum (DESIGN.md section 16 records how far), never further from it than rule 2's start
    assert d <= sh.corner_distance(sh.assembled(name)["X0"], ref["X"], rig_placed)
    assert st["rounds"] <= rig_stats[0]["rounds"] and rig_stats[0]["cost"] <= st["cost"] <= st["cost_init"] == rig_stats[0]["cost_init"]


def test_model_file_round_trip_and_straight_into_the_rig_calls(env, tmp_path):
    b, det, cam, M, rigs, (R, rig_stats, model_stats, placed), view = _fit(env, sh.NAMES[2])
    path = str(tmp_path / "assembled.model")
    R.save(path)
    back = ca.Model(path).view()
    assert all(back[k].tobytes() == view[k].tobytes() for k in ("ids", "base", "axis", "corners"))
    A = sh.assembled(sh.NAMES[2])
    rigs_out = ca.Rigs(R, placed)
    o = next(o for o in A["obs"] if o is not None and o["rig"] == 0)
    rec = det.estimate_rig_pose(b["recs"][o["frame"]], R, rigs_out, cam)[0]
    assert rec["status"] == 0 and rec["n_members"] == len(o["markers"]) and rec["n_points"] == len(o["ids"])


def test_rejections(env):
    """Rule 7, each on its own."""
    b = sh.batch(sh.NAMES[0])
    det, cam = env["dets"].of(b), ca.make_camera(b["K"], b["dist"])
    M, rigs = input_of(b)
    L = det.L
    recs = np.ascontiguousarray(b["recs"])
    out = C.c_void_p()
    rs, msx = np.zeros(4, ca.RIG_FIT_STAT_DT), np.zeros(32, ca.RIG_FIT_MODEL_STAT_DT)

    def call(fn=L.ctag_rig_fit, res=recs.ctypes.data, n=len(recs), m=M.m, r=rigs.r, camera=cam, opts=None, o=C.byref(out), a=rs.ctypes.data, c=msx.ctypes.data, h=None):
        return fn(det.h if h is None else h, res, n, m, r, C.byref(camera) if camera is not None else None, C.byref(opts) if opts is not None else None, o, a, c)

    for bad in (dict(max_rounds=-1), dict(min_frames=0), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda_max=0.0), dict(rel_tol=0.0), dict(lambda0=float("nan"))):
        assert call(opts=ca.rig_fit_opts(**bad)) == capi.ERR_ARG, bad
    for null in (dict(res=None), dict(m=None), dict(r=None), dict(camera=None), dict(o=None), dict(a=None), dict(c=None), dict(n=0)):
        assert call(**null) == capi.ERR_ARG, null
    other = sh.batch(sh.NAMES[1])                       # rigs made for 4 models against a model of 2
    Mo, ro = input_of(other)
    assert call(r=ro.r) == capi.ERR_ARG
    wide = sh.batch(sh.NAMES[3])                        # 20 columns against a handle of 12
    Mw, rw = input_of(wide)
    assert call(m=Mw.m, r=rw.r) == capi.ERR_ARG
    truth, rig17, state = sh.over_the_cap()             # 17 models in one rig
    e = sh.batch(sh.NAMES[4])
    det4 = env["dets"].of(e)
    M17 = model_of(truth)
    r17 = ca.Rigs(M17, rig17, 1)
    big = np.zeros(17, ca.RIG_FIT_MODEL_STAT_DT)
    assert call(h=det4.h, res=np.ascontiguousarray(e["recs"]).ctypes.data, n=len(e["recs"]), m=M17.m, r=r17.r, c=big.ctypes.data) == capi.ERR_ARG
    M16, r16 = input_of(e)
    assert call(h=det4.h, res=np.ascontiguousarray(e["recs"]).ctypes.data, n=2, m=M16.m, r=r16.r, c=big.ctypes.data) == 0   # 16 pass
    L.ctag_model_free(out)
    out.value = None
    tilted = ca.make_camera(b["K"], np.float32([0] * 12 + [0.1, 0]))
    assert call(camera=tilted) == capi.ERR_UNSUPPORTED
    assert call(camera=ca.make_camera(b["K"], np.zeros(3, np.float32))) == capi.ERR_UNSUPPORTED
    assert call(fn=L.ctag_rig_fit_device, res=None) == capi.ERR_ARG
    assert not out.value
