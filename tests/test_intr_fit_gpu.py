"""GPU tests of the intrinsics fit through the public calls (Detector.fit_intrinsics / fit_intrinsics_device): every end-to-end case of
tests/intr_fit_shapes.py is fitted once and the result is held to rules 1-8 of include/ctag_pose.h and to the independent statement's
joint minimum (tests/intr_fit_statement.py)."""
import numpy as np
import pytest

import cylindertag_amd as ca
import intr_fit_shapes as sh
import intr_fit_statement as it
from cylindertag_amd import capi
from intr_fit_testlib import Detectors, cost_sum, device_rig_poses, input_of, model_of, opts_of, poses_of, vector_of

pytestmark = pytest.mark.gpu
E2E = [n for n in sh.NAMES if sh.case(n)["shape"] in sh.END_TO_END]
JOINT = [n for n in sh.NAMES if sh.case(n)["shape"] in sh.JOINT]


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "fit": {}}
    yield e
    e["dets"].close()


def _fit(env, name, **kw):
    """The case fitted once (host entry) and shared: (case, detector, Model, Rigs, seed, (CameraC, stat, poses))."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in env["fit"]:
        c = sh.case(name)
        det = env["dets"].of(c)
        M, rigs, seed = input_of(c)
        env["fit"][key] = (c, det, M, rigs, seed, det.fit_intrinsics(c["recs"], M, rigs, seed, **opts_of(c, **kw)))
    return env["fit"][key]


@pytest.mark.parametrize("name", E2E)
def test_result_obeys_the_rules(env, name):
    """Rules 1, 2 and 6 from the outputs: the observation set, the record fields, stat.cost and stat.pose_cost byte for byte, the
    statement's cost at the returned state, sigma2_hat and rms."""
    c, det, M, rigs, seed, (cam, stat, poses) = _fit(env, name)
    V = sh.views(name)
    seed_pass = device_rig_poses(det, c["recs"], M, rigs, seed)
    items = [i for i in range(len(seed_pass)) if seed_pass[i]["status"] == 0 and seed_pass[i]["n_points"] >= c["min_points"]]
    tie = sh.tie_of(c)
    rows = it.free_rows(c["mask"], tie)
    assert items == V.items and stat["status"] == 0 and stat["n_records"] == V.R and stat["n_points"] == sum(V.n_points)
    assert stat["n_free"] == len(rows) and stat["free_mask"] == sum(1 << i for i in rows) and 1 <= stat["rounds"] <= 30
    for i in range(len(poses)):
        if i in items:
            for k in ca.RIG_POSE_DT.names:
                if k not in ("rvec", "tvec", "cost"):
                    assert poses[i][k].tobytes() == seed_pass[i][k].tobytes(), (i, k)
        else:
            assert poses[i].tobytes() == seed_pass[i].tobytes(), i
    assert stat["cost"] == cost_sum(poses, items), "stat.cost is not the sum of the observations' cost fields"
    assert stat["cost"] <= stat["cost0"]
    p = vector_of(cam)
    want = it.total_cost(it.record_costs(V, p, poses_of(poses, V))[0])
    # every residual entry off by at most 64 roundings at a pixel coordinate's size: |d cost| <= sqrt(2 cost) sqrt(2 n) delta
    assert abs(stat["cost"] - want) <= np.sqrt(2 * want) * np.sqrt(2 * sum(V.n_points)) * 64 * 2.0 ** -52 * 2048, (stat["cost"], want)
    under = device_rig_poses(det, c["recs"], M, rigs, cam)
    assert stat["pose_cost"] == cost_sum(under, items), "stat.pose_cost is not the pose call's own sum under the returned camera"
    dof = 2 * stat["n_points"] - 6 * stat["n_records"] - stat["n_free"]
    assert stat["sigma2_hat"] == 2.0 * stat["cost"] / dof and stat["rms_px"] == np.sqrt(2.0 * stat["cost"] / stat["n_points"])
    assert cam.n_dist == seed.n_dist and [cam.K[i] for i in (1, 3, 6, 7, 8)] == [seed.K[i] for i in (1, 3, 6, 7, 8)]
    fixed = [i for i in range(it.N) if i not in rows and not (tie is not None and i == 1)]
    assert (p[fixed] == vector_of(seed)[fixed]).all()
    if tie is not None:
        assert p[1] == float(np.float32(p[0] * tie))
    print("%s: %d records, %d rounds, cost %.6g -> %.6g (pose back end's %.6g), rms %.3g px, lambda %.3g" % (name, V.R, stat["rounds"], stat["cost0"], stat["cost"],
                                                                                                       stat["pose_cost"], stat["rms_px"], stat["lambda"]))


@pytest.mark.parametrize("name", JOINT)
def test_camera_against_the_joint_minimum(env, name):
    """Every free parameter within the camera bar of the statement's joint minimum over the camera and all view poses."""
    c, _, _, _, _, (cam, stat, _) = _fit(env, name)
    J = sh.joint_reference(name)
    rows = it.free_rows(c["mask"], sh.tie_of(c))
    d, bar = np.abs(vector_of(cam) - J["p"]), it.camera_bar(J["p"], not c["noise"])
    print("%s: distance / bar %s, cost %.9g against the joint minimum's %.9g" % (name, [float("%.2g" % (d[i] / bar[i])) for i in rows], stat["cost"], J["cost"]))
    assert (d[rows] <= bar[rows]).all(), [(it.PARAMS[i], d[i], bar[i]) for i in rows if d[i] > bar[i]]


@pytest.mark.parametrize("name", JOINT)
def test_sigma_against_the_statement(env, name):
    """Rule 6's sigmas against the statement's at the returned state."""
    c, _, _, _, _, (cam, stat, poses) = _fit(env, name)
    V = sh.views(name)
    tie = sh.tie_of(c)
    rows = it.free_rows(c["mask"], tie)
    p = vector_of(cam)
    S, _ = it.reduced_system(V, p, poses_of(poses, V), tie)
    want, s2 = it.sigma(S, c["mask"], float(stat["cost"]), sum(V.n_points), V.R, tie)
    got = np.array(stat["sigma"])
    dev = float((np.abs(got - want)[rows] / want[rows]).max())
    print("%s: sigma %s, %.2e from the statement's (bar %.2e)" % (name, ["%s %.3g" % (it.PARAMS[i], got[i]) for i in rows], dev, it.SYSTEM_BAR["sigma"]))
    assert dev <= it.SYSTEM_BAR["sigma"]
    fixed = [i for i in range(it.N) if i not in rows and not (tie is not None and i == 1)]
    assert not got[fixed].any()
    if tie is not None:
        assert got[1] == tie * got[0]


@pytest.mark.parametrize("name", JOINT)
def test_defaults_end_no_further_from_the_joint_minimum(env, name):
    """The default rel_tol and round count: no free parameter ends further from the joint minimum than the seed was."""
    c = sh.case(name)
    det = env["dets"].of(c)
    M, rigs, seed = input_of(c)
    cam, stat, _ = det.fit_intrinsics(c["recs"], M, rigs, seed, free_mask=c["mask"], tie_focal=int(c["tie"]))
    J = sh.joint_reference(name)
    rows = it.free_rows(c["mask"], sh.tie_of(c))
    d1, d0 = np.abs(vector_of(cam) - J["p"]), np.abs(vector_of(seed) - J["p"])
    print("%s: defaults, %d rounds, distance now / at the seed %s" % (name, stat["rounds"], [float("%.2g" % (d1[i] / max(d0[i], 1e-300))) for i in rows]))
    assert stat["status"] == 0 and (d1[rows] <= d0[rows]).all()


@pytest.mark.parametrize("name", ["b 0.1 px", "c noise-free", "e 0.1 px"])
def test_two_calls_and_both_entries_return_the_same_bytes(env, name):
    import torch
    c, det, M, rigs, seed, (cam, stat, poses) = _fit(env, name)
    cam2, stat2, poses2 = det.fit_intrinsics(c["recs"], M, rigs, seed, **opts_of(c))
    d_recs = torch.from_numpy(np.ascontiguousarray(c["recs"]).view(np.uint8).reshape(-1)).cuda()
    cam3, stat3, poses3 = det.fit_intrinsics_device(d_recs.data_ptr(), len(c["recs"]), M, rigs, seed, **opts_of(c))
    for cm, st, ps_ in ((cam2, stat2, poses2), (cam3, stat3, poses3)):
        assert bytes(cm) == bytes(cam) and st.tobytes() == stat.tobytes() and ps_.tobytes() == poses.tobytes()


@pytest.mark.parametrize("name", ["a 0.1 px", "b 0.1 px", "d noise-free"])
def test_result_as_seed_is_kept_or_improved(env, name):
    """The camera a fit returns, given back as the seed, comes back unchanged or with a lower cost."""
    c, det, M, rigs, seed, (cam, stat, _) = _fit(env, name)
    cam2, stat2, _ = det.fit_intrinsics(c["recs"], M, rigs, cam, **opts_of(c))
    assert stat2["status"] == 0
    assert bytes(cam2) == bytes(cam) or stat2["cost"] < stat["cost"], (stat["cost"], stat2["cost"])
    assert stat2["cost"] <= stat["cost"] * (1 + 1e-12)


def test_max_rounds_0_returns_the_seed(env):
    c, det, M, rigs, seed, (_, stat, _) = _fit(env, "b 0.1 px")
    cam0, stat0, poses0 = det.fit_intrinsics(c["recs"], M, rigs, seed, **opts_of(c, max_rounds=0))
    assert bytes(cam0) == bytes(seed) and stat0["status"] == 0 and stat0["rounds"] == 0 and stat0["cost"] == stat0["cost0"] == stat["cost0"]


def test_rigs_none_makes_every_model_a_rig(env):
    c = sh.case("a 0.1 px")
    det = env["dets"].of(c)
    M, rigs, seed = input_of(c)
    a = det.fit_intrinsics(c["recs"], M, None, seed, **opts_of(c))
    b = det.fit_intrinsics(c["recs"], M, rigs, seed, **opts_of(c))
    assert bytes(a[0]) == bytes(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_statuses_of_rule_6(env):
    c = sh.case("c 0.1 px")
    det = env["dets"].of(c)
    M, rigs, seed = input_of(c)
    # no observation: every frame failed
    recs = c["recs"].copy()
    recs["status"] = 1
    cam, stat, poses = det.fit_intrinsics(recs, M, rigs, seed, **opts_of(c))
    assert stat["status"] == capi.POSE_NOT_SEEN and bytes(cam) == bytes(seed) and stat["n_records"] == 0 and (poses["status"] == capi.POSE_NOT_SEEN).all()
    # one record of one column: 8 points, 2 x 8 - 6 = 10 is not above the twelve unknowns of the eight-coefficient default mask
    one = c["recs"][:1].copy()
    one["n_markers"] = 1
    one["markers"][0, 0]["n_features"] = one["markers"][0, 0]["n_pos"] = 1
    cam, stat, poses = det.fit_intrinsics(one, M, rigs, seed, min_points=8, free_mask=0)
    assert stat["n_records"] == 1 and stat["n_points"] == 8 and stat["n_free"] == 12
    assert stat["status"] == capi.POSE_TOO_FEW and bytes(cam) == bytes(seed)
    assert poses.tobytes() == device_rig_poses(det, one, M, rigs, seed).tobytes()
    cam, stat, poses = det.fit_intrinsics(one, M, rigs, seed, min_points=8, free_mask=0xF)   # four unknowns: enough
    assert stat["status"] == capi.POSE_OK and stat["n_free"] == 4
    # a seed under which no point can be projected: the rational denominator is negative everywhere but at the principal point
    bad = ca.make_camera(c["seed"][0], np.float32([0, 0, 0, 0, 0, -1e9, 0, 0]))
    cam, stat, poses = det.fit_intrinsics(c["recs"], M, rigs, bad, min_points=8, free_mask=0xF)
    print("unusable seed: status %d, %d records" % (stat["status"], stat["n_records"]))
    assert stat["n_records"] > 0 and stat["status"] == capi.POSE_DEGENERATE and bytes(cam) == bytes(bad) and stat["rounds"] == 0


def test_tied_focal_length_with_a_ratio_other_than_one(env):
    """tie_focal through the public call with the planted fy / fx (0.99986): the returned fy is float32(fx x ratio), sigma[fy] is ratio x
    sigma[fx], bit 1 is out of the mask in use, and the cost is that of the statement's joint minimum under the same tie up to what
    half a float32 spacing of the tied fy is worth (the distance per parameter is printed: DESIGN.md section 18 says why the tied
    cases held to the camera bar tie fy = fx)."""
    c = sh.case("b 0.1 px")
    det = env["dets"].of(c)
    M, rigs, seed = input_of(c)
    V = sh.views(c["name"])
    mask = 0x3F
    cam, stat, poses = det.fit_intrinsics(c["recs"], M, rigs, seed, free_mask=mask, tie_focal=1, rel_tol=1e-12)
    p, p0 = vector_of(cam), vector_of(seed)
    tie = float(p0[1] / p0[0])
    assert tie != 1.0 and stat["status"] == 0 and stat["free_mask"] == mask & ~2 and stat["n_free"] == 5
    assert p[1] == float(np.float32(p[0] * tie)) and stat["sigma"][1] == tie * stat["sigma"][0] and stat["cost"] < stat["cost0"]
    J = it.joint_minimum(V, p0, mask, tie, sh.planted_poses(c, V))
    rows = it.free_rows(mask, tie)
    d, bar = np.abs(p - J["p"]), it.camera_bar(J["p"], False)
    print("tie %.6f: distance / bar %s, cost %.9g against the joint minimum's %.9g" % (tie, [float("%.2g" % (d[i] / bar[i])) for i in rows], stat["cost"], J["cost"]))
    # moving fy alone by half a spacing h changes the cost by at most |g_fy| h + S_fyfy h^2 / 2 at the tied minimum, where the gradient in
    # fy alone is what the tie holds back; both from the statement's untied system there
    S, g = it.reduced_system(V, J["p"], J["poses"], None)
    h = float(it.half_spacing(J["p"])[1])
    assert abs(stat["cost"] - J["cost"]) <= 4 * (abs(g[1]) * h + 0.5 * S[1, 1] * h * h) + 1e-9 * J["cost"], (stat["cost"], J["cost"], abs(g[1]) * h)


def test_rejections_of_rule_8(env):
    c = sh.case("b 0.1 px")
    det = env["dets"].of(c)
    M, rigs, seed = input_of(c)

    def status_of(model=M, rigs_=rigs, seed_=seed, **kw):
        with pytest.raises(ca.CtagError) as e:
            det.fit_intrinsics(c["recs"], model, rigs_, seed_, **kw)
        return e.value.status

    for kw in (dict(max_rounds=-1), dict(min_points=0), dict(lambda0=0.0), dict(lambda_max=float("inf")), dict(rel_tol=float("nan")), dict(rel_tol=-1.0),
               dict(free_mask=1 << 16), dict(free_mask=1 << 9), dict(free_mask=2, tie_focal=1)):
        assert status_of(**kw) == capi.ERR_ARG, kw
    with pytest.raises(ca.CtagError) as e:                                     # n_frames < 1: no record at all
        det.fit_intrinsics(c["recs"][:0], M, rigs, seed)
    assert e.value.status == capi.ERR_ARG
    import ctypes as C
    res = np.ascontiguousarray(c["recs"])
    out, stat, o = ca.CameraC(), np.zeros(1, ca.INTRINSICS_FIT_STAT_DT), ca.intrinsics_fit_opts()
    good = [det.h, res.ctypes.data, len(res), M.m, rigs.r, C.byref(seed), C.byref(o), C.byref(out), stat.ctypes.data, None]
    for fn in (det.L.ctag_intrinsics_fit, det.L.ctag_intrinsics_fit_device):
        for k in (0, 1, 3, 4, 5, 7, 8):                                        # every pointer but opts and poses_out, which may be null
            args = list(good)
            args[k] = None
            assert fn(*args) == capi.ERR_ARG, (fn, k)
        args = list(good)
        args[2] = 0
        assert fn(*args) == capi.ERR_ARG
    args = list(good)
    args[6] = None                                                             # opts == NULL: the defaults
    assert det.L.ctag_intrinsics_fit(*args) == 0 and stat[0]["status"] == 0
    other = sh.case("a 0.1 px")
    assert status_of(model=model_of(other["model"]), rigs_=ca.Rigs(model_of(other["model"]), other["rig_of_model"], 1)) == capi.ERR_ARG   # 20 columns on a 12-column dictionary
    assert status_of(rigs_=ca.Rigs(model_of(sh.case("c 0.1 px")["model"]), [0, 0, 1, 1], 2)) == capi.ERR_ARG                              # rigs made for four models
    tilted = ca.make_camera(c["seed"][0], np.float32([0] * 12 + [0.01, 0]))
    assert status_of(seed_=tilted) == capi.ERR_UNSUPPORTED
    three = ca.make_camera(c["seed"][0], np.zeros(3, np.float32))
    assert status_of(seed_=three) == capi.ERR_UNSUPPORTED
