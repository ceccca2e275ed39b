"""CPU tests of tests/cov_statement.py, the independent statement the pose covariance of the device is held against
(tests/test_pose_cov_gpu.py): its Jacobians against central differences of the pose statements' residuals, its two
parametrisations against each other, the float64 error its comparison bar comes from, its consistency on planted poses with
known pixel noise, and the planted errors its checker must refuse."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import cov_shapes as sh
import cov_statement as cs
import mv_statement as ms
import pose_statement as ps
from ctag_testlib import RESULT_DT
from pose_testlib import POSE_DT, golden_camera_and_model
from rig_shapes import FULL
from rig_testlib import stacked_rig_model, synth_rig_frame


@pytest.fixture(scope="module")
def cases():
    return sh.all_cases()


def _parts(case, P):
    if case["kind"] == "marker":
        return cs.parts_of_marker(P, case["recs"], case["model"])
    if case["kind"] == "rig":
        return cs.parts_of_rig(P, case["recs"], case["model"])
    return cs.parts_of_mv(P, case["recs"], case["model"])


def _log(R):
    return ms.rotvec(R)


def test_jacobians_against_central_differences_of_the_statements_residual(cases):
    """Both Jacobians, for a per-marker, a rig and a three-camera record: |J - central difference| <= 1e-7 max|J| with step 1e-6 (a
    trial gave 3e-11; a wrong derivative is off by order 1).  The residual itself equals mv_statement.MvProblem's."""
    worst = 0.0
    for name, w in (("marker size 20 golden", 4), ("rig golden", 0), ("mv three own cameras", 0)):
        case = next(c for c in cases if c["name"] == name)
        P = case["sources"][w]
        parts = _parts(case, P)
        pb = ms.MvProblem(case["cameras"], case["camera_poses"], parts)
        pp = cs.problem_parts(parts, case["cameras"], case["camera_poses"])
        x = np.concatenate([P["rvec"], P["tvec"]])
        h = 1e-6
        for param in (cs.RVEC, cs.TANGENT):
            r, J, _ = cs.residual_jacobian(pp, P["rvec"], P["tvec"], param)
            assert np.abs(r - pb.residual(x)).max() <= 1e-9

            def at(d):
                if param == cs.RVEC:
                    return pb.residual(x + d)
                rv = _log(ps.rodrigues(d[:3]) @ ps.rodrigues(x[:3]))
                return pb.residual(np.concatenate([rv, x[3:] + d[3:]]))
            num = np.stack([(at(h * e) - at(-h * e)) / (2 * h) for e in np.eye(6)], 1)
            d = float(np.abs(J - num).max() / np.abs(J).max())
            worst = max(worst, d)
            assert d <= 1e-7, (name, param, d)
    print("Jacobians against central differences: worst %.1e of max|J|" % worst)


def _left_jacobian(r):
    th = np.sqrt(r @ r)
    rx = cs.skew(r)
    return np.eye(3) + (1 - np.cos(th)) / th ** 2 * rx + (th - np.sin(th)) / th ** 3 * rx @ rx


def test_the_two_parametrisations_agree(cases):
    """Exp(dw) Exp(r) = Exp(r + Jl(r)^-1 dw): the RVEC covariance is the TANGENT covariance carried by blockdiag(Jl^-1, I)."""
    worst = 0.0
    for case in cases:
        for opts in (cs.default_opts(sigma_px=0.2), cs.default_opts()):
            T = sh.expected_of(case, dict(opts, param=cs.TANGENT))
            R = sh.expected_of(case, dict(opts, param=cs.RVEC))
            for P, t, r in zip(case["sources"], T, R):
                assert t["status"] == r["status"]
                if t["status"] != cs.COV_OK:
                    continue
                B = np.eye(6)
                B[:3, :3] = np.linalg.inv(_left_jacobian(np.asarray(P["rvec"], np.float64)))
                moved = dict(t, cov=B @ t["cov"] @ B.T, min_pivot=r["min_pivot"])
                d = cs.deviation(moved, r)
                worst = max(worst, d)
                assert d <= cs.BAR, (case["name"], d)
    print("RVEC against the moved TANGENT covariance: worst deviation %.1e (bar %.1e)" % (worst, cs.BAR))


def test_float64_error_of_the_statement_is_the_written_figure(cases):
    """The worst deviation of the float64 statement from the longdouble statement over every record of every case, in both
    parametrisations, is cov_statement.MEASURED_F64_DEVIATION (not above it, and not below a quarter of it: the written figure is
    the measured one); the bar is 16 times that."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    worst, where = 0.0, None
    for case in cases:
        for param in (cs.TANGENT, cs.RVEC):
            opts = cs.default_opts(param=param)
            a, b = sh.expected_of(case, opts), sh.expected_of(case, opts, np.longdouble)
            for w, (x, y) in enumerate(zip(a, b)):
                assert x["status"] == y["status"], (case["name"], w)
                if x["status"] == cs.COV_OK:
                    for k in ("n_points", "dof", "worst_point", "n_outliers"):
                        assert x[k] == y[k]
                    d = cs.deviation(x, y)
                    if d > worst:
                        worst, where = d, (case["name"], w, int(x["n_points"]))
    print("float64 statement against longdouble: worst deviation %.2e at %s; written %.2e, bar %.2e" % (worst, where, cs.MEASURED_F64_DEVIATION, cs.BAR))
    assert cs.MEASURED_F64_DEVIATION / 4 <= worst <= cs.MEASURED_F64_DEVIATION
    assert cs.BAR == 16 * cs.MEASURED_F64_DEVIATION


def test_rules_of_the_statement(cases):
    """Every case's "expect" list; the planted 5 px outlier is the worst point and is counted; every OK record of the well-posed
    cases keeps its smallest pivot far above the threshold."""
    for case in cases:
        E = sh.expected_of(case, cs.default_opts(sigma_px=0.2))
        if "expect" in case:
            assert [e["status"] for e in E] == case["expect"], case["name"]
        else:
            assert all(e["status"] == cs.COV_OK and e["min_pivot"] > 1e-9 for e in E), case["name"]
        if case.get("outlier"):
            w, i = case["outlier"]
            for opts in (cs.default_opts(sigma_px=0.2), cs.default_opts()):
                e = sh.expected_of(dict(case, sources=case["sources"][w:w + 1]), opts)[0]
                assert e["worst_point"] == i and e["n_outliers"] >= 1 and e["max_residual_px"] > 4.0
            assert sh.expected_of(dict(case, sources=case["sources"][w:w + 1]), cs.default_opts(outlier_k=0.0))[0]["n_outliers"] == 0
    singular = next(c for c in cases if c["name"] == "rules")
    for P in singular["sources"][-2:]:  # the pivots the threshold separates from the well-posed ones
        pp = cs.problem_parts(cs.parts_of_marker(P, singular["recs"], singular["model"]), singular["cameras"], singular["camera_poses"])
        _, J, _ = cs.residual_jacobian(pp, P["rvec"], P["tvec"], cs.TANGENT)
        assert cs.scaled_inverse(J.T @ J) == (None, None)


def _undistortion_converged(K, dist, img):
    """The residual lives in undistorted pixels.  Far off the axis (the stacked rig is taller than the golden camera's image) the five
    fixed-point steps of the undistortion do not converge; such a pixel, distorted again, misses itself by tens of pixels and is no
    observation of the planted pose under that residual.  A draw with such a pixel (about 1 in 100) is drawn again."""
    xn = ps.undistort12(K, dist, img)
    back = ps.project12(K, dist, np.zeros(3), np.zeros(3), np.column_stack([xn, np.ones(len(xn))]))
    return bool(np.abs(back - np.asarray(img, np.float64)).max() < 0.01)


def _consistency(model, rigs, K, dist, sigma, n=300, seed=7):
    """n planted poses (rig_testlib.random_pose through synth_rig_frame), iid Gaussian pixel noise sigma, the pose scipy's minimum
    from the planted one: d^T cov^-1 d of d = (Log(R_est R_true^T), t_est - t_true), with sigma_px = sigma and with sigma2_hat."""
    rng = np.random.default_rng(seed)
    rig_of_model = np.full(len(model["ids"]), -1, np.int32)
    rig_of_model[rigs[0]] = 0
    given, hat, points = [], [], []
    import rig_statement as rs
    while len(given) < n:
        rec, truth = synth_rig_frame(rng, model, rigs, K, dist, sigma, feats=(2, 5), patterns=(FULL,))
        H, obj, img = rs.expected_header(rec, model, rig_of_model, 0, 0)
        assert H["status"] == 0
        if not _undistortion_converged(K, dist, img):
            continue
        pp = cs.problem_parts([(0, obj, img)], [(K, dist)], [cs.IDENTITY_POSE])

        def fun(p):
            return cs.residual_jacobian(pp, p[:3], p[3:], cs.RVEC)[0]

        def jac(p):
            return cs.residual_jacobian(pp, p[:3], p[3:], cs.RVEC)[1]
        sol = least_squares(fun, np.concatenate(truth[0]), jac=jac, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac")
        d = np.concatenate([_log(ps.rodrigues(sol.x[:3]) @ ps.rodrigues(truth[0][0]).T), sol.x[3:] - truth[0][1]])
        for out, opts in ((given, cs.default_opts(sigma_px=sigma)), (hat, cs.default_opts())):
            e = cs.covariance(pp, sol.x[:3], sol.x[3:], opts)
            assert e["status"] == cs.COV_OK
            out.append(float(d @ np.linalg.solve(e["cov"], d)))
        points.append(len(obj))
    return np.array(given), np.array(hat), (min(points), max(points))


@pytest.mark.parametrize("sigma", [0.2, 0.5])
@pytest.mark.parametrize("what", ["one marker", "three stacked markers"])
def test_covariance_is_consistent_with_planted_noise(what, sigma):
    """The mean of d^T cov^-1 d over 300 planted poses lies within 6 +- 5 sqrt(12 / 300) = [5, 7] (6 and 12: mean and variance of
    chi^2 with 6 degrees of freedom).  Measured: one marker (16-40 points) 6.11 at 0.2 px, 6.32 at 0.5 px; three stacked markers
    (48-120 points) 6.29 and 6.30.  The sigma2_hat variant is printed only (its expectation is 6 nu / (nu - 2), not 6)."""
    K, dist, golden = golden_camera_and_model()
    model, rigs = (golden, [[0]]) if what == "one marker" else (stacked_rig_model(golden, 3, 70.0), [[0, 1, 2]])
    given, hat, pts = _consistency(model, rigs, K, dist, sigma)
    print("%s, %d-%d points, sigma %.1f px: mean d^T cov^-1 d = %.2f (median %.2f); with sigma2_hat %.2f" %
          (what, pts[0], pts[1], sigma, given.mean(), np.median(given), hat.mean()))
    assert 5.0 <= given.mean() <= 7.0


def _one_record(case, w, opts):
    sub = dict(case, sources=case["sources"][w:w + 1])
    e = sh.expected_of(sub, opts)[0]
    return sub, e, np.array([cs.to_record(e)])


def test_checker_refuses_planted_errors(cases, monkeypatch):
    case = next(c for c in cases if c["name"] == "marker size 20 golden")
    opts = cs.default_opts(sigma_px=0.2)
    sub, e, G = _one_record(case, 4, opts)
    assert cs.check_cov_records(G, [e], sub["sources"]) <= 1e-12  # the statement's own record passes

    def refused(rec, want=e, src=sub["sources"]):
        with pytest.raises(AssertionError):
            cs.check_cov_records(rec, [want], src)
    # a transposed [e_k]x
    good_rotation = cs.rotation

    def transposed(rvec, param, ft=np.float64):
        R, dR = good_rotation(rvec, param, ft)
        return R, [cs.skew(np.eye(3)[k]).T @ R for k in range(3)] if param == cs.TANGENT else dR
    monkeypatch.setattr(cs, "rotation", transposed)
    bad = np.array([cs.to_record(sh.expected_of(sub, opts)[0])])
    monkeypatch.setattr(cs, "rotation", good_rotation)
    refused(bad)
    # cov not scaled by sigma2_used
    bad = G.copy()
    bad["cov"] /= bad["sigma2_used"]
    refused(bad)
    # dof = 2n
    bad = G.copy()
    bad["dof"] = 2 * bad["n_points"]
    refused(bad)
    bad["sigma2_hat"] = 2 * bad["cost"] / bad["dof"]
    refused(bad)
    # the rotation and translation blocks swapped
    bad = G.copy()
    p = [3, 4, 5, 0, 1, 2]
    bad["cov"][0] = G["cov"][0][np.ix_(p, p)]
    refused(bad)
    # cov not symmetric bit for bit
    bad = G.copy()
    bad["cov"][0][0, 1] = np.nextafter(bad["cov"][0][0, 1], np.inf)
    refused(bad)
    # a field set on a record without a pose
    P = sub["sources"].copy()
    P["status"] = 2
    bad = np.array([cs.to_record({"status": cs.COV_NO_POSE})])
    cs.check_cov_records(bad, [{"status": cs.COV_NO_POSE}], P)
    bad["n_points"] = 60
    refused(bad, {"status": cs.COV_NO_POSE}, P)


def test_checker_refuses_the_last_of_tied_maxima():
    """Two features with the same position and the same pixels give pairs of equal residual norms; the largest belongs to points 2
    and 10: worst_point is 2, and a record that names 10 is refused."""
    K, dist, _ = golden_camera_and_model()
    from pose_testlib import make_cylinder_model
    from rig_shapes import _pixels, _place, _pose
    model = make_cylinder_model(1, 12)
    rng = np.random.default_rng(3)
    pose = _pose(rng, model["corners"][0])
    rec = np.zeros(1, RESULT_DT)
    _place(rec[0], 0, _pixels(rng, model, 0, K, dist, pose, 0.2), 4, [FULL, FULL, FULL])
    F = rec[0]["features"]
    F[0]["corners"][8] += np.float32(5.0)  # corner 4: point 2 of the feature
    F[1] = F[0]
    P = np.zeros(1, POSE_DT)
    P["n_points"], P["rvec"], P["tvec"] = 24, pose[0], pose[1]
    case = sh._fill_costs({"kind": "marker", "recs": rec, "model": model, "cameras": [(K, dist)], "camera_poses": [sh.ZERO_POSE], "sources": P})
    e = sh.expected_of(case, cs.default_opts())[0]
    assert e["status"] == cs.COV_OK and e["worst_point"] == 2
    G = np.array([cs.to_record(e)])
    cs.check_cov_records(G, [e], P)
    G["worst_point"] = 10
    with pytest.raises(AssertionError):
        cs.check_cov_records(G, [e], P)
