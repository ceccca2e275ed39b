"""CPU tests of tests/robust_statement.py, the independent statement the robust refit of the device is held against
(tests/test_robust_pose_gpu.py), and of the shapes of tests/robust_shapes.py: the conditions every shape must meet on the statement
alone, the three measured figures the comparison bars come from, the coverage the shapes claim, the planted errors the checker must
refuse, the layout of the two new structs and log64 on the host.

What the loop's step counts can be held to.  PoseBA's stop rules are a step of 1e-10 |x| and a cost change of 1e-15 of the cost.  The
residual is a difference of two pixel coordinates near 1000 that agree to a fraction of a pixel, so a float64 cost carries a relative
rounding error of about 2.2e-16 x 1000 / (rms residual): 1e-12 at 0.2 px, a thousand times the cost rule.  Every loop that is not
ended by max_iterations therefore ends in steps whose acceptance is decided by rounding:
test_uncapped_loops_end_in_the_rounding_of_their_cost asserts that, measured in longdouble where there is no such rounding, the
smallest relative cost change an uncapped loop decides on lies within 100 times that rounding for every record (within 1 for nine in
ten), and prints in how many of them float64 and longdouble accept the same number of steps (about half).  A condition that float64
and longdouble agree on the accepted steps of EVERY refitted record can therefore not be met by choosing other shapes, and a device
that sums in another order cannot be held to the statement's iteration count there.  Step counts are held equal -- between float64
and longdouble here, between the device and float64 on the GPU -- for every loop that max_iterations ends (0, 1 and 2) and for the
record that runs into the cap of 50; an uncapped loop is held to its final pose, under the bar LOOP and STOP give."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.optimize import least_squares

import cov_statement as cs
import robust_shapes as shp
import robust_statement as rb
from ctag_testlib import ROOT

LD = np.longdouble
pytestmark = pytest.mark.skipif(np.finfo(LD).eps >= np.finfo(np.float64).eps, reason="no extended precision on this platform")


@pytest.fixture(scope="module")
def runs():
    """[(case, run name, options, float64 dicts, longdouble dicts)] for every run of every case."""
    return [(c, name, o, shp.expected_of(c, o), shp.expected_of(c, o, LD)) for c in shp.all_cases() for name, o in shp.runs_of(c)]


def _ok(A, B):
    return [(w, a, b) for w, (a, b) in enumerate(zip(A, B)) if a["status"] == rb.ROBUST_OK]


def test_conditions_every_shape_meets(runs):
    """On the statement alone: statuses are the expected ones and the same in both float types; no point of any record lies within
    THRESHOLD_MARGIN a^2 of the inlier threshold in either, so masks, n_inliers and worst_point are EQUAL in both; every record that is
    refitted has min_pivot >= 1e-6 in its covariance; loops that max_iterations ends, and the one that runs into the cap of 50, take
    the same steps in both."""
    seen = set()
    for c, name, o, A, B in runs:
        assert rb.opts_ok(o)
        assert [a["status"] for a in A] == [b["status"] for b in B], (c["name"], name)
        if "expect" in c:
            assert [a["status"] for a in A] == c["expect"], (c["name"], name)
        elif c["name"] != "nan pixel":
            assert all(a["status"] == rb.ROBUST_OK for a in A), (c["name"], name)
        for w, a, b in _ok(A, B):
            at = (c["name"], name, w)
            assert min(a["threshold_gap"], b["threshold_gap"]) >= rb.THRESHOLD_MARGIN, at
            for k in ("n_points", "n_inliers", "worst_point", "loss"):
                assert a[k] == b[k], (at, k)
            assert np.array_equal(a["inlier_mask"], b["inlier_mask"]), at
            assert a["n_inliers"] == sum(bin(int(v)).count("1") for v in a["inlier_mask"])
            capped = a["trace"]["stop"] == "cap" and b["trace"]["stop"] == "cap"
            if o["max_iterations"] <= 2 or capped:
                assert capped and a["iterations"] == b["iterations"] == o["max_iterations"], at
                assert a["trace"]["accepted"] == b["trace"]["accepted"], at
            if (c["name"], w) not in seen:
                seen.add((c["name"], w))
                P = c["sources"][w]
                e = cs.expected(P, rb.parts_of(c, P), c["cameras"], c["camera_poses"], cs.default_opts())
                assert e["status"] == cs.COV_OK and e["min_pivot"] >= 1e-6, (at, e.get("min_pivot"))


def test_uncapped_loops_end_in_the_rounding_of_their_cost(runs):
    """See the module's text."""
    total = same = inside = 0
    for c, name, o, A, B in runs:
        if o["max_iterations"] < rb.MAX_ITERATIONS:
            continue
        for w, a, b in _ok(A, B):
            if b["trace"]["stop"] == "cap":
                continue
            total += 1
            same += a["trace"]["accepted"] == b["trace"]["accepted"]
            assert b["trace"]["stop"] in ("step", "cost"), (c["name"], name, w, b["trace"])
            rounding = np.finfo(np.float64).eps * 1000.0 / np.sqrt(2 * float(b["cost_ls"]) / b["n_points"])
            assert b["trace"]["least_change"] < 100 * rounding, (c["name"], name, w, b["trace"], rounding)
            inside += b["trace"]["least_change"] < rounding
    print("uncapped loops: %d; smallest decided cost change within the cost's rounding in %d; float64 and longdouble accept the same "
          "number of steps in %d" % (total, inside, same))
    assert total >= 200 and inside >= 0.9 * total and same < 0.75 * total


def _polished(pp, e, o):
    """scipy's minimum of rule 5's objective from the float64 loop's end: the residual sqrt(rho(s_i) / s_i) r_i has rule 5's cost as
    its sum of squares and is smooth (the factor tends to 1 at s_i = 0)."""
    a = np.float64(e["scale_px"])

    def fun(x):
        ru, rv, _, _ = rb.rows(pp, x)
        s = ru * ru + rv * rv
        rho, _ = rb.loss(s, a, o["loss"])
        f = np.sqrt(np.where(s > 0, rho / np.where(s > 0, s, 1.0), 1.0))
        return np.concatenate([ru * f, rv * f])
    x0 = np.concatenate([e["rvec"], e["tvec"]]).astype(np.float64)
    return least_squares(fun, x0, jac="3-point", method="trf", x_scale="jac", xtol=None, ftol=None, gtol=1e-14, max_nfev=12).x


def test_measured_figures_are_the_written_ones(runs):
    """EVAL over every record of every run with max_iterations = 0; LOOP and STOP over every record of every other run.  Each written
    constant is not below its measured figure and not above four times it; the bars are 16 times the constants."""
    ev = lo = st = 0.0
    where = {}
    for c, name, o, A, B in runs:
        for w, a, b in _ok(A, B):
            if o["max_iterations"] == 0:
                d = rb.eval_deviation(a, b)
                if d > ev:
                    ev, where["EVAL"] = d, (c["name"], name, w)
                continue
            H = rb.hessian_at(shp.pparts_of(c, LD)(w), rb.pose_of(b), b["scale_px"], o["loss"])
            d = rb.pose_distance(rb.pose_of(a), rb.pose_of(b), H)
            if d > lo:
                lo, where["LOOP"] = d, (c["name"], name, w)
            if o["max_iterations"] == rb.MAX_ITERATIONS and a["trace"]["stop"] != "cap":
                d = rb.pose_distance(rb.pose_of(a), _polished(shp.pparts_of(c)(w), a, o), H)
                if d > st:
                    st, where["STOP"] = d, (c["name"], name, w)
    print("EVAL %.3e (written %.1e)  LOOP %.3e (written %.1e)  STOP %.3e (written %.1e)  at %s" % (ev, rb.EVAL, lo, rb.LOOP, st, rb.STOP, where))
    print("bars: evaluated fields %.2e, final poses %.2e pose sigmas per pixel of noise" % (rb.EVAL_BAR, rb.POSE_BAR))
    assert rb.EVAL / 4 <= ev <= rb.EVAL and rb.LOOP / 4 <= lo <= rb.LOOP and rb.STOP / 4 <= st <= rb.STOP
    assert rb.EVAL_BAR == 16 * rb.EVAL and rb.POSE_BAR == 16 * max(rb.LOOP, rb.STOP)


def _run(runs, case, name):
    return next(r for r in runs if r[0]["name"] == case and r[1] == name)


def test_shapes_cover_what_they_claim(runs):
    """From the statement's own records and traces."""
    cases = {c["name"]: c for c in shp.all_cases()}
    m = cases["marker size 20 golden"]
    assert [int(n) for n in m["sources"]["n_points"][0::2]] == list(shp.MARKER_COUNTS) and set(m["runs"]) == set(shp.OPTION_SETS)
    assert sorted(int(n) for n in cases["rig golden"]["sources"]["n_points"]) == [164, 256, 796, 800]
    assert [len(cases[k]["cameras"]) for k in ("mv 8 + 8", "mv three own cameras", "mv eight cameras")] == [2, 3, 8]
    losses = {o["loss"] for _, _, o, _, _ in runs}
    caps = {o["max_iterations"] for _, _, o, _, _ in runs}
    assert losses == {rb.HUBER, rb.CAUCHY} and {0, 1, 2, 50} <= caps
    # a record that runs into the cap of 50
    assert any(a["status"] == 0 and a["iterations"] == 50 and a["trace"]["stop"] == "cap" for _, _, o, A, _ in runs for a in A if o["max_iterations"] == 50)
    # scale: automatic above the floor, the floor, given
    _, _, _, A, _ = _run(runs, "marker size 20 golden", "cauchy auto")
    assert all(a["scale_px"] == 2.5 * a["sigma_hat"] > 0.05 for a in A)
    _, _, _, A, _ = _run(runs, "noise free", "cauchy auto")
    assert all(a["scale_px"] == 0.05 and 2.5 * a["sigma_hat"] < 1e-3 and a["n_inliers"] == a["n_points"] for a in A)
    _, _, _, A, _ = _run(runs, "marker size 20 golden", "huber 0.5")
    assert all(a["scale_px"] == 0.5 for a in A)
    # tied norms at the median: the median's rank lies inside a pair of equal values
    c, _, o, A, _ = _run(runs, "tied median", "cauchy auto eval")
    norms = np.sort(np.sqrt(A[0]["s"]))
    r = (len(norms) - 1) // 2
    assert (norms == norms[r]).sum() == 2 and A[0]["sigma_hat"] == norms[r] / np.float64(rb.RAYLEIGH_MEDIAN)
    # the threshold edge: the point is an inlier under the first scale and an outlier under the second, 2e-5 a^2 away
    c = cases["threshold edge"]
    for name, inside in (("edge inside", True), ("edge outside", False)):
        for e in _run(runs, "threshold edge", name)[3:5]:
            i = c["edge_point"]
            assert bool(e[0]["inlier_mask"][i >> 5] >> (i & 31) & 1) == inside and 1e-5 < e[0]["threshold_gap"] < 3e-5
    # scale_px = 1e9 under Huber: every weight is exactly 1
    for name in ("weight one", "weight one eval"):
        for a in _run(runs, "marker size 20 golden", name)[3]:
            assert a["cost0"] == a["cost_ls0"] and a["cost"] == a["cost_ls"] and a["n_inliers"] == a["n_points"]
    # the planted outlier: the worst point, outside the inlier set under every automatic scale, before and after the loop
    w, i = m["outlier"]
    for name in ("cauchy auto", "cauchy auto eval", "huber auto", "huber auto eval"):
        a = _run(runs, "marker size 20 golden", name)[3][w]
        assert a["worst_point"] == i and not a["inlier_mask"][i >> 5] >> (i & 31) & 1 and a["max_residual_px"] > 4.0
    # a whole feature shifted: with 8 of 40 points wrong Cauchy ends with exactly the clean 32; with 8 of 80, too, and closer to the planted pose
    c = cases["feature shifted"]
    A = _run(runs, "feature shifted", "cauchy auto")[3]
    for w, a in enumerate(A):
        out = [i for i in range(a["n_points"]) if not a["inlier_mask"][i >> 5] >> (i & 31) & 1]
        assert set(c["shifted"][w]) <= set(out), (w, out)
    assert [i for i in range(80) if not A[1]["inlier_mask"][i >> 5] >> (i & 31) & 1] == list(c["shifted"][1])


def test_checker_refuses_planted_errors():
    """The statement's own record passes; a record with one planted error does not."""
    m = shp.all_cases()[0]
    w = m["outlier"][0]
    sub = dict(m, name="one", sources=m["sources"][w:w + 1])
    pp = shp.pparts_of(sub)

    def check(opts, plant, must_fail):
        want = rb.expected_of(sub, opts)
        got = np.array([rb.to_record(e) for e in rb.expected_of(sub, opts, plant=plant)])
        if not must_fail:
            return rb.check_robust_records(got, want, sub["sources"], pp)
        with pytest.raises(AssertionError):
            rb.check_robust_records(got, want, sub["sources"], pp)
    for opts in (rb.default_opts(), rb.default_opts(loss=rb.HUBER), rb.default_opts(max_iterations=0)):
        assert max(check(opts, (), False)) <= 1e-12
    check(rb.default_opts(), ("scaled cost",), True)
    check(rb.default_opts(max_iterations=0), ("scaled cost",), True)
    check(rb.default_opts(), ("upper median",), True)
    check(rb.default_opts(max_iterations=0), ("upper median",), True)
    check(rb.default_opts(), ("scale in the loop",), True)
    check(rb.default_opts(loss=rb.HUBER), ("huber without offset",), True)
    check(rb.default_opts(loss=rb.HUBER, max_iterations=0), ("huber without offset",), True)
    check(rb.default_opts(), ("unweighted jacobian",), True)
    check(rb.default_opts(loss=rb.HUBER), ("unweighted jacobian",), True)
    # s < a^2 differs from s <= a^2 only for a point exactly on the threshold: a scale whose square IS one point's s_i
    s = rb.expected_of(sub, rb.default_opts(max_iterations=0))[0]["s"]
    a = next(float(np.sqrt(v)) for v in s if np.sqrt(v) * np.sqrt(v) == v)
    on_edge = rb.default_opts(loss=rb.HUBER, max_iterations=0, scale_px=a)
    assert rb.expected_of(sub, on_edge)[0]["threshold_gap"] == 0.0
    check(on_edge, (), False)
    check(on_edge, ("strict inlier",), True)
    # a field set on a record without a pose; a moved pose on a record whose loop accepted no step
    P = sub["sources"].copy()
    P["status"] = 2
    bad = np.array([rb.to_record({"status": rb.ROBUST_NO_POSE})])
    rb.check_robust_records(bad, [{"status": rb.ROBUST_NO_POSE}], P)
    bad["n_points"] = 64
    with pytest.raises(AssertionError):
        rb.check_robust_records(bad, [{"status": rb.ROBUST_NO_POSE}], P)
    want = rb.expected_of(sub, rb.default_opts(max_iterations=0))
    bad = np.array([rb.to_record(want[0])])
    bad["tvec"][0][2] = np.nextafter(bad["tvec"][0][2], np.inf)
    with pytest.raises(AssertionError):
        rb.check_robust_records(bad, want, sub["sources"], pp)


def test_option_rules():
    good = rb.default_opts()
    assert rb.opts_ok(good) and (good["loss"], good["max_iterations"], good["scale_px"], good["auto_k"], good["min_scale_px"]) == (rb.CAUCHY, 50, 0.0, 2.5, 0.05)
    for k, v in (("loss", 2), ("loss", -1), ("max_iterations", -1), ("max_iterations", 51), ("scale_px", np.nan), ("auto_k", np.inf),
                 ("min_scale_px", -np.inf), ("auto_k", 0.0), ("min_scale_px", 0.0)):
        assert not rb.opts_ok(dict(good, **{k: v})), (k, v)
    assert rb.opts_ok(dict(good, scale_px=1.0, auto_k=0.0, min_scale_px=-1.0))


def test_struct_layouts_match_the_header():
    """ctag_robust_pose_rec and ctag_robust_opts as a C compiler lays them out, against ROBUST_POSE_DT and RobustOptsC."""
    import cylindertag_amd as ca
    from cylindertag_amd import capi
    rec = ["status", "n_points", "n_inliers", "iterations", "loss", "worst_point", "inlier_mask", "reserved", "scale_px", "sigma_hat", "cost_ls0",
           "cost_ls", "cost0", "cost", "max_residual_px", "rvec", "tvec"]
    opt = ["struct_size", "loss", "max_iterations", "reserved", "scale_px", "auto_k", "min_scale_px"]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ctag_pose.h\"\nint main(){printf(\"%zu %zu\", sizeof(ctag_robust_pose_rec), sizeof(ctag_robust_opts));\n"
    src += "".join("printf(\" %%zu\", offsetof(ctag_robust_pose_rec, %s));\n" % f for f in rec)
    src += "".join("printf(\" %%zu\", offsetof(ctag_robust_opts, %s));\n" % f for f in opt) + "return 0;}\n"
    exe = os.path.join(ROOT, "cylindertag_amd", "_build", "robust_layout")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert ca.ROBUST_POSE_DT == rb.ROBUST_POSE_DT and tuple(ca.ROBUST_POSE_DT.names) == tuple(rec)
    want = [232, C.sizeof(capi.RobustOptsC)] + [ca.ROBUST_POSE_DT.fields[f][1] for f in rec] + [getattr(capi.RobustOptsC, f).offset for f in opt]
    assert got == want and C.sizeof(capi.RobustOptsC) == 40
    assert {"ctag_robust_opts_default", "ctag_pose_robust_batch_device", "ctag_rig_pose_robust_batch_device", "ctag_mv_rig_pose_robust_batch_device",
            "ctag_estimate_pose_robust", "ctag_estimate_rig_pose_robust", "ctag_estimate_mv_rig_pose_robust"} <= set(capi.POSE_EXPORTS)


def test_log64_on_the_host(tmp_path):
    """ctm::log64 (ctag_math.h) compiled for the host without contraction: below 1 ulp from the true logarithm on log64_points, exact
    at 1, -inf at 0, NaN below 0 and for NaN, inf at inf."""
    src = tmp_path / "log64_host.cpp"
    src.write_text('#include <cstdio>\n#include "ctag_math.h"\nint main(){double x; while (std::fread(&x, 8, 1, stdin) == 1){double y = ctm::log64(x); std::fwrite(&y, 8, 1, stdout);} return 0;}\n')
    exe = tmp_path / "log64_host"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "cylindertag_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    x = np.concatenate([shp.log64_points(), [0.0, -0.0, -1.0, np.nan, np.inf]])
    out = np.frombuffer(subprocess.run([str(exe)], input=x.tobytes(), capture_output=True, check=True).stdout, np.float64)
    assert len(out) == len(x)
    worst = shp.log64_ulps(x[:-5], out[:-5])
    print("log64 on the host: worst %.3f ulp over %d arguments" % (worst, len(x) - 5))
    assert worst < 1.0 and out[list(x).index(1.0)] == 0.0
    assert out[-5] == -np.inf and out[-4] == -np.inf and np.isnan(out[-3]) and np.isnan(out[-2]) and out[-1] == np.inf
