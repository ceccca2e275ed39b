"""The track filter's statement (tests/track_filter_statement.py) held to what does not depend on it: its Jacobians to central
differences, its result to the smoother's statement where the model is linear, its covariance to the scatter of its own errors, and
the float64-against-longdouble figures the device bars are made of."""
import numpy as np
import pytest

import track_filter_shapes as fsh
import track_filter_statement as fs
import track_shapes as sh
import track_statement as ts

T = np.float64


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(3)
    o = dict(fs.DEFAULTS)
    for trial in range(6):
        R = ts.so3_exp(rng.uniform(-1, 1, 3))
        t, v = rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3)
        w = rng.uniform(-1, 1, 3) * (30.0 if trial % 2 else 2.0)   # D |w| up to about a radian
        D = T(1.0 / 30.0)
        E, F, _ = fs.transition(w, D, o, T)

        def propagate(d):
            """the state perturbed by d (theta on the left), propagated, and its difference from the nominal in the same chart"""
            R1, w1 = ts.so3_exp(d[0:3]) @ R, w + d[6:9]
            Rn, tn = ts.so3_exp(D * w1) @ R1, t + d[3:6] + D * (v + d[9:12])
            return np.concatenate([ts.so3_log(Rn @ (E @ R).T), tn - (t + D * v), d[6:9], d[9:12]])

        h = 1e-6
        num = np.stack([(propagate(h * np.eye(12)[k]) - propagate(-h * np.eye(12)[k])) / (2 * h) for k in range(12)], 1)
        assert np.abs(num - F).max() < 1e-8, np.abs(num - F).max()
        # H: e(Exp(d) R-, t- + d) - e
        Rm, tm = ts.so3_exp(ts.so3_log(R) + rng.uniform(-0.3, 0.3, 3)), t + rng.uniform(-0.1, 0.1, 3)
        e0, H = fs.observation(R, t, Rm, tm, T)

        def resid(d):
            return fs.observation(ts.so3_exp(d[0:3]) @ R, t + d[3:6], Rm, tm, T)[0]

        numH = np.stack([(resid(h * np.eye(12)[k]) - resid(-h * np.eye(12)[k])) / (2 * h) for k in range(12)], 1)
        assert np.abs(numH - H).max() < 1e-8, np.abs(numH - H).max()
    # Jl Jl^-1 = I, through the series' threshold too
    for th in (1e-9, 1e-3, 0.0999, 0.1001, 1.0, 3.0):
        p = th * np.array([0.6, -0.64, 0.48])
        assert np.abs(fs.so3_jl(p) @ ts.so3_jlinv(p) - np.eye(3)).max() < 1e-13


LINK_PREFIXES = (1, 2, 3, 9, 17, 64)


def linear_batch(n, seed):
    """translation-only motion, one constant measured rotation, covariances without rotation-translation coupling: the model is linear"""
    rng = np.random.default_rng(seed)
    b = sh.make_batch("linear%d" % n, seed, n, [np.ones(n, bool)], ["good"], opts=dict(max_iterations=3, lambda0=0.0))
    for f in range(n):
        b["rvec"][f, 0] = b["rvec"][0, 0]
        c = np.array(b["cov"][f, 0], copy=True)
        c[0:3, 3:6] = c[3:6, 0:3] = 0.0
        b["cov"][f, 0] = c
    return b


def link_figures(Tt):
    out = []
    for n in LINK_PREFIXES:
        b = linear_batch(n, 50 + n)
        out.append((fs.run_batch(b, Tt), ts.smooth(b, Tt)[0]))
    return out


def last(rec):
    return {k: np.asarray(v)[-1:] for k, v in rec.items()}


def test_link_to_the_smoother():
    """at the last frame of a batch the filter has seen what the smoother has: where the model is linear the two records agree"""
    f64, ld = link_figures(np.float64), link_figures(np.longdouble)
    measured = {k: 0.0 for k in fs.LINK_BAR}
    for (a, s), (al, sl) in zip(f64, ld):
        for got, want in ((a, al), (s, sl)):
            d = fs.deviation(last(got), last(want))
            for k in measured:
                measured[k] = max(measured[k], d[k])
    print("MEASURED_LINK_DEVIATION =", {k: float("%.3g" % v) for k, v in measured.items()})
    for n, (a, s) in zip(LINK_PREFIXES, f64):
        assert a["status"][-1, 0] == fs.OK and s["status"][-1, 0] == ts.OK
        d = fs.deviation(last(a), last(s))
        print("link", n, {k: "%.3g" % d[k] for k in fs.LINK_BAR})
        for k in fs.LINK_BAR:
            assert d[k] <= fs.LINK_BAR[k], (n, k, d[k], fs.LINK_BAR[k])


def test_distance_to_the_smoother_on_general_batches():
    """information, not a bar: the filter's last tracked frame against the smoother's, in the smoother's sigma"""
    for name in ("noise", "mv"):
        b = sh.batch(name)
        a, s = fs.run_batch(b), sh.full_lm(name)[0]
        for g in range(b["n_rigs"]):
            fr = [f for f in range(b["n_frames"]) if a["status"][f, g] == fs.OK and s["status"][f, g] == ts.OK]
            if fr:
                f = fr[-1]
                sd = np.sqrt(np.diag(s["cov"][f, g]))
                d = np.concatenate([a["rvec"][f, g] - s["rvec"][f, g], a["tvec"][f, g] - s["tvec"][f, g]]) / sd
                print("to the smoother", name, "rig", g, "frame", f, "worst %.3g sigma" % np.abs(d).max())


def test_calibration():
    """one frame from each of 480 independent 8-frame tracks: the mean of delta^T cov^-1 delta is 6 within 6 +- 0.63 (DESIGN section 21's band)"""
    b = sh.calibration_batch()
    rec = fs.run_batch(b)
    vals = []
    for g in range(b["n_rigs"]):
        for a, e in ts.pieces([b["pose_status"][f, g] == 0 for f in range(b["n_frames"])], fs.filter_opts(b)["max_gap"]):
            assert rec["status"][e, g] == fs.OK and rec["flags"][a, g] & fs.FLAG_STARTED
            d = np.concatenate([ts.so3_log(ts.so3_exp(rec["rvec"][e, g]) @ b["true_R"][e, g].T), rec["tvec"][e, g] - b["true_t"][e, g]])
            vals.append(d @ np.linalg.solve(rec["cov"][e, g], d))
    assert len(vals) == 480
    print("calibration mean %.3f" % np.mean(vals))
    assert abs(np.mean(vals) - 6.0) <= 0.63


def test_structure_of_the_statement_on_the_batches():
    """what the batches are for happens in them: drops, restarts, gating, downweighting, bad input"""
    g = fsh.statement("gate")
    f, r = fsh.batch("gate")["planted"]
    assert g["flags"][f, r] == fs.FLAG_MEASURED | fs.FLAG_GATED and g["status"][f, r] == fs.OK and g["weight"][f, r] == 0
    run = fsh.statement("gated_run")
    assert list(run["status"][20:25, 0]) == [fs.OK] * 3 + [fs.NOT_TRACKED, fs.OK] and run["flags"][24, 0] == fs.FLAG_MEASURED | fs.FLAG_STARTED
    for name in ("huber", "cauchy"):
        h = fsh.statement(name)
        assert h["flags"][f, r] == fs.FLAG_MEASURED | fs.FLAG_DOWNWEIGHTED and h["weight"][f, r] < 1
    gp = fsh.statement("gaps")
    assert (gp["flags"][:, 0] & fs.FLAG_STARTED).astype(bool).sum() == len(ts.pieces(fsh.batch("gaps")["pose_status"][:, 0] == 0, fsh.MG))
    assert (gp["flags"][:, 1] & fs.FLAG_STARTED).astype(bool).sum() == 2
    bad = fsh.statement("bad_rig")
    assert (bad["status"][:, 1] == fs.BAD_INPUT).all() and (bad["status"][:, 0] == fs.OK).all()
    ht = fsh.statement("half_turn")
    assert np.pi - np.linalg.norm(fsh.batch("half_turn")["rvec"][12, 0]) < 1e-3 and (ht["status"] == fs.OK).all()
    sp = fsh.batch("spin")
    assert 0.5 < np.median(np.linalg.norm(fsh.statement("spin")["w"][5:, 0], axis=1)) / 30.0 < 2.0 and sp["n_frames"] == 50


def test_split_invariance_of_the_statement():
    b = fsh.batch("n129")
    whole = fsh.statement("n129")
    F = fs.Filter(b["n_rigs"], fs.filter_opts(b))
    parts = [F.run(fs.frames_slice(b, a, e)) for a, e in ((0, 63), (63, 129))]
    for k in sh.FIELDS:
        assert np.concatenate([p[k] for p in parts]).tobytes() == np.asarray(whole[k]).tobytes(), k


def test_f64_deviation():
    """-k deviation: float64 against longdouble over every batch; prints the dict track_filter_statement.py carries"""
    measured = {k: 0.0 for k in fs.MEASURED_F64_DEVIATION}
    for name in fsh.BATCHES:
        a, l = fsh.statement(name), fsh.statement(name, True)
        assert (a["status"] == l["status"]).all() and (a["flags"] == l["flags"]).all(), name
        d = fs.deviation(a, l)
        print(name, {k: "%.3g" % v for k, v in d.items()})
        for k in measured:
            measured[k] = max(measured[k], d[k])
    print("MEASURED_F64_DEVIATION =", {k: float("%.3g" % v) for k, v in measured.items()})
    for k, v in measured.items():
        assert v <= fs.MEASURED_F64_DEVIATION[k] * 1.01, (k, v)  # the figures in the file are this test's output, to three digits
