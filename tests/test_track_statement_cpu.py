"""tests/track_statement.py held to itself and to scipy, without a GPU: its two solution routes against each other, its loop against
scipy's minimum of the same cost, planted errors it must tell from the real thing, the calibration of the covariance it reports on
tracks drawn from the model, and the float64-to-longdouble deviation its bars are made of."""
import numpy as np
import pytest

import track_shapes as sh
import track_statement as ts


def exceeds(dev, bar):
    return any(dev[k] > bar[k] for k in dev)


def test_pieces_and_start():
    m = np.zeros(30, bool)
    m[[2, 3, 7, 12, 13, 20]] = True
    assert ts.pieces(m, 4) == [(2, 7), (12, 13), (20, 20)]
    assert ts.pieces(m, 5) == [(2, 13), (20, 20)]
    assert ts.pieces(np.zeros(5, bool), 3) == []
    b = sh.batch("gaps")
    meas, pcs = ts.batch_pieces(b)[0]
    assert pcs == [(3, 99)] and meas[101] is None   # a pose without a usable covariance is unmeasured
    a, e = pcs[0]
    P = ts.Piece(meas[a:e + 1], ts.batch_times(b, np.float64)[a:e + 1], ts.batch_opts(b), np.float64)
    R, x = P.start()
    k = 8   # frame 11: the middle of the gap 10 .. 12 between measured 9 and 13
    s = (P.t[k] - P.t[6]) / (P.t[10] - P.t[6])
    assert np.allclose(x[k][0:3], meas[9][1] + s * (meas[13][1] - meas[9][1]), rtol=0, atol=1e-15)
    assert np.allclose(R[k], ts.so3_exp(s * ts.so3_log(meas[13][0] @ meas[9][0].T)) @ meas[9][0], rtol=0, atol=1e-15)
    assert (x[-1][3:9] == x[-2][3:9]).all()
    one = ts.Piece([meas[a]], [0.0], ts.batch_opts(b), np.float64).run()
    assert one["cost"] == 0 and np.allclose(one["S"][0][0:6, 0:6], b["cov"][a, 0], rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", ("noise", "gaps"))
def test_dense_and_chain_routes_agree(name):
    """the plain inverse of the whole matrix against the chain's backward recursion, on pieces up to 97 frames"""
    b = sh.with_opts(sh.batch(name), max_iterations=1, lambda0=0.0)
    d, sd, _ = ts.smooth(b, dense=True)
    c, sc, _ = ts.smooth(b, dense=False)
    dev = ts.deviation(d, c, sc, sd)
    print(name, dev)
    assert not exceeds(dev, ts.BAR_STEP)


@pytest.mark.parametrize("name", sh.SCIPY_BATCHES)
def test_lm_reaches_scipy_minimum(name):
    """the loop of rule 6 and scipy's trust-region least squares on rule 4's residual vector end in the same minimum: the costs agree to
    1e-9, the states to a ten-thousandth of a sigma (scipy stops on a finite-difference Jacobian; the measured distance is recorded as
    track_statement.MEASURED_LM_TO_SCIPY)"""
    lm, slm, _ = sh.full_lm(name)
    sp, ssp, _ = sh.scipy_min(name)
    dev = ts.deviation(lm, sp, ssp, slm)
    print(name, "LM to scipy", dev)
    assert (lm["status"] == sp["status"]).all() and (lm["flags"] == sp["flags"]).all()
    assert dev["cost"] < 1e-9 and max(dev["pose"], dev["vel"]) <= 1e-4
    assert max(dev["pose"], dev["vel"]) <= ts.SCIPY_BAR
    if name in ("huber", "cauchy"):
        f, g = sh.batch(name)["planted"]
        assert lm["weight"][f, g] < 0.5 and lm["flags"][f, g] == ts.FLAG_MEASURED | ts.FLAG_DOWNWEIGHTED


class SignSwapped(ts.Piece):
    def motion_residual(self, R, x, k):
        dt, psi, r = super().motion_residual(R, x, k)
        r = r.copy()
        r[0:3] = psi + dt * x[k][3:6]
        return dt, psi, r


class PriorAtEnd(ts.Piece):
    def prior_at(self):
        return self.n - 1


def as_mutant(cls):
    return lambda P: cls(P.meas, P.t, P.o, P.T).run()


def test_planted_errors_are_rejected():
    """each of four wrong readings of the rules, run as the kernels would be, misses the statement by more than the bar"""
    b = sh.with_opts(sh.batch("gaps"), max_iterations=1, lambda0=0.0)
    want, wstat, table = sh.single_step("gaps")
    for label, cls in (("a swapped sign in a", SignSwapped), ("the velocity prior on the last frame", PriorAtEnd)):
        got, gstat, _ = ts.smooth(b, runner=as_mutant(cls))
        dev = ts.deviation(got, want, wstat, gstat)
        print(label, dev)
        assert exceeds(dev, ts.BAR), label
    # W used where cov is meant: the measurement weighted by its covariance instead of its inverse
    c = dict(b, cov=np.array(b["cov"], copy=True))
    ok = (b["pose_status"] == 0) & (b["cov_status"] == 0)
    c["cov"][ok] = np.linalg.inv(b["cov"][ok])
    got, gstat, _ = ts.smooth(c)
    assert exceeds(ts.deviation(got, want, wstat, gstat), ts.BAR)
    # a gap of max_gap + 1 bridged
    got, gstat, gtable = ts.smooth(sh.with_opts(b, max_gap=b["opts"]["max_gap"] + 1))
    assert gtable != table and (got["status"] != want["status"]).any()


def test_calibration_on_model_drawn_tracks():
    """delta^T cov^-1 delta against the truth, delta = [Log(R R_true^T); t - t_true], is chi-square with 6 degrees of freedom at every
    tracked frame when the tracks come from the model.  The frames of one piece are correlated, the pieces are independent draws: ONE
    frame a piece (its middle one) gives N independent chi-square(6) values, whose mean has variance 12 / N exactly.  With N = 480 pieces
    the mean is held to 6 +- 4 sqrt(12 / 480) = 6 +- 0.632: a covariance wrong by a factor 1.2 (mean 5.0 or 7.2) is 6 sigma off."""
    b = sh.calibration_batch()
    rec, stat, table = ts.smooth(b)
    one, every = [], []
    for g, pcs in enumerate(table):
        for a, e in pcs:
            for f in range(a, e + 1):
                assert rec["status"][f, g] == ts.OK
                R = ts.so3_exp(rec["rvec"][f, g])
                d = np.concatenate([ts.so3_log(R @ b["true_R"][f, g].T), rec["tvec"][f, g] - b["true_t"][f, g]])
                m2 = d @ np.linalg.solve(rec["cov"][f, g], d)
                every.append(m2)
                if f == (a + e) // 2:
                    one.append(m2)
    N, mean = len(one), float(np.mean(one))
    half = 4.0 * np.sqrt(12.0 / N)
    print("calibration: mean %.3f over one frame of each of %d pieces (all %d frames: %.3f), allowed 6 +- %.3f" % (mean, N, len(every), np.mean(every), half))
    assert N == 16 * 30 and abs(mean - 6.0) <= half


def test_f64_deviation():
    """measures MEASURED_F64_DEVIATION(_STEP) again; the float64 statement itself must pass the bars made from them"""
    step = {k: 0.0 for k in ts.MEASURED_F64_DEVIATION}
    every = dict(step)
    for name in sh.BATCHES:
        for mode, fn in (("step", sh.single_step), ("lm", sh.full_lm)):
            if name == "long" and mode == "lm":
                continue
            r, s, _ = fn(name)
            rl, sl, _ = fn(name, True)
            assert (r["status"] == rl["status"]).all() and (r["flags"] == rl["flags"]).all()
            d = ts.deviation(r, rl, sl, s)
            for k in d:
                every[k] = max(every[k], d[k])
                if mode == "step":
                    step[k] = max(step[k], d[k])
    print("MEASURED_F64_DEVIATION_STEP", step)
    print("MEASURED_F64_DEVIATION", every)
    assert not exceeds(step, ts.BAR_STEP) and not exceeds(every, ts.BAR)
    assert all(ts.BAR_STEP[k] <= ts.BAR[k] for k in ts.BAR)
