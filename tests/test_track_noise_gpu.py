"""The track noise fit's kernels (k_track_noise.hip through include/ctag_pose.h, track noise fit) against the float64 statement of
tests/track_noise_statement.py on every batch of tests/track_noise_shapes.py.  The score call pins k_track_noise: L and sum_m2 within the
statement's measured bar per term, the counts and the status exact, and sum_m2 equal to the filter's own mahalanobis2 fields summed on
the host.  The fit is checked round by round from its trace: the candidates' values, the winner against the statement's minimum over the
device's grid, the record against the last row, and the planted noise levels recovered."""
import numpy as np
import pytest

import track_filter_shapes as fsh
import track_noise_shapes as nsh
import track_noise_statement as ns
import track_shapes as sh
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

BAR = ns.BAR


@pytest.mark.parametrize("name", nsh.BATCHES)
def test_score_matches_statement(detector, name):
    """at the batch's start values and the 16 fixed candidates (`stride`: 64 candidates x 40 rigs, every block loops over items)"""
    b, cands = nsh.batch(name), nsh.candidates(name)
    got = nsh.device_score(detector, b, cands)
    want = nsh.statement_scores(name)
    assert got.shape == (len(cands), b["n_rigs"]) and not got["reserved"].any()
    worst = {"L": 0.0, "sum_m2": 0.0}
    for c in range(len(cands)):
        for g in range(b["n_rigs"]):
            w = want[c][g]
            assert (got["n_terms"][c, g], got["n_singular"][c, g], got["status"][c, g]) == (w["n_terms"], w["n_singular"], w["status"]), (name, c, g)
            for k in worst:
                worst[k] = max(worst[k], nsh.per_term(got[k][c, g], w[k], w["n_terms"]))
    print(name, {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= BAR[k], (name, k, v, BAR[k])
    if name == "stride":   # the copies of a rig give its bytes wherever the item falls in the grid-stride loop
        for g in range(nsh.STRIDE_DISTINCT, b["n_rigs"]):
            assert got[:, g].tobytes() == got[:, g % nsh.STRIDE_DISTINCT].tobytes()
    if name == "bad_rig":
        assert (got["status"][:, 1] == capi.NOISE_BAD_INPUT).all() and not got["L"][:, 1].any() and not got["n_terms"][:, 1].any()
    if name == "overflow":
        assert got["n_singular"][:, 0].any() and not got["n_singular"][:, 0].all() and not got["n_singular"][:, 1].any()


@pytest.mark.parametrize("name", ("n129", "gaps", "spin", "mv", "planted_times"))
def test_sum_m2_is_the_filters_mahalanobis2_summed_in_frame_order(detector, name):
    """at theta = (the options' q, s = 1) the walk is the filter's: exact"""
    b = nsh.batch(name)
    o = ns.noise_opts(b)
    got = nsh.device_score(detector, b, np.array([[o["q_rot"], o["q_trans"], 1.0]]))[0]
    with fsh.DeviceFilter(detector, b, loss=2, gate=0.0, max_gap=o["max_gap"], q_rot=o["q_rot"], q_trans=o["q_trans"]) as F:
        rec = F.run(b)
    for g in range(b["n_rigs"]):
        s, n = 0.0, 0
        for f in range(b["n_frames"]):
            upd = rec["status"][f, g] == capi.TRACK_OK and (rec["flags"][f, g] & capi.TRACK_FLAG_MEASURED) and not (rec["flags"][f, g] & capi.TRACK_FLAG_STARTED)
            if upd:
                s, n = s + rec["mahalanobis2"][f, g], n + 1
        assert got["n_terms"][g] == n and got["sum_m2"][g] == s, (name, g)


def check_fit_against_statement(b, rec, trace, q, rigs, **over):
    """search q of a device fit, from its trace: every round's candidates and winner, then the record"""
    o = ns.noise_opts(b, **over)
    axes, start = ns.free_axes(o["free_mask"]), nsh.start_of(b, **over)
    meas = {g: ns.measurements(b, g) for g in rigs}
    good = [g for g in rigs if meas[g] is not None]
    memo = {}

    def at(v):
        key = tuple(float(x) for x in v)
        if key not in memo:
            memo[key] = ns.pooled([ns.score_rig(b, g, v, o, np.float64, meas[g]) for g in good])
        return memo[key]

    uc, n_terms_max = np.zeros(3), 1
    for r in range(o["rounds"]):
        row, h = trace[q, r], ns.step_of(o, r)
        U = ns.grid_u(uc, h, axes)
        win = int(row["winner"])
        assert 0 <= win < len(U) and not row["reserved"]
        assert (row["u"] == U[win]).all(), (r, row["u"], U[win])
        want_v = start * np.exp2(U[win])
        assert (np.abs(row["value"] - want_v) <= 4 * np.spacing(want_v)).all(), (r, row["value"], want_v)   # start * 2^u to 4 ulp
        res = [at(v) for v in ns.values_of(start, U)]
        ok = [x["n_singular"] == 0 for x in res]
        assert ok[win]
        n_terms_max = max(x["n_terms"] for x in res)
        best = min(x["L"] for x, k in zip(res, ok) if k)
        # the device's winner is the statement's minimum over this grid, within the bar on each of the two
        assert res[win]["L"] - best <= 2 * BAR["L"] * max(1, n_terms_max), (r, win, res[win]["L"], best)
        assert nsh.per_term(row["L"], res[win]["L"], res[win]["n_terms"]) <= BAR["L"]
        uc = U[win]
    last, R = trace[q, o["rounds"] - 1], rec[q]
    assert R["status"] == capi.NOISE_OK and R["rounds"] == o["rounds"] and R["n_free"] == len(axes)
    assert (R["q_rot"], R["q_trans"], R["cov_scale"]) == tuple(last["value"]) and R["score"] == last["L"]
    w = res[win]
    assert R["n_terms"] == w["n_terms"] and nsh.per_term(R["score_start"], at(start)["L"], at(start)["n_terms"]) <= BAR["L"]
    assert abs(R["mean_m2"] - w["sum_m2"] / w["n_terms"]) <= BAR["sum_m2"] + 4 * np.spacing(R["mean_m2"])
    # log2_sigma and the flags from the statement's L on the device's last grid: with every L within dL = BAR n_terms the curvature is within
    # 4 dL / h^2, and sigma = sqrt(2 / c) moves by sigma / 2 x that / c
    Ls, sing = [x["L"] for x in res], [x["n_singular"] for x in res]
    sig, flags = ns.curvature_sigma(Ls, sing, win, h, axes)
    assert R["flags"] == flags
    for a in range(3):
        if sig[a] == 0:
            continue   # (a curvature within its own error of 0 may fall on either side)
        c = 2.0 / sig[a] ** 2
        dc = 4 * BAR["L"] * max(1, n_terms_max) / (h * h)
        assert dc < 0.5 * c and abs(R["log2_sigma"][a] - sig[a]) <= sig[a] * dc / c, (a, R["log2_sigma"], sig)
    for a in range(3):
        if a not in axes:
            assert R["log2_sigma"][a] == 0.0


def test_fit_round_by_round_q(detector):
    b = nsh.select_rigs(nsh.batch("planted_s1"), [2, 0])
    over = dict(free_mask=3, rounds=4, cov_scale=1.0)
    rec, trace = nsh.device_fit(detector, b, **over)
    assert rec.shape == (2,) and trace.shape == (2, 4) and (rec["rig"] == [0, 1]).all()
    check_fit_against_statement(b, rec, trace, 1, [1], **over)


def test_fit_round_by_round_all_three_on_40_frames(detector):
    b = nsh.select_rigs(nsh.batch("planted_s4"), [2])
    b = dict(b, n_frames=40, **{k: b[k][:40] for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov", "rec_rig", "rec_frame")})
    over = dict(free_mask=7, rounds=2, span=8.0)
    rec, trace = nsh.device_fit(detector, b, **over)
    check_fit_against_statement(b, rec, trace, 0, [0], **over)


def test_fit_pooled_round_by_round(detector):
    b = nsh.batch("planted_times")
    over = dict(free_mask=4, rounds=6, mode=ns.POOLED, q_rot=b["planted"][0], q_trans=b["planted"][1])
    rec, trace = nsh.device_fit(detector, b, **over)
    assert rec.shape == (1,) and rec["rig"][0] == -1
    check_fit_against_statement(b, rec, trace, 0, [0, 1, 2], **over)


def recovered(b, rec, axes):
    """the condition of the statement's own recovery test"""
    for R in rec:
        assert R["status"] == capi.NOISE_OK and R["flags"] == 0
        u = np.log2(np.array([R["q_rot"], R["q_trans"], R["cov_scale"]]) / b["planted"])
        print(b["name"], axes, "u", u, "log2_sigma", R["log2_sigma"], "mean_m2", R["mean_m2"])
        for a in axes:
            assert R["log2_sigma"][a] > 0 and abs(u[a]) <= 4.0 * R["log2_sigma"][a]
        assert abs(R["mean_m2"] - 6.0) <= 1.0


@pytest.mark.parametrize("name", nsh.PLANTED_BATCHES)
def test_planted_noise_recovered_on_the_device(detector, name):
    """the default search (three free axes, 10 rounds, 125 candidates), per rig and pooled, from starts 3, 2 and 1 octaves off"""
    b = nsh.batch(name)
    rec = nsh.device_fit(detector, b, trace=False)
    recovered(b, rec, (0, 1, 2))
    recovered(b, nsh.device_fit(detector, b, trace=False, mode=ns.POOLED), (0, 1, 2))


def test_fit_with_no_free_axis_scores_the_start_values(detector):
    b = nsh.batch("n65")
    rec, trace = nsh.device_fit(detector, b, free_mask=0, rounds=3)
    sc = nsh.device_score(detector, b, nsh.start_of(b)[None, :])[0]
    for g in range(b["n_rigs"]):
        R = rec[g]
        assert R["status"] == capi.NOISE_OK and R["n_free"] == 0 and R["flags"] == 0 and not R["log2_sigma"].any() and R["rounds"] == 3
        assert (R["q_rot"], R["q_trans"], R["cov_scale"]) == tuple(nsh.start_of(b))
        assert R["score"] == R["score_start"] == sc["L"][g] and R["n_terms"] == sc["n_terms"][g] and R["mean_m2"] == sc["sum_m2"][g] / sc["n_terms"][g]
        assert (trace["winner"][g] == 0).all() and (trace["L"][g] == sc["L"][g]).all()
