"""GPU tests of the rig assembly's kernels through the probe ctag_testkit_rig_fit_system (k_rfit_record, k_fit_assemble<96>,
k_fit_solve<96> at a given state): S, g and delta of every rig of every batch of tests/rig_fit_shapes.py against the independent statement at the
rule-2 start and at one perturbed state, the pass-size independence of rule 6, a pivot that is not positive, and the limits."""
import numpy as np
import pytest

import cylindertag_amd as ca
import model_fit_statement as ms
import pose_statement as ps
import rig_fit_shapes as sh
import rig_fit_statement as rf
import testkit as tk
from rig_fit_testlib import Detectors, device_rig_poses, model_at

pytestmark = pytest.mark.gpu
LAMBDA = 1e-3


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "state": {}}
    yield e
    e["dets"].close()


def _perturbed(b, A, X0):
    """The rule-2 start with every placed model but the anchors moved by about 1e-3 rad and 0.1 mm, as float32 values."""
    rng = np.random.default_rng(5)
    T = {}
    for g, rig in A["rigs"].items():
        for m in rig["placed"]:
            if m != rig["anchor"]:
                c = X0[m].mean(0)
                R = ps.rodrigues(rng.normal(0, 1e-3, 3))
                T[m] = (R, c - R @ c + rng.normal(0, 0.1, 3))
    return rf.layout(X0.astype(np.float32), T)


def _state(env, name, which):
    """The batch at a state: (batch, detector, camera, Model, Rigs, device rig-pose records, the statement's observations on them)."""
    key = (name, which)
    if key not in env["state"]:
        b, A = sh.batch(name), sh.assembled(name)
        X = A["X0"] if which == "start" else _perturbed(b, A, A["X0"])
        det, cam, M = env["dets"].of(b), ca.make_camera(b["K"], b["dist"]), model_at(b, X)
        rigs = ca.Rigs(M, A["rig_placed"], b["n_rigs"])
        recs = device_rig_poses(det, b["recs"], M, rigs, cam)
        obs = rf.rig_observations(b["recs"], dict(b["model"], corners=X.astype(np.float32)), A["rig_placed"], b["n_rigs"], sh.camera_of(b),
                                  ok_of=lambda w: recs[w]["status"] == 0)
        assert [o is not None for o in obs] == [o is not None for o in A["obs"]], "an item the statement counts has no rig pose at this state"
        env["state"][key] = (b, A, det, cam, M, rigs, recs, obs, X)
    return env["state"][key]


def test_limits_are_the_shapes_files():
    lim = tk.rig_fit_limits()
    assert lim["record_grid"] == sh.RECORD_GRID and lim["pass_records"] == sh.PASS_RECORDS


@pytest.mark.parametrize("which", ["start", "perturbed"])
@pytest.mark.parametrize("name", sh.NAMES)
def test_system_against_the_statement(env, name, which):
    """S, g and delta of every rig with observations; deviations scaled as ms.system_deviation scales them, within 16 x the float64
    statement's own error against long double (rf.SYSTEM_BAR)."""
    b, A, det, cam, M, rigs, recs, obs, X = _state(env, name, which)
    P = b["model"]["size"] * 8
    worst = np.zeros(3)
    for g, rig in A["rigs"].items():
        B = ms.Batch(obs, g, sh.camera_of(b))
        if rig["anchor"] < 0 or not B.recs:
            continue
        got = det.rig_fit_system(b["recs"], recs, M, rigs, cam, g, LAMBDA)
        N = 6 * len(rig["placed"])
        assert got["S"].shape == (N, N) and not got["bad_pivot"]
        state = np.array([np.concatenate([recs[o["w"]]["rvec"], recs[o["w"]]["tvec"]]) for o in B.recs])
        S, gv = rf.reduced_system(B, X.reshape(-1, 3), state, rig["placed"], P)
        dropped = np.array([m == rig["anchor"] for m in rig["placed"]])
        d, pd = rf.step(S, gv, dropped, LAMBDA)
        assert pd
        cost = float(sum(recs[o["w"]]["cost"] for o in B.recs))
        dev = np.array(rf.system_deviation(got["S"], got["g"], got["delta"], S, gv, d, cost))
        worst = np.maximum(worst, dev)
        assert (got["S"] == got["S"].T).all()
        assert not got["delta"].reshape(-1, 6)[dropped].any(), "the anchor moves"
        assert got["delta"].reshape(-1, 6)[~dropped].all(1).all()
    print("%s %s: S %.2e g %.2e delta %.2e (bars %.2e %.2e %.2e)" % ((name, which) + tuple(worst) + tuple(rf.SYSTEM_BAR[k] for k in ("S", "g", "delta"))))
    for k, v in zip(("S", "g", "delta"), worst):
        assert v <= rf.SYSTEM_BAR[k], (k, v)


@pytest.mark.parametrize("name", sh.NAMES)
def test_the_pass_size_changes_no_bit(env, name):
    """Rule 6, every rig with observations: the workspace processed 7 or 100 records a pass, or all of them in ONE pass (batch (f) takes
    two passes of its own accord); and a second call."""
    b, A, det, cam, M, rigs, recs, obs, X = _state(env, name, "start")
    n_obs = sum(o is not None for o in obs)
    checked = 0
    for g, rig in A["rigs"].items():
        if rig["anchor"] < 0 or not any(o is not None and o["rig"] == g for o in obs):
            continue
        ref = det.rig_fit_system(b["recs"], recs, M, rigs, cam, g, LAMBDA)
        again = det.rig_fit_system(b["recs"], recs, M, rigs, cam, g, LAMBDA)
        for pass_records in (7, 100, n_obs):
            got = det.rig_fit_system(b["recs"], recs, M, rigs, cam, g, LAMBDA, pass_records=pass_records)
            for k in ("S", "g", "delta"):
                assert got[k].tobytes() == ref[k].tobytes() == again[k].tobytes(), (g, k, pass_records)
        assert np.abs(ref["S"]).max() > 0
        checked += 1
    assert checked == len(b["claims"]["n_placed"])


def test_a_pivot_that_is_not_positive_is_reported(env):
    b, A, det, cam, M, rigs, recs, obs, X = _state(env, sh.NAMES[0], "start")
    got = det.rig_fit_system(b["recs"], recs, M, rigs, cam, 0, -2.0)   # S - 2 diag S is indefinite
    assert got["bad_pivot"] and not got["delta"].any()
    assert not det.rig_fit_system(b["recs"], recs, M, rigs, cam, 0, 0.5)["bad_pivot"]
