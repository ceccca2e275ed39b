"""GPU tests of the model reconstruction's kernels through the probe ctag_testkit_model_fit_system (k_mfit_record, k_mfit_assemble,
k_mfit_solve at a given state): S, g and delta of every model of every batch of tests/model_fit_shapes.py against the independent
statement, the pass-size independence of rule 7, a pivot that is not positive, and the held corners' rows."""
import numpy as np
import pytest

import cylindertag_amd as ca
import model_fit_shapes as sh
import model_fit_statement as ms
import testkit as tk
from model_fit_testlib import Detectors, device_poses, model_of

pytestmark = pytest.mark.gpu
LAMBDA = 1e-3


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "state": {}}
    yield e
    e["dets"].close()


def _state(env, name):
    """The batch at its seed: device pose records, the statement's observations (the records the device posed) and held mask."""
    if name not in env["state"]:
        b = sh.batch(name)
        det, M, cam = env["dets"].of(b), model_of(b["seed"]), ca.make_camera(b["K"], b["dist"])
        poses = device_poses(det, b["recs"], M, cam)
        obs = ms.observations(b["recs"], b["seed"], sh.camera_of(b), ok_of=lambda w: poses[w]["status"] == 0)
        n, P = len(b["seed"]["ids"]), b["seed"]["size"] * 8
        assert [o is not None for o in obs] == [o is not None for o in sh.observed(name)[0]], "a record the statement counts has no pose under the seed"
        env["state"][name] = (b, det, M, cam, poses, obs, ms.held_mask(obs, n, P, b["min_obs"]))
    return env["state"][name]


def test_limits_are_the_shapes_files():
    assert tk.model_fit_limits()["record_grid"] == sh.RECORD_GRID


@pytest.mark.parametrize("name", sh.NAMES)
def test_system_against_the_statement(env, name):
    """S, g, delta and the held mask of every model with observations; deviations scaled as ms.system_deviation scales them, within
    16 x the float64 statement's own error against long double (ms.SYSTEM_BAR)."""
    b, det, M, cam, poses, obs, held = _state(env, name)
    P = b["seed"]["size"] * 8
    worst = np.zeros(3)
    for m in range(len(b["seed"]["ids"])):
        B = ms.Batch(obs, m, sh.camera_of(b))
        if not B.recs:
            continue
        got = det.model_fit_system(b["recs"], poses, M, cam, m, LAMBDA, min_obs=b["min_obs"])
        assert (got["held"] == held[m]).all() and not got["bad_pivot"]
        if held[m].all():
            continue
        state = np.array([np.concatenate([poses[o["w"]]["rvec"], poses[o["w"]]["tvec"]]) for o in B.recs])
        seed = b["seed"]["corners"][m].astype(np.float64)
        S, g = ms.reduced_system(B, seed, state, P)
        d, pd = ms.step(S, g, held[m], LAMBDA)
        assert pd
        cost = float(sum(poses[o["w"]]["cost"] for o in B.recs))
        dev = np.array(ms.system_deviation(got["S"], got["g"], got["delta"], S, g, d, held[m], cost))
        worst = np.maximum(worst, dev)
        assert (got["S"] == got["S"].T).all()
        assert not got["delta"].reshape(P, 3)[held[m]].any(), "a held corner moves"
        unseen = ~np.abs(np.diag(S)).reshape(P, 3).any(1)
        assert not got["S"].reshape(P, 3, P, 3)[unseen].any() and not got["g"].reshape(P, 3)[unseen].any()
    print("%s: S %.2e g %.2e delta %.2e (bars %.2e %.2e %.2e)" % ((name,) + tuple(worst) + tuple(ms.SYSTEM_BAR[k] for k in ("S", "g", "delta"))))
    for k, v in zip(("S", "g", "delta"), worst):
        assert v <= ms.SYSTEM_BAR[k], (k, v)


@pytest.mark.parametrize("name", [sh.NAMES[1], sh.NAMES[4]])
def test_the_pass_size_changes_no_bit(env, name):
    """Rule 7: the workspace processed 7 or 100 records a pass, or all at once."""
    b, det, M, cam, poses, obs, held = _state(env, name)
    m = 1
    ref = det.model_fit_system(b["recs"], poses, M, cam, m, LAMBDA, min_obs=b["min_obs"])
    again = det.model_fit_system(b["recs"], poses, M, cam, m, LAMBDA, min_obs=b["min_obs"])
    for pass_records in (7, 100):
        got = det.model_fit_system(b["recs"], poses, M, cam, m, LAMBDA, min_obs=b["min_obs"], pass_records=pass_records)
        for k in ("S", "g", "delta"):
            assert got[k].tobytes() == ref[k].tobytes() == again[k].tobytes(), (k, pass_records)
    assert np.abs(ref["S"]).max() > 0


def test_a_pivot_that_is_not_positive_is_reported(env):
    b, det, M, cam, poses, obs, held = _state(env, sh.NAMES[0])
    B = ms.Batch(obs, 0, sh.camera_of(b))
    got = det.model_fit_system(b["recs"], poses, M, cam, 0, -2.0, min_obs=b["min_obs"])   # S - 2 diag S is indefinite
    assert got["bad_pivot"] and not got["delta"].any()
    state = np.array([np.concatenate([poses[o["w"]]["rvec"], poses[o["w"]]["tvec"]]) for o in B.recs])
    S, g = ms.reduced_system(B, b["seed"]["corners"][0].astype(np.float64), state, b["seed"]["size"] * 8)
    assert not ms.step(S, g, held[0], -2.0)[1]
    assert not det.model_fit_system(b["recs"], poses, M, cam, 0, 0.5, min_obs=b["min_obs"])["bad_pivot"]


def test_held_corners_follow_min_obs(env):
    """The corners of model 0 of the first batch seen by exactly 1, 2 and 3 records: held or fitted as min_obs says, rows 0 when held."""
    b, det, M, cam, poses, obs, _ = _state(env, sh.NAMES[0])
    P = b["seed"]["size"] * 8
    for min_obs in (1, 2, 3, 4):
        got = det.model_fit_system(b["recs"], poses, M, cam, 0, LAMBDA, min_obs=min_obs)
        want = ms.held_mask(obs, len(b["seed"]["ids"]), P, min_obs)[0]
        assert (got["held"] == want).all()
        assert [bool(got["held"][c]) for c in (0, 8, 16)] == [min_obs > 1, min_obs > 2, min_obs > 3]
        d = got["delta"].reshape(P, 3)
        assert not d[want].any() and d[~want].all(1).all()
