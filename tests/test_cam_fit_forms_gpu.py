"""GPU tests of the camera set fit's kernels through the probe ctag_testkit_camera_fit_system (k_cfit_record, k_fit_assemble<48>,
k_fit_solve<48> at a given state): S, g and delta of every case of tests/cam_fit_shapes.py against the independent statement at the
rule-2 start, with the anchor in its own slot and (case c) in the last one, the pass-size independence of rule 5, a pivot that is not
positive, and the limits."""
import numpy as np
import pytest

import cam_fit_shapes as sh
import cam_fit_statement as cf
import cylindertag_amd as ca
import pose_statement as ps
import testkit as tk
from cam_fit_testlib import Detectors, device_mv_poses, input_of, set_of

pytestmark = pytest.mark.gpu
LAMBDA = 1e-3


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "state": {}}
    yield e
    e["dets"].close()


def _state(env, name, order="forward"):
    """The case at the statement's rule-2 start, its placed cameras in ascending or descending order: (case, detector, Model, Rigs,
    placed, anchor slot, CameraSet, records of the placed cameras, device multi-view records, the statement's observations on them, the
    state (R, t) as the set holds it)."""
    key = (name, order)
    if key not in env["state"]:
        b, A = sh.case(name), sh.assembled(name)
        det = env["dets"].of(b)
        M, _, _ = input_of(b)
        rigs = ca.Rigs(M, b["rig_of_model"], b["n_rigs"])
        placed, R0, t0 = A["init"]["placed"], A["R0"], A["t0"]
        if order == "reversed":
            placed, R0, t0 = placed[::-1], R0[::-1], t0[::-1]
        slot = placed.index(A["init"]["anchor"])
        cs = set_of(b, placed, R0, t0)
        recs = np.ascontiguousarray(b["recs"][placed])
        mvp = device_mv_poses(det, recs, M, rigs, cs)
        O = cf.Observations(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], placed, ok_of=lambda w: mvp[w]["status"] == 0)
        assert O.items == [w for w in range(len(mvp)) if mvp[w]["status"] == 0 and mvp[w]["n_cameras"] >= 2], "the statement's observation set is not the device's"
        poses = cs.poses()
        R = np.array([ps.rodrigues(rv) for rv, _ in poses])
        t = np.array([tv for _, tv in poses])
        env["state"][key] = (b, det, M, rigs, placed, slot, cs, recs, mvp, O, R, t)
    return env["state"][key]


def test_limits_are_the_shapes_files():
    lim = tk.camera_fit_limits()
    assert lim["record_grid"] == sh.RECORD_GRID and lim["pass_records"] == sh.PASS_RECORDS


@pytest.mark.parametrize("name,order", [(n, "forward") for n in sh.NAMES] + [(n, "reversed") for n in sh.NAMES if n.startswith("c")])
def test_system_against_the_statement(env, name, order):
    """S, g and delta; deviations scaled as cf.system_deviation scales them, within 16 x the float64 statement's own error against long
    double (cf.SYSTEM_BAR)."""
    b, det, M, rigs, placed, slot, cs, recs, mvp, O, R, t = _state(env, name, order)
    got = det.camera_fit_system(recs, mvp, M, rigs, cs, slot, LAMBDA)
    N = 6 * len(placed)
    assert got["S"].shape == (N, N) and not got["bad_pivot"]
    state = np.array([np.concatenate([mvp[w]["rvec"], mvp[w]["tvec"]]) for w in O.items])
    S, g = cf.reduced_system(O, R, t, state)
    d, pd = cf.step(S, g, slot, LAMBDA)
    assert pd
    cost = float(sum(mvp[w]["cost"] for w in O.items))
    dev = cf.system_deviation(got["S"], got["g"], got["delta"], S, g, d, cost)
    print("%s %s: S %.2e g %.2e delta %.2e (bars %.2e %.2e %.2e)" % ((name, order) + tuple(dev) + tuple(cf.SYSTEM_BAR[k] for k in ("S", "g", "delta"))))
    assert (got["S"] == got["S"].T).all()
    moved = np.arange(len(placed)) != slot
    assert not got["delta"].reshape(-1, 6)[slot].any(), "the anchor moves"
    assert got["delta"].reshape(-1, 6)[moved].all(1).all()
    for k, v in zip(("S", "g", "delta"), dev):
        assert v <= cf.SYSTEM_BAR[k], (k, v)


@pytest.mark.parametrize("name", ["a 0.1 px", "c 0.1 px", "e noise-free", "e 0.1 px"])
def test_the_pass_size_changes_no_bit(env, name):
    """Rule 5: the workspace processed 1 or 7 records a pass, or its own size (case (e) takes two passes of its own accord); and a second call."""
    b, det, M, rigs, placed, slot, cs, recs, mvp, O, R, t = _state(env, name)
    ref = det.camera_fit_system(recs, mvp, M, rigs, cs, slot, LAMBDA)
    again = det.camera_fit_system(recs, mvp, M, rigs, cs, slot, LAMBDA, pass_records=0)
    for pass_records in (1, 7):
        got = det.camera_fit_system(recs, mvp, M, rigs, cs, slot, LAMBDA, pass_records=pass_records)
        for k in ("S", "g", "delta"):
            assert got[k].tobytes() == ref[k].tobytes() == again[k].tobytes(), (k, pass_records)
    assert np.abs(ref["S"]).max() > 0


def test_a_pivot_that_is_not_positive_is_reported(env):
    b, det, M, rigs, placed, slot, cs, recs, mvp, O, R, t = _state(env, "a noise-free")
    got = det.camera_fit_system(recs, mvp, M, rigs, cs, slot, -2.0)   # S - 2 diag S is indefinite
    assert got["bad_pivot"] and not got["delta"].any()
    assert not det.camera_fit_system(recs, mvp, M, rigs, cs, slot, 0.5)["bad_pivot"]
