"""GPU tests of the intrinsics fit's kernels through the testkit probes: k_ifit_record + k_ifit_assemble + k_ifit_solve and k_ifit_pose
at a state the independent statement (tests/intr_fit_statement.py) names, on every case of tests/intr_fit_shapes.py."""
import numpy as np
import pytest

import intr_fit_shapes as sh
import intr_fit_statement as it
import testkit as tk
from intr_fit_testlib import Detectors, camera_c, device_rig_poses, input_of, poses_of, records_at

pytestmark = pytest.mark.gpu
LAMBDAS = (1e-3, 1.0)
COST_DELTA_PX = 64 * 2.0 ** -52 * 2048   # what 64 roundings at the size of a pixel coordinate (below 2048) can move one residual entry by


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "state": {}}
    yield e
    e["dets"].close()


def _state(env, name):
    """(case, detector, Model, Rigs, planted CameraC, views, statement state (p, poses), the probe's records at it), once per case."""
    if name not in env["state"]:
        c, V = sh.case(name), sh.views(name)
        det = env["dets"].of(c)
        M, rigs, _ = input_of(c)
        p, poses = sh.probed_state(name)
        cam = camera_c(p, c)
        template = device_rig_poses(det, c["recs"], M, rigs, cam)
        env["state"][name] = (c, det, M, rigs, cam, V, p, poses, template, records_at(template, V, poses))
    return env["state"][name]


def _masks(c):
    """The case's own mask and tie, and for the default-mask cases the intrinsics alone and the coefficients alone."""
    out = [(c["mask"], c["tie"])]
    if c["shape"] in ("b", "c12", "d"):
        full = it.default_mask(c["n_dist"])
        out += [(0xF, False), (0xF, True), (full & ~0xF, False)] + ([(full, False)] if full != c["mask"] else [])
    return out


@pytest.mark.parametrize("name", sh.NAMES)
def test_system_against_the_statement(env, name):
    """S, g and delta of the probe at the planted camera with every view pose at the statement's minimum, over the free rows."""
    c, det, M, rigs, cam, V, p, poses, _, recs = _state(env, name)
    cost = it.total_cost(it.record_costs(V, p, poses)[0])
    for mask, tied in _masks(c):
        tie = float(p[1] / p[0]) if tied else None
        rows = it.free_rows(mask, tie)
        S, g = it.reduced_system(V, p, poses, tie)
        for lam in LAMBDAS:
            d, pd = it.step(S, g, mask, lam, tie)
            got = det.intrinsics_fit_system(c["recs"], recs, M, rigs, cam, lam, free_mask=mask, tie_focal=int(tied))
            assert pd and not got["bad_pivot"] and got["n_free"] == len(rows)
            eS, eg, ed = it.system_deviation(got["S"], got["g"], got["delta"], S, g, d, cost, rows)
            print("%s mask %#x tie %d lambda %g: S %.2e g %.2e delta %.2e (bars %.2e %.2e %.2e)" % (name, mask, tied, lam, eS, eg, ed, it.SYSTEM_BAR["S"],
                                                                                                  it.SYSTEM_BAR["g"], it.SYSTEM_BAR["delta"]))
            assert eS <= it.SYSTEM_BAR["S"] and eg <= it.SYSTEM_BAR["g"] and ed <= it.SYSTEM_BAR["delta"]
            fixed = [i for i in range(it.N) if i not in rows]
            assert not got["delta"][fixed].any()


@pytest.mark.parametrize("name", [n for n in sh.NAMES if n[0] in "ce"])
def test_pass_size_does_not_change_a_byte(env, name):
    c, det, M, rigs, cam, V, p, poses, _, recs = _state(env, name)
    own = det.intrinsics_fit_system(c["recs"], recs, M, rigs, cam, 1e-3, free_mask=c["mask"], tie_focal=int(c["tie"]))
    for pass_records in (1, 7):
        got = det.intrinsics_fit_system(c["recs"], recs, M, rigs, cam, 1e-3, free_mask=c["mask"], tie_focal=int(c["tie"]), pass_records=pass_records)
        for k in ("S", "g", "delta"):
            assert got[k].tobytes() == own[k].tobytes(), (k, pass_records)


@pytest.mark.parametrize("name", ["a 0.1 px", "c12 noise-free"])
def test_pivot_flag(env, name):
    """A negative lambda makes (S + lambda diag S) indefinite: the flag is raised and delta stays zero."""
    c, det, M, rigs, cam, V, p, poses, _, recs = _state(env, name)
    got = det.intrinsics_fit_system(c["recs"], recs, M, rigs, cam, -2.0, free_mask=c["mask"])
    assert got["bad_pivot"] and not got["delta"].any()


@pytest.mark.parametrize("name", sh.NAMES)
def test_view_poses_against_the_statement(env, name):
    """k_ifit_pose from the pose call's own poses under the planted camera against the statement's minimiser from the planted poses."""
    c, det, M, rigs, cam, V, p, poses, template, _ = _state(env, name)
    start = records_at(template, V, poses_of(template, V))
    got, usable = det.intrinsics_fit_poses(c["recs"], start, M, rigs, cam)
    assert usable
    a, b = poses_of(got, V), poses
    dev = float(max(np.abs(a[:, :3] - b[:, :3]).max(), (np.abs(a[:, 3:] - b[:, 3:]).max(1) / np.abs(b[:, 3:]).max(1)).max()))
    costs = it.record_costs(V, p, a)[0]
    # cost = 0.5 |r|^2 with every residual entry off by at most COST_DELTA_PX: |d cost| <= |r| sqrt(2 n) delta = sqrt(2 cost) sqrt(2 n) delta
    worst = max(abs(float(got[i]["cost"]) - costs[k]) / (np.sqrt(2 * costs[k]) * np.sqrt(2 * V.n_points[k]) * COST_DELTA_PX) for k, i in enumerate(V.items))
    print("%s: view poses %.2e from the statement's (bar %.2e), cost fields %.2e of their bound from the statement's cost at them" % (name, dev, it.SYSTEM_BAR["pose"], worst))
    assert dev <= it.SYSTEM_BAR["pose"]
    assert worst <= 1.0
    untouched = [i for i in range(len(got)) if i not in V.items]
    assert got[untouched].tobytes() == start[untouched].tobytes()
    again, _ = det.intrinsics_fit_poses(c["recs"], start, M, rigs, cam)
    assert again.tobytes() == got.tobytes()


def test_limits():
    assert tk.intrinsics_fit_limits() == {"record_grid": sh.RECORD_GRID, "pass_records": sh.PASS_RECORDS}
