"""CPU tests of tests/rig_statement.py, the independent statement of the rig pose: on every batch of tests/rig_shapes.py it must
accept the records the pose oracle's composition (rig_testlib.compose_rig_poses) gives -- which decides, before any device run,
whether the bars of pose_statement.check_pose_records hold at 161-800 points -- it must refuse planted errors, and noise-free
frames must return their planted poses.  tests/test_rig_forms_gpu.py asks the same of the kernels on the same batches."""
import numpy as np
import pytest

import mv_statement as ms
import rig_shapes as shapes
import rig_statement as rs
from pose_statement import Problem
from pose_testlib import PoseOracle, test_cameras
from rig_testlib import RIG_POSE_DT, compose_batch

CAMERAS = ("golden", "n_dist8", "n_dist12")


@pytest.fixture(scope="module")
def po():
    return PoseOracle()


def check(po, b, what, recs=None, degenerate=None, cap=None, planted=None):
    recs = b["recs"] if recs is None else recs
    want = compose_batch(po, b, recs)
    n = rs.check_rig_records(want, recs, b["model"], b["rig_of_model"], b["n_rigs"], (b["K"], b["dist"]), degenerate=degenerate, planted=planted,
                             max_minimum_checks=cap)
    print("\n" + rs.report(what))
    return want, n


def same_membership(b, recs):
    """rig_statement.membership against the one-camera case of mv_statement.membership."""
    for f in range(len(recs)):
        for g in range(b["n_rigs"]):
            members, excluded, obj, img = rs.membership(recs[f], b["model"], b["rig_of_model"], g)
            per_camera, mv_excluded = ms.membership([recs[f]], b["model"], b["rig_of_model"], g)
            assert (members, excluded) == (per_camera[0][0], mv_excluded), (f, g)
            assert np.array_equal(obj, per_camera[0][1]) and np.array_equal(img, per_camera[0][2]), (f, g)


def test_record_layout_is_the_projects():
    assert rs.RIG_POSE_DT == RIG_POSE_DT


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("model_size", [20, 12])
@pytest.mark.parametrize("form", ["small", "large"])
def test_size_edges(po, form, model_size, camera):
    """Every point count of both work lists, from 160- and from 96-point members, under three cameras: the oracle's records pass
    every check, each count of 16 points or more is held against scipy, and the noise-free frames return their planted poses."""
    b = shapes.size_edges(form, model_size, None if camera == "golden" else test_cameras()[camera])
    same_membership(b, b["recs"])
    want, n = check(po, b, "size edges, %s list, %d-column members, camera %s" % (form, model_size, camera), planted=b["planted"])
    big = [c for c in b["counts"] if c >= 16]
    assert n == 4 * len(big) and rs.last_stats["checked_sizes"] == set(big) and rs.last_stats["planted_checks"] == 2 * len(big)
    assert (want["iterations"] > 0).sum() >= 2 * len(big)


def test_stride_batch(po):
    """The 18 distinct frames of the stride batch (the tiled call holds nothing else)."""
    b = shapes.stride_batch()
    same_membership(b, b["distinct"])
    want, n = check(po, b, "stride batch, distinct frames", recs=b["distinct"], degenerate=b["degenerate"])
    assert n == ((want["status"] == 0) & (want["n_points"] >= 16)).sum() == 13
    assert (want["status"] == rs.DEGENERATE).sum() == 2 and set(int(v) for v in want["n_points"]) == {0, 8, 24, 160, 164, 168, 516, 800}
    assert len(b["recs"]) * 2 > 2 * shapes.SMALL_GRID + 2 * shapes.LARGE_GRID


def test_count_stride_batch(po):
    b = shapes.count_stride_batch()
    same_membership(b, b["distinct"])
    want, n = check(po, b, "count stride batch, distinct frames", recs=b["distinct"])
    assert n == 2 and (want["status"] == 0).sum() == 3 and len(b["recs"]) * b["n_rigs"] == shapes.COUNT_GRID + 64


def test_rule_batch(po):
    b = shapes.rule_batch()
    same_membership(b, b["recs"])
    want, n = check(po, b, "rule batch")
    assert n == (want["status"] == 0).sum() - 2 == 14  # the two 8-point records of rig 1 are too small for the minimum check
    hundred, clamped = want[2:4].copy(), want[4:6].copy()
    clamped["frame"] = 1
    assert hundred.tobytes() == clamped.tobytes()  # n_markers 120 reads the record's 100 markers and no more


def test_cap_keeps_every_size(po):
    """max_minimum_checks thins check 3 but leaves one record of every point count."""
    b = shapes.size_edges("large", 20)
    want = compose_batch(po, b)
    n = rs.check_rig_records(want, b["recs"], b["model"], b["rig_of_model"], 1, (b["K"], b["dist"]), max_minimum_checks=4)
    assert len(b["counts"]) <= n < len(want) and rs.last_stats["checked_sizes"] == set(b["counts"])


def test_checker_rejects_planted_errors(po):
    """Each error on an otherwise good record."""
    b = shapes.rule_batch()
    args = (b["model"], b["rig_of_model"], 2, (b["K"], b["dist"]))
    good = compose_batch(po, b)
    assert rs.check_rig_records(good, b["recs"], *args) == 14

    def refused(bad, recs=b["recs"]):
        with pytest.raises(AssertionError):
            rs.check_rig_records(bad, recs, *args)

    hundred = 2 * 1  # frame 1, rig 0: 8 members at both ends of every mask word
    bad = good.copy()
    bad[hundred]["member_mask"][0] ^= np.uint32(1 << 31)
    bad[hundred]["member_mask"][1] |= np.uint32(1 << 30)
    refused(bad)                                                       # one mask bit moved to the neighbouring word
    bad = good.copy()
    bad[2 * 4]["n_excluded"] += 1
    refused(bad)                                                       # n_excluded off by one
    fewer = b["recs"].copy()
    fewer[1]["markers"][99]["marker_id"] = 1099
    dropped = compose_batch(po, b, fewer)
    assert dropped[hundred]["status"] == 0 and dropped[hundred]["n_members"] == 7
    refused(dropped)                                                   # a member dropped, everything else consistent
    plain = 0
    _, obj, img = rs.expected_header(b["recs"][0], b["model"], b["rig_of_model"], 0, 0)
    pb = Problem(b["K"], b["dist"], obj, img)
    bad = good.copy()
    bad[plain]["cost"] = pb.cost_at(good[plain]["rvec"] + [1e-3, 0, 0], good[plain]["tvec"])
    assert bad[plain]["cost"] > good[plain]["cost"] * (1 + 1e-6)
    bad[plain]["cost0"] = max(bad[plain]["cost0"], bad[plain]["cost"])
    refused(bad)                                                       # the cost of a slightly different pose
    bad = good.copy()
    bad[plain]["rvec"][0] += 1e-5
    bad[plain]["cost"] = pb.cost_at(bad[plain]["rvec"], bad[plain]["tvec"])
    assert bad[plain]["cost"] <= bad[plain]["cost0"]
    refused(bad)                                                       # a pose 1e-5 rad off the minimum with its own true cost
    not_seen = 2 * 5
    assert good[not_seen]["status"] == rs.NOT_SEEN
    for field in ("tvec", "cost0", "iterations"):
        bad = good.copy()
        bad[not_seen][field] = 1
        refused(bad)                                                   # pose fields set on NOT_SEEN
    bad = good.copy()
    bad["rig"][[0, 1]] = bad["rig"][[1, 0]]
    refused(bad)                                                       # rig swapped between two records
    bad = good.copy()
    bad["frame"][[0, 2]] = bad["frame"][[2, 0]]
    refused(bad)                                                       # frame swapped between two records
    moved = b["recs"].copy()
    c = moved[0]["features"][1]["corners"]
    c[2:4] = c[0:2]                                                    # corner 1 of a member's feature takes corner 0's pixel
    wrong = compose_batch(po, b, moved)
    assert wrong[plain]["status"] == 0 and wrong[plain]["n_points"] == good[plain]["n_points"]
    refused(wrong)                                                     # right count, wrong points
