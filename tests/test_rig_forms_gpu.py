"""The rig pose kernels (k_rig_count, k_rig_solve<160,64>, k_rig_solve<800,256>) through ctag_rig_pose_batch_device, on the paths
the parity tests of test_rig_pose_gpu.py never drive: every point count next to the 256-thread solve's loop edges and to the
switch between the two work lists, more items than twice either solve grid and than k_rig_count's grid, member_mask words 1-3,
the clamp of n_markers, the bound that skips a member and fits the next, duplicates of rejected markers, markers that point
outside the record, and the rejections of the batch call.

Every call is checked twice: with tests/rig_statement.py (numpy / scipy only; tests/test_rig_statement_cpu.py holds it against
the oracle on the same batches of tests/rig_shapes.py) and byte for byte against the oracle's composition, which runs first."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import cylindertag_amd as ca
import rig_shapes as shapes
import rig_statement as rs
import testkit as tk
from cylindertag_amd import capi
from ctag_testlib import GOLDEN
from pose_testlib import PoseOracle, test_cameras
from rig_testlib import compose_batch

pytestmark = pytest.mark.gpu

GUARD = 4  # records before and after the output that must stay untouched
SZ = ca.RIG_POSE_DT.itemsize
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def env():
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    yield {"det": det, "po": PoseOracle(), "marker": (state, fs)}
    det.close()


def device_model(m):
    return ca.Model(ids=m["ids"], corners=m["corners"], model_size=m["size"], base=m["base"], axis=m["axis"])


def device_records(det, b, recs=None):
    """ctag_rig_pose_batch_device on a device copy of the records; returns the n_frames * n_rigs records after checking that the
    guard records before and after them are untouched."""
    import torch
    recs = np.ascontiguousarray(b["recs"] if recs is None else recs)
    n = len(recs)
    M = device_model(b["model"])
    rigs = ca.Rigs(M, b["rig_of_model"], n_rigs=b["n_rigs"])
    d = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).cuda()
    n_out = n * b["n_rigs"]
    out = torch.full(((n_out + 2 * GUARD) * SZ,), 0xA5, dtype=torch.uint8, device="cuda")
    det.rig_pose_batch_device(d.data_ptr(), n, M, rigs, ca.make_camera(b["K"], b["dist"]), out.data_ptr() + GUARD * SZ)
    det.sync()
    raw = out.cpu().numpy()
    assert (raw[:GUARD * SZ] == 0xA5).all() and (raw[(GUARD + n_out) * SZ:] == 0xA5).all(), "bytes written outside n_frames * n_rigs records"
    return raw[GUARD * SZ:(GUARD + n_out) * SZ].copy().view(ca.RIG_POSE_DT)


def differing(got, want):
    """Indices of the records whose bytes differ."""
    assert len(got) == len(want)
    return np.nonzero((got.view(np.uint8).reshape(-1, SZ) != want.view(np.uint8).reshape(-1, SZ)).any(axis=1))[0]


def run(env, b, what, planted=None):
    """Oracle on the CPU, then the device; the statement and the oracle's bytes.  Returns (records, records held against scipy)."""
    t0 = time.perf_counter()
    want = compose_batch(env["po"], b)
    got = device_records(env["det"], b)
    n = rs.check_rig_records(got, b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], (b["K"], b["dist"]), planted=planted)
    bad = differing(got, want)
    assert not len(bad), "%s: %d records differ from the oracle, first %d\n%s\n%s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    print("\n%s; %.1f s" % (rs.report(what), time.perf_counter() - t0))
    return got, n


def run_tiled(env, b, what):
    """A batch tiled from b["distinct"] by b["order"]: the oracle and the statement on the distinct frames, then every record of
    the call against both.  Returns (records, the statement's headers of the call, records held against scipy)."""
    t0 = time.perf_counter()
    n_rigs, order, D = b["n_rigs"], b["order"], len(b["distinct"])
    frames = np.repeat(np.arange(len(order)), n_rigs)
    want = compose_batch(env["po"], b, b["distinct"]).reshape(D, n_rigs)[order].reshape(-1)
    want["frame"] = frames
    got = device_records(env["det"], b)
    assert np.array_equal(got["frame"], frames)
    first = [int(np.argmax(order == d)) for d in range(D)]  # the first copy of every distinct frame, renumbered
    assert all(order[f] == d for d, f in enumerate(first))
    picked = np.concatenate([got[f * n_rigs:(f + 1) * n_rigs] for f in first])
    picked["frame"] = np.repeat(np.arange(D), n_rigs)
    n = rs.check_rig_records(picked, b["distinct"], b["model"], b["rig_of_model"], n_rigs, (b["K"], b["dist"]), degenerate=b.get("degenerate"))
    H = shapes._headers(b, b["distinct"]).reshape(D, n_rigs)
    for d in range(D):
        for g in range(n_rigs):
            if H[d][g]["status"] == rs.OK and b.get("degenerate", lambda f, g: False)(d, g):
                H[d][g]["status"] = rs.DEGENERATE
    H = H[order].reshape(-1)
    H["frame"] = frames
    for k in rs.HEADER_FIELDS:
        assert np.array_equal(got[k], H[k]), (what, k, np.nonzero((got[k] != H[k]).reshape(len(got), -1).any(axis=1))[0][:8])
    bad = differing(got, want)
    assert not len(bad), "%s: %d records differ from the oracle, first %d\n%s\n%s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    print("\n%s; %d items in the call, %.1f s" % (rs.report(what), len(got), time.perf_counter() - t0))
    return got, H, n


@pytest.mark.parametrize("camera", ["golden", "n_dist8", "n_dist12"])
@pytest.mark.parametrize("model_size", [20, 12])
@pytest.mark.parametrize("form", ["small", "large"])
def test_size_edges(env, form, model_size, camera):
    """4 .. 160 points through k_rig_solve<160,64> and 164 .. 800 through k_rig_solve<800,256>, next to 64, 128, 160, 256, 512,
    768 and 800, where the last trip of a per-point loop is partly filled; from 160-point members and from 96-point members;
    under the golden camera and the 8- and 12-coefficient cameras.  Planted poses on the noise-free frames."""
    b = shapes.size_edges(form, model_size, None if camera == "golden" else test_cameras()[camera])
    got, n = run(env, b, "size edges, %s list, %d-column members, camera %s" % (form, model_size, camera), planted=b["planted"])
    big = [c for c in b["counts"] if c >= 16]
    assert set(int(v) for v in got["n_points"]) == set(b["counts"]) and (got["status"] == 0).all()
    assert n == 4 * len(big) and rs.last_stats["checked_sizes"] == set(big) and rs.last_stats["planted_checks"] == 2 * len(big)
    assert (got["n_members"] >= 2).sum() >= 4 * len(big)


def test_stride_batch(env):
    """9220 items in one call: both solve kernels take more than two items per workgroup, of different lengths and kinds."""
    b = shapes.stride_batch()
    got, H, n = run_tiled(env, b, "stride batch")
    solved = (H["status"] == rs.OK) | (H["status"] == rs.DEGENERATE)
    small, large = int((solved & (H["n_points"] <= 160)).sum()), int((solved & (H["n_points"] > 160)).sum())
    assert (small, large) == (b["small_items"], b["large_items"]) and small > 2 * shapes.SMALL_GRID and large > 2 * shapes.LARGE_GRID
    assert n == 13 and rs.last_stats["checked_sizes"] == {160, 164, 516, 800}
    assert {0, rs.TOO_FEW, rs.DEGENERATE, rs.NOT_SEEN} == set(int(s) for s in got["status"])
    mixed = (H["n_points"].reshape(-1, 2) > 160).sum(axis=1) == 1  # one rig in each list
    assert (mixed & solved.reshape(-1, 2).all(axis=1)).sum() >= 200
    print("stride batch: %d items in the small list, %d in the large list" % (small, large))


def test_count_stride_batch(env):
    """262 208 items: k_rig_count's 262 144 threads take a second item, and what they write there is right on both sides."""
    b = shapes.count_stride_batch()
    got, H, n = run_tiled(env, b, "count stride batch")
    assert len(got) == shapes.COUNT_GRID + 64 and n == 2
    for base in (shapes.COUNT_GRID - 64, shapes.COUNT_GRID):  # the last frame of the first trip, the only frame of the second
        assert [int(got[base + g]["status"]) for g in (0, 5, 63, 1, 17)] == [rs.OK, rs.TOO_FEW, rs.OK, rs.NOT_SEEN, rs.NOT_SEEN]
        assert [int(H[base + g]["status"]) for g in (0, 5, 63, 1, 17)] == [rs.OK, rs.TOO_FEW, rs.OK, rs.NOT_SEEN, rs.NOT_SEEN]
        assert [int(got[base + g]["n_points"]) for g in (0, 5, 63)] == [8, 0, 16] and got[base]["cost0"] > 0
    assert got[-1]["status"] == rs.OK and got[-1]["frame"] == 4096 and got[-1]["rig"] == 63 and got[-1]["cost"] > 0


def test_rule_batch(env):
    """member_mask words 1-3, n_markers 120 and -3, the bound that skips 16 points and fits 8, a duplicate of a rejected marker,
    markers that point outside the record, one id in two models, members without points: in one batch, and each frame alone
    through ctag_estimate_rig_pose with the same bytes apart from `frame`."""
    b = shapes.rule_batch()
    got, n = run(env, b, "rule batch")
    assert n == 14
    assert [int(v) for v in got[2]["member_mask"]] == [0x80000001, 0x80000001, 0x80000001, 0x9] and got[2]["n_members"] == 8
    clamped = got[4:6].copy()
    clamped["frame"] = 1
    assert clamped.tobytes() == got[2:4].tobytes() and (got[6:8]["status"] == rs.NOT_SEEN).all()
    assert got[8]["n_points"] == 800 and got[8]["n_excluded"] == 1 and got[8]["member_mask"][0] == 0b1011111
    M = device_model(b["model"])
    rigs = ca.Rigs(M, b["rig_of_model"])
    cam = ca.make_camera(b["K"], b["dist"])
    for f, name in enumerate(b["names"]):
        one = env["det"].estimate_rig_pose(b["recs"][f], M, rigs, cam)
        one["frame"] = f  # the single-frame call numbers its frame 0
        assert one.tobytes() == got[2 * f:2 * f + 2].tobytes(), name


def test_smaller_call_after_a_larger_one(env):
    """The work lists of a handle are reused, not regrown, by a call with fewer items: same bytes as a fresh handle's."""
    b = shapes.rule_batch()
    det = env["det"]
    large = device_records(det, b)
    small = device_records(det, b, b["recs"][3:6])
    fresh_det = tk.Detector(*env["marker"], device=0)
    try:
        fresh = device_records(fresh_det, b, b["recs"][3:6])
    finally:
        fresh_det.close()
    assert small.tobytes() == fresh.tobytes()
    again = large[6:12].copy()
    again["frame"] -= 3
    assert small.tobytes() == again.tobytes()


def test_rejections_at_the_batch_call(env):
    """Null arguments, n_frames < 0, a tilted camera, a rig set of another model size and more than INT_MAX / 2 items are refused
    with their own status and write nothing; n_frames == 0 succeeds and writes nothing."""
    import torch
    b = shapes.rule_batch()
    det, L = env["det"], capi.load_library()
    M = device_model(b["model"])
    rigs = ca.Rigs(M, b["rig_of_model"])
    cam = ca.make_camera(b["K"], b["dist"])
    recs = np.ascontiguousarray(b["recs"][:2])
    d = torch.from_numpy(recs.view(np.uint8).reshape(2, -1)).cuda()
    out = torch.full((8 * SZ,), 0xA5, dtype=torch.uint8, device="cuda")
    good = [det.h, d.data_ptr(), 2, M.m, rigs.r, C.byref(cam), out.data_ptr()]
    for i, name in ((0, "handle"), (1, "results"), (3, "model"), (4, "rigs"), (6, "out")):
        args = list(good)
        args[i] = None
        assert L.ctag_rig_pose_batch_device(*args) == capi.ERR_ARG, name
    args = list(good)
    args[5] = None
    assert L.ctag_rig_pose_batch_device(*args) == capi.ERR_UNSUPPORTED  # no camera: none the pose back end handles
    golden_model = ca.Model(os.path.join(GOLDEN, "CTag_2f12c.model"))  # 6 models, the rig set was made for 10
    tilted = ca.make_camera(b["K"], np.r_[test_cameras()["n_dist12"], 0.01, 0.0])
    too_many = (INT_MAX // 2) // rigs.n_rigs + 1
    assert too_many * rigs.n_rigs > INT_MAX // 2 >= (too_many - 1) * rigs.n_rigs
    for what, status, call in (("n_frames -1", capi.ERR_ARG, (d.data_ptr(), -1, M, rigs, cam)),
                               ("tilted camera", capi.ERR_UNSUPPORTED, (d.data_ptr(), 2, M, rigs, tilted)),
                               ("another model size", capi.ERR_ARG, (d.data_ptr(), 2, golden_model, rigs, cam)),
                               ("more than INT_MAX / 2 items", capi.ERR_LIMIT, (d.data_ptr(), too_many, M, rigs, cam))):
        with pytest.raises(ca.CtagError) as e:
            det.rig_pose_batch_device(*call, out.data_ptr())
        assert e.value.status == status, what
    det.sync()
    assert (out.cpu().numpy() == 0xA5).all()
    det.rig_pose_batch_device(d.data_ptr(), 0, M, rigs, cam, out.data_ptr())  # no frames: nothing written
    det.sync()
    assert (out.cpu().numpy() == 0xA5).all()
    det.rig_pose_batch_device(d.data_ptr(), 2, M, rigs, cam, out.data_ptr())  # and the same arguments with two frames do write
    det.sync()
    assert (out.cpu().numpy()[:4 * SZ] != 0xA5).any() and (out.cpu().numpy()[4 * SZ:] == 0xA5).all()
