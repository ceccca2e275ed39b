"""The pose kernels (k_pose_offsets, k_pose<96,2>, k_pose<160,1>, pose_solve of ctag_pose_dev.h) through
ctag_pose_batch_device, on the paths the parity tests of test_pose_gpu.py never drive: every camera model and the
icdist < 0 escape, point counts at the capacity of both forms, the grid-stride loop, every status, corrupted records,
k_pose_offsets at frame counts around its 256 threads, and camera_ok's rejections.

Every call is checked twice: with tests/pose_statement.py (numpy / scipy only; tests/test_pose_statement_cpu.py holds it
against the oracle on the same batches) and byte for byte against the CPU pose oracle, which runs first."""
import os
import time

import numpy as np
import pytest

import cylindertag_amd as ca
import pose_statement as ps
import testkit as tk
from ctag_testlib import GOLDEN
from pose_testlib import (GRID_BLOCKS, OFFSET_FRAME_COUNTS, PoseOracle, camera_batch, capacity_batch, check_batch,
                          golden_camera_and_model, grid_stride_batch, guard_batch, offsets_batch, oracle_records, status_batches,
                          test_cameras)

pytestmark = pytest.mark.gpu

CAMERAS = sorted(test_cameras())
GUARD = 4  # records / offsets past the end that must stay untouched


@pytest.fixture(scope="module")
def env():
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    yield {"det": det, "po": PoseOracle()}
    det.close()


def device_model(model):
    return ca.Model(ids=model["ids"], corners=model["corners"], model_size=model["size"])


def device_records(det, batch, camera=None):
    """ctag_pose_batch_device on a device copy of the batch's records with capacity = the batch's total; returns
    (offsets[n_frames + 1], records[total]) after checking that nothing past either was written."""
    import torch
    recs = np.ascontiguousarray(batch["recs"])
    n = len(recs)
    total = int(ps.offsets_of(recs)[-1])
    d = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).cuda()
    off = torch.full((n + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    poses = torch.full(((total + GUARD) * ca.POSE_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    M = device_model(batch["model"])
    det.pose_batch_device(d.data_ptr(), n, M, camera or ca.make_camera(batch["K"], batch["dist"]), off.data_ptr(), poses.data_ptr(), total)
    det.sync()
    offs, raw = off.cpu().numpy(), poses.cpu().numpy()
    assert (offs[n + 1:] == -7).all() and (raw[total * ca.POSE_DT.itemsize:] == 0xA5).all(), "written past the end"
    return offs[:n + 1], raw[:total * ca.POSE_DT.itemsize].view(ca.POSE_DT)


def assert_same_bytes(got, want, what):
    assert len(got) == len(want), what
    for w in range(len(got)):
        assert got[w].tobytes() == want[w].tobytes(), "%s: record %d differs from the oracle\n%s\n%s" % (what, w, got[w], want[w])


def run(env, batch, what):
    """Oracle on the CPU, then the device; offsets, the statement and the oracle's bytes.  Returns (offsets, records)."""
    t0 = time.perf_counter()
    want = oracle_records(env["po"], batch)
    offs, P = device_records(env["det"], batch)
    assert np.array_equal(offs, ps.offsets_of(batch["recs"])), what
    n = check_batch(P, batch)
    assert_same_bytes(P, want, what)
    print("\n%s: %d work items, %d held against scipy; worst cost mismatch %.1e (relative), cost above the minimum %.1e, "
          "|d rvec| %.1e, |d tvec|/|t| %.1e; %.1f s" % (what, len(P), n, ps.last_stats["cost_rel"], ps.last_stats["min_cost_excess"],
                                                        ps.last_stats["drvec"], ps.last_stats["dtvec_rel"], time.perf_counter() - t0))
    return offs, P, n


@pytest.mark.parametrize("form", ["small", "large"])
@pytest.mark.parametrize("name", CAMERAS)
def test_camera_models(env, name, form):
    """n_dist 0 / 4 / 5 / 8 / 12 / 14 (rational and thin-prism terms, PoseCam::k[5..11]) and the icdist < 0 escape through
    undistort_normalised, 64 frames, in k_pose<96,2> (12 columns) and k_pose<160,1> (16 columns)."""
    batch = camera_batch(name, form)
    assert batch["model"]["size"] == (12 if form == "small" else 16)
    if name == "icdist":
        assert batch["escaping_points"] > 1000
    _, P, n = run(env, batch, "camera %s, %s form" % (name, form))
    assert n == 150 and (P["status"] == 0).sum() >= 250


@pytest.mark.parametrize("size", [12, 13, 19, 20])
def test_capacity_edges(env, size):
    """Markers of exactly 4, 8, 92 and 96 points in the small form (96 = its LDS capacity: all twelve columns with ids (3,3));
    100, 104, 152 and 160 points in the large form (160 = its capacity) on 13-, 19- and 20-column models, and there a marker with
    a repeated position that would have size*8 + 4 points: BAD_POS, n_points 0, its neighbours computed.  Planted poses."""
    batch = capacity_batch(size)
    _, P, n = run(env, batch, "capacity edges, %d columns" % size)
    ok = P[P["status"] == 0]
    assert set(int(v) for v in ok["n_points"]) == set(c for c in batch["counts"] if c <= size * 8)
    assert len(ok) == 6 * len([c for c in batch["counts"] if c <= size * 8])
    if size > 12:
        bad = P[P["status"] == ps.BAD_POS]
        assert len(bad) == 6 and not bad["n_points"].any() and len(bad) + len(ok) == len(P)
    assert n == (ok["n_points"] >= 16).sum() == ps.last_stats["planted_checks"]


@pytest.mark.parametrize("form", ["small", "large"])
def test_grid_stride(env, form):
    """More than 2 * 4096 + 33 work items in one call with capacity = total: every block of k_pose takes a second item and some
    a third, and the three items of a block are of different kinds (56 points, 4 points, NO_MODEL, BAD_POS, TOO_FEW, planar
    DEGENERATE), so the LDS union is reused after a solve, after an early return from pose_solve, and after items that never
    reach it.  The first 64 frames come again as the last 64: same pose bytes at other work indices."""
    batch = grid_stride_batch(form)
    recs = batch["recs"]
    offs, P, n = run(env, batch, "grid stride, %s form" % form)
    assert n == 150 and len(P) >= 2 * GRID_BLOCKS + 33
    kinds = np.arange(len(P)) % 6
    assert np.array_equal(P["status"], np.array([0, 0, ps.NO_MODEL, ps.BAD_POS, ps.TOO_FEW, ps.DEGENERATE])[kinds])
    assert np.array_equal(P["n_points"], np.array([56, 4, 0, 0, 0, 24])[kinds])
    w = np.arange(len(P) - 2 * GRID_BLOCKS)  # blocks with three items: three kinds
    assert len(w) >= 33 and (kinds[w] != kinds[w + GRID_BLOCKS]).all() and (kinds[w + GRID_BLOCKS] != kinds[w + 2 * GRID_BLOCKS]).all()
    assert (kinds[w] != kinds[w + 2 * GRID_BLOCKS]).all()
    first, last = P[:offs[64]].copy(), P[offs[len(recs) - 64]:].copy()
    assert recs[:64].tobytes() == recs[-64:].tobytes() and len(first) == len(last) >= 512
    assert np.array_equal(last["frame"], first["frame"] + len(recs) - 64)
    last["frame"] = first["frame"]
    assert first.tobytes() == last.tobytes()


def test_statuses(env):
    """DEGENERATE from both exits of pose_solve -- singular control points (planar and collinear models) and a non-finite EPnP
    result (NaN and Inf image corners) -- with n_points kept and the pose fields zero; TOO_FEW from a marker without features."""
    batches = status_batches()
    for name in ("planar", "collinear"):
        _, P, _ = run(env, batches[name], "%s model" % name)
        posed = (P["model_index"] >= 0) & (P["n_points"] >= 4)
        assert posed.sum() >= 20 and (P["status"][posed] == ps.DEGENERATE).all() and not (P["status"] == 0).any()
        for k in ps.POSE_FIELDS:
            assert not P[k].any(), k
    b = batches["non-finite corners"]
    off, P, _ = run(env, b, "non-finite corners")
    for f in (3, 4):
        assert [int(s) for s in P["status"][off[f]:off[f + 1]]] == [0, ps.DEGENERATE, 0]
        hit = P[off[f] + 1]
        assert hit["n_points"] == 40 and not any(hit[k].any() for k in ps.POSE_FIELDS)
    assert [int(s) for s in P["status"][off[5]:off[6]]] == [0, ps.TOO_FEW, 0] and P[off[5] + 1]["n_points"] == 0


def test_guards(env):
    """Corrupted records in the middle of a batch: first_feature 98 with 5 features and first_feature -1 give BAD_POS with
    their neighbours computed; n_markers -3 counts 0 and n_markers 1000 counts 100 in the offsets."""
    b = guard_batch()
    off, P, _ = run(env, b, "guards")
    assert list(np.diff(off)) == [3] * 7 + [0, 100] + [3] * 7
    assert P[off[5] + 1]["status"] == ps.BAD_POS and P[off[6] + 1]["status"] == ps.BAD_POS
    assert [int(s) for s in P["status"][[off[5], off[5] + 2, off[6], off[6] + 2]]] == [0, 0, 0, 0]
    assert (P["status"][off[8] + 3:off[9]] == ps.TOO_FEW).all()


@pytest.mark.parametrize("n_frames", OFFSET_FRAME_COUNTS)
def test_offsets(env, n_frames):
    """k_pose_offsets below, at and past its 256 threads (1, 2, 255, 256, 257, 513 frames), with frames that are not CTAG_OK
    and empty frames: numpy's exclusive scan."""
    b = offsets_batch(n_frames)
    off, P, _ = run(env, b, "offsets, %d frames" % n_frames)
    counts = np.where(b["recs"]["status"] == 0, b["recs"]["n_markers"], 0)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(counts)]))
    if n_frames > 8:
        assert (b["recs"]["status"] != 0).any() and len(P) > n_frames // 2


def test_camera_rejections(env):
    """camera_ok through the C ABI: n_dist 7, a 14-term camera with a tilt term, and K[0] = 0 return CTAG_ERR_UNSUPPORTED and
    write neither offsets nor records."""
    import torch
    K, dist, _ = golden_camera_and_model()
    b = offsets_batch(2)
    recs = np.ascontiguousarray(b["recs"])
    d = torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1)).cuda()
    M = device_model(b["model"])
    tilt = np.concatenate([test_cameras()["n_dist12"], np.float32([0.01, 0])])
    K0 = K.copy()
    K0[0, 0] = 0
    cameras = (("n_dist 7", ca.make_camera(K, np.zeros(7))), ("tilt", ca.make_camera(K, tilt)), ("K[0] == 0", ca.make_camera(K0, dist)))
    for what, cam in cameras:
        off = torch.full((len(recs) + 1,), -7, dtype=torch.int32, device="cuda")
        poses = torch.full((8 * ca.POSE_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(ca.CtagError) as e:
            env["det"].pose_batch_device(d.data_ptr(), len(recs), M, cam, off.data_ptr(), poses.data_ptr(), 8)
        env["det"].sync()
        assert e.value.status == ca.capi.ERR_UNSUPPORTED, what
        assert (off.cpu().numpy() == -7).all() and (poses.cpu().numpy() == 0xA5).all(), what
    assert ca.make_camera(K, tilt).n_dist == 14 and ca.make_camera(K, tilt).dist[12] == np.float32(0.01)
