"""The independent statement of the pose stage (tests/pose_statement.py) held against the CPU pose oracle, without a GPU:
its camera model equals the oracle's exactly, it accepts the oracle's records on every batch tests/test_pose_forms_gpu.py
sends through the kernel (same builders, same shapes), the degenerate and corrupted inputs get the statuses it states, and
it rejects records with planted errors."""
import hashlib

import numpy as np
import pytest

import pose_statement as ps
from pose_testlib import (OFFSET_FRAME_COUNTS, PoseOracle, camera_batch, capacity_batch, check_batch, golden_camera_and_model,
                          grid_stride_batch, guard_batch, make_camera, make_cylinder_model, offsets_batch,
                          oracle_records, random_view, status_batches, synth_pose_results, test_cameras)

CAMERAS = sorted(test_cameras())
N_DIST_CAMERAS = [c for c in CAMERAS if c != "icdist"]

# sha256 of synth_pose_results(golden model, golden camera, n_frames, seed) with default arguments -- records, then truth --
# taken at the commit before the generator gained its optional arguments
GENERATOR_HASHES = {(512, 1): "fe91d21c7a7b9859b300b673a97bb7195bfeb471e55b96eef1823392ad8c5496",
                    (64, 3): "cf8be3b8293973b00cf5bcfbe944e6c1cd9649e0e5132e34086c21f167cd989a",
                    (16, 5): "283bae4b08856b5dbb90aba3730d6b6f2b637f924761c1a3052838d4549adab7",
                    (40, 11): "4a55ed4b075b600e62aa22a5eea4664b3d761c6a9a406ce7bfbaae79f52cfb6a",
                    (60, 13): "025bae1d77208fb74a6408faae1ee9b4a096d37c94c82af6c1dfaa64e819f574"}


@pytest.fixture(scope="module")
def po():
    return PoseOracle()


def test_default_generator_records_are_unchanged():
    K, dist, model = golden_camera_and_model()
    for (n, seed), want in GENERATOR_HASHES.items():
        recs, truth = synth_pose_results(model, K, dist, n, seed)
        h = hashlib.sha256(recs.tobytes())
        h.update(repr([[(mi, rv.tobytes(), tv.tobytes()) for mi, rv, tv in t] for t in truth]).encode())
        assert h.hexdigest() == want, (n, seed)


def _frame_points(rng):
    """Pixels of a 1920x1200 frame: its corners and border, a grid, and the corners of twelve random marker views."""
    K, dist, model = golden_camera_and_model()
    gx, gy = np.meshgrid(np.linspace(0, 1919, 25), np.linspace(0, 1199, 17))
    pts = [np.stack([gx.ravel(), gy.ravel()], 1)]
    for v in range(12):
        pts.append(random_view(rng, model["corners"][v % 6], K, dist, 0.2)[2])
    return np.concatenate(pts).astype(np.float32)


@pytest.mark.parametrize("name", CAMERAS)
def test_undistort12_equals_the_oracle_exactly(po, name):
    K = golden_camera_and_model()[0]
    dist = test_cameras()[name]
    uv = _frame_points(np.random.default_rng(17))
    got, escaped = ps.undistort12(K, dist, uv, return_escaped=True)
    want = po.undistort(make_camera(K, dist), uv, False)
    assert np.array_equal(got, want), np.abs(got - want).max()
    if name == "icdist":  # 1 - 60 r^2 < 0 beyond 558 px from the principal point: the frame's corners escape, its middle does not
        assert 100 < escaped.sum() < len(uv) - 100
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        start = np.stack([(uv[:, 0].astype(np.float64) - cx) / fx, (uv[:, 1].astype(np.float64) - cy) / fy], 1)
        assert np.array_equal(got[escaped], start[escaped])
        assert escaped[[0, 24, 16 * 25, 16 * 25 + 24]].all()  # the four corner pixels
    else:
        assert not escaped.any()
    # the BA observation: through K, rounded to float32
    assert np.array_equal(ps.observations(K, dist, uv), po.undistort(make_camera(K, dist), uv, True).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name", N_DIST_CAMERAS)
def test_project12_inverts_undistort12_inside_the_frame(name):
    K = golden_camera_and_model()[0]
    dist = test_cameras()[name]
    uv = _frame_points(np.random.default_rng(18))
    uv = uv[(uv[:, 0] >= 0) & (uv[:, 0] <= 1919) & (uv[:, 1] >= 0) & (uv[:, 1] <= 1199)]
    xn = ps.undistort12(K, dist, uv)
    back = ps.project12(K, dist, np.zeros(3), np.zeros(3), np.concatenate([xn, np.ones((len(xn), 1))], 1))
    assert np.abs(back - uv).max() < 2e-3  # pixels: float32 input and five iterations


def test_models_and_cameras():
    for size in (12, 13, 16, 19, 20):
        m = make_cylinder_model(3, size)
        assert m["corners"].shape == (3, size * 8, 3) and m["corners"].dtype == np.float32
        assert len(np.unique(m["corners"].reshape(-1, 3), axis=0)) == 3 * size * 8
        assert np.linalg.matrix_rank(m["corners"][0].astype(np.float64) - m["corners"][0].mean(0)) == 3
    cams = test_cameras()
    assert sorted(len(d) for d in cams.values()) == [0, 4, 5, 5, 8, 12, 14]
    assert list(cams["n_dist14"][5:]) == [np.float32(v) for v in (0.8, -3, 5, 2e-3, -4e-3, 1e-3, 3e-3, 0, 0)]
    assert list(cams["icdist"]) == [-60, 0, 0, 0, 0]


def _report(what, batch, n):
    print("\n%s: %d work items, %d held against scipy; worst cost mismatch %.1e (relative), cost above the minimum %.1e, "
          "|d rvec| %.1e, |d tvec|/|t| %.1e" % (what, int(ps.offsets_of(batch["recs"])[-1]), n, ps.last_stats["cost_rel"],
                                                ps.last_stats["min_cost_excess"], ps.last_stats["drvec"], ps.last_stats["dtvec_rel"]))


@pytest.mark.parametrize("form", ["small", "large"])
@pytest.mark.parametrize("name", CAMERAS)
def test_statement_accepts_the_oracle_camera_models(po, name, form):
    batch = camera_batch(name, form)
    n = check_batch(oracle_records(po, batch), batch)
    _report("camera %s, %s form" % (name, form), batch, n)
    assert n == 150


@pytest.mark.parametrize("size", [12, 13, 19, 20])
def test_statement_accepts_the_oracle_capacity_edges(po, size):
    batch = capacity_batch(size)
    P = oracle_records(po, batch)
    n = check_batch(P, batch)
    _report("capacity edges, %d columns" % size, batch, n)
    ok = P[P["status"] == 0]
    assert set(int(v) for v in ok["n_points"]) == set(c for c in batch["counts"] if c <= size * 8)
    if size > 12:  # the marker with a repeated position
        bad = P[P["status"] == ps.BAD_POS]
        assert len(bad) == 6 and not bad["n_points"].any()
    assert n == (ok["n_points"] >= 16).sum() == ps.last_stats["planted_checks"]


@pytest.mark.parametrize("form", ["small", "large"])
def test_statement_accepts_the_oracle_grid_stride_batch(po, form):
    batch = grid_stride_batch(form)
    P = oracle_records(po, batch)
    n = check_batch(P, batch)
    _report("grid stride, %s form" % form, batch, n)
    assert n == 150 and len(P) >= 2 * 4096 + 33
    want = np.array([0, 0, ps.NO_MODEL, ps.BAD_POS, ps.TOO_FEW, ps.DEGENERATE])[np.arange(len(P)) % 6]
    assert np.array_equal(P["status"], want)
    assert np.array_equal(P["n_points"], np.array([56, 4, 0, 0, 0, 24])[np.arange(len(P)) % 6])


def test_statement_and_oracle_statuses(po):
    """Planar and collinear models, NaN and Inf corners: DEGENERATE with n_points kept and the pose fields zero; a marker
    without features: TOO_FEW."""
    batches = status_batches()
    for name in ("planar", "collinear"):
        P = oracle_records(po, batches[name])
        check_batch(P, batches[name])
        posed = (P["model_index"] >= 0) & (P["n_points"] >= 4)
        assert posed.sum() >= 20 and (P["status"][posed] == ps.DEGENERATE).all() and not (P["status"] == 0).any()
    b = batches["non-finite corners"]
    P = oracle_records(po, b)
    check_batch(P, b)
    off = ps.offsets_of(b["recs"])
    for f in (3, 4):
        assert [int(s) for s in P["status"][off[f]:off[f + 1]]] == [0, ps.DEGENERATE, 0]
        assert P[off[f] + 1]["n_points"] == 40 and not P[off[f] + 1]["tvec0"].any()
    assert [int(s) for s in P["status"][off[5]:off[6]]] == [0, ps.TOO_FEW, 0] and P[off[5] + 1]["n_points"] == 0


def test_statement_and_oracle_guards(po):
    b = guard_batch()
    P = oracle_records(po, b)
    check_batch(P, b)
    off = ps.offsets_of(b["recs"])
    assert list(np.diff(off)) == [3] * 7 + [0, 100] + [3] * 7
    assert P[off[5] + 1]["status"] == ps.BAD_POS and P[off[6] + 1]["status"] == ps.BAD_POS
    assert [int(s) for s in P["status"][[off[5], off[5] + 2, off[6], off[6] + 2]]] == [0, 0, 0, 0]
    assert (P["status"][off[8] + 3:off[9]] == ps.TOO_FEW).all()  # markers 3 .. 99 of the record: zeros


@pytest.mark.parametrize("n_frames", OFFSET_FRAME_COUNTS)
def test_statement_accepts_the_oracle_offsets_batches(po, n_frames):
    b = offsets_batch(n_frames)
    P = oracle_records(po, b)
    check_batch(P, b)
    counts = np.where(b["recs"]["status"] == 0, b["recs"]["n_markers"], 0)
    assert np.array_equal(ps.offsets_of(b["recs"]), np.concatenate([[0], np.cumsum(counts)]))
    if n_frames > 8:
        assert (b["recs"]["status"] != 0).any() and len(P) > n_frames // 2


def test_check_pose_records_rejects_planted_errors(po):
    """The check must be able to fail: one rvec component moved by 1e-5, n_points off by 4, and a record computed from the
    corner order 0 1 2 3 4 5 6 7 are each rejected."""
    batch = camera_batch("n_dist5", "small")
    batch["recs"] = batch["recs"][:12]
    batch.pop("min_cap")
    good = oracle_records(po, batch)
    assert check_batch(good, batch) >= 20
    cand = [w for w in range(len(good)) if good[w]["status"] == 0 and good[w]["n_points"] >= 16]
    w = cand[0]
    bad = good.copy()
    bad[w]["rvec"][1] += 1e-5
    with pytest.raises(AssertionError):
        check_batch(bad, batch)
    bad = good.copy()
    bad[w]["n_points"] += 4
    with pytest.raises(AssertionError):
        check_batch(bad, batch)
    # a marker with a 4-point feature: the order 0 1 2 3 .. takes corners 2 3 where the reference takes 4 5
    cam = make_camera(batch["K"], batch["dist"])
    planted = 0
    for w in cand:
        f, m = int(good[w]["frame"]), int(good[w]["marker"])
        if good[w]["n_points"] % 8 == 0:
            continue
        st, obj, img = ps.correspondences(batch["recs"][f], m, batch["model"], int(good[w]["model_index"]), corner_order=tuple(range(8)))
        assert st == 0 and len(obj) == good[w]["n_points"]
        st, r0, t0 = po.epnp(cam, obj, img)
        assert st == 0
        it, r, t, c0, c1 = po.ba(cam, obj, img, r0, t0)
        bad = good.copy()
        for k, v in (("rvec0", r0), ("tvec0", t0), ("rvec", r), ("tvec", t), ("iterations", it), ("cost0", c0), ("cost", c1)):
            bad[w][k] = v
        with pytest.raises(AssertionError):
            check_batch(bad, batch)
        planted += 1
    assert planted >= 3
