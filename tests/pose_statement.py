"""An independent statement of the pose stage (k_pose_offsets, k_pose, pose_solve), in numpy / scipy only.

Nothing here comes from oracle/, cylindertag_amd/csrc or testkit: the detection and pose records are read through the field
names of their dtypes, a model is {"ids", "size", "corners"}, a camera is (K 3x3, dist[n_dist]).  What is restated, from
PoseEstimator::PnPSolver / PoseBA (pose_estimation.cpp:50-143) and the published OpenCV / Ceres definitions:

  model lookup       the first model with the marker's id
  correspondences    the end-feature skip, corners 0 1 4 5 [2 3 6 7], and the status rules of include/ctag_pose.h
  project12          cv::projectPoints with k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
  undistort12        cv::undistortPoints: 5 fixed-point iterations, the icdist < 0 escape, coefficients beyond n_dist zero
  observation        float32(fx * xn + cx), model points as float32
  cost_at            half the sum of squared reprojection residuals
  minimum_from       scipy.optimize.least_squares (trf, all tolerances 1e-15, x_scale="jac") on that residual

EPnP and the LM loop are NOT restated step by step: check_pose_records states what they must reach."""
import numpy as np
from scipy.optimize import least_squares

OK, NO_MODEL, TOO_FEW, BAD_POS, DEGENERATE = 0, 1, 2, 3, 4
MAX_POINTS = 160     # CTAG_POSE_MAX_POINTS
MAX_FEATURES = 100   # features of one detection record
MAX_MARKERS = 100    # markers of one detection record
CORNER_ORDER = (0, 1, 4, 5, 2, 3, 6, 7)
MIN_POINTS_FOR_MINIMUM = 16  # fewer points can leave a flat or two-fold minimum
POSE_FIELDS = ("rvec", "tvec", "rvec0", "tvec0", "cost0", "cost", "iterations")


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.sqrt(r @ r)
    if th < 1e-12:
        return np.eye(3)
    w = r / th
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * Wx + (1 - np.cos(th)) * np.outer(w, w)


def _k12(dist):
    """The 12 coefficients the pose stage reads: those beyond n_dist (and the two tilt terms) are zero."""
    d = np.asarray(dist, np.float32).ravel().astype(np.float64)
    k = np.zeros(12)
    k[:min(12, d.size)] = d[:12]
    return k


def _intrinsics(K):
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def project12(K, dist, rvec, tvec, X):
    """cv::projectPoints, float64: radial (1 + k1 r2 + k2 r4 + k3 r6) / (1 + k4 r2 + k5 r4 + k6 r6), tangential p1 p2,
    thin prism s1..s4."""
    fx, fy, cx, cy = _intrinsics(K)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _k12(dist)
    P = np.asarray(X, np.float64) @ rodrigues(rvec).T + np.asarray(tvec, np.float64)
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    rad = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
    return np.stack([fx * xd + cx, fy * yd + cy], 1)


def undistort12(K, dist, uv, return_escaped=False):
    """cv::undistortPoints to normalised coordinates (cvUndistortPointsInternal, OpenCV 4.5.3): exactly 5 fixed-point
    iterations x <- (x0 - delta(x)) * icdist(x); a point whose icdist turns negative keeps its start value (x0, y0).
    With return_escaped also the mask of the points that left that way."""
    fx, fy, cx, cy = _intrinsics(K)
    k = _k12(dist)
    uv = np.asarray(uv, np.float32).astype(np.float64).reshape(-1, 2)
    x0 = (uv[:, 0] - cx) / fx
    y0 = (uv[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    escaped = np.zeros(uv.shape[0], bool)
    with np.errstate(all="ignore"):
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            escaped |= icdist < 0                       # these points are back at (x0, y0) and stay there
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = np.where(escaped, x0, (x0 - dx) * icdist)
            y = np.where(escaped, y0, (y0 - dy) * icdist)
    out = np.stack([x, y], 1)
    return (out, escaped) if return_escaped else out


def observations(K, dist, img):
    """What PoseBA fits: undistortPoints(..., P = K) written back into vector<Point2f>."""
    fx, fy, cx, cy = _intrinsics(K)
    with np.errstate(all="ignore"):
        xn = undistort12(K, dist, img)
        return np.stack([fx * xn[:, 0] + cx, fy * xn[:, 1] + cy], 1).astype(np.float32).astype(np.float64)


def model_lookup(model, marker_id):
    """pose_estimation.cpp:57-63: the first model with the marker's id, -1 if none."""
    hit = np.nonzero(np.asarray(model["ids"]) == marker_id)[0]
    return int(hit[0]) if hit.size else -1


def correspondences(rec, m, model, mi, corner_order=CORNER_ORDER):
    """pose_estimation.cpp:72-95 for marker m of detection record rec against model mi, with the rejections of
    include/ctag_pose.h.  Returns (status, obj float32 [n,3], img float32 [n,2]); n = 0 unless the status is OK."""
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32))
    M = rec["markers"][m]
    first, nf, n_pos = int(M["first_feature"]), int(M["n_features"]), int(M["n_pos"])
    size = int(model["size"])
    if first < 0 or nf < 0 or first + nf > MAX_FEATURES:
        return (BAD_POS,) + none                      # features outside the record
    obj, img = [], []
    for j in range(nf):
        F = rec["features"][first + j]
        il, ir, pos = int(F["id_left"]), int(F["id_right"]), int(F["pos"])
        ad = abs(il - ir)
        if nf > 3 and (j == 0 or j == nf - 1) and (ad > 1 or ir == -1):
            continue                                  # :73-76
        if j >= n_pos or pos < 0 or pos >= size:
            return (BAD_POS,) + none                  # no position, or one outside the model
        ks = corner_order[:8] if (ad < 3 and ir != -1) else corner_order[:4]   # :77-94
        if len(obj) + len(ks) > min(size * 8, MAX_POINTS):
            return (BAD_POS,) + none                  # repeated positions: more points than the model has
        for k in ks:
            img.append(F["corners"][2 * k:2 * k + 2])
            obj.append(model["corners"][mi][pos * 8 + k])
    if not obj:
        return (OK,) + none
    return OK, np.array(obj, np.float32).reshape(-1, 3), np.array(img, np.float32).reshape(-1, 2)


def marker_count(rec):
    """Pose records of one detection record: none for a frame that is not CTAG_OK, else n_markers clamped to [0, 100]."""
    return min(max(int(rec["n_markers"]), 0), MAX_MARKERS) if int(rec["status"]) == 0 else 0


def offsets_of(detection_records):
    """ctag_pose_batch_device's offsets: the exclusive scan of the per-frame record counts, n_frames + 1 entries."""
    counts = np.array([marker_count(r) for r in detection_records], np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def expected_record(rec, m, model):
    """(status, model_index, n_points, obj, img) of marker m; status OK stands for "EPnP + PoseBA run" (OK or DEGENERATE)."""
    mi = model_lookup(model, int(rec["markers"][m]["marker_id"]))
    if mi < 0:
        return NO_MODEL, -1, 0, None, None
    st, obj, img = correspondences(rec, m, model, mi)
    if st != OK:
        return st, mi, 0, None, None
    if len(obj) < 4:
        return TOO_FEW, mi, len(obj), None, None
    return OK, mi, len(obj), obj, img


class Problem:
    """The least-squares problem PoseBA poses for one marker."""

    def __init__(self, K, dist, obj, img):
        self.fx, self.fy, self.cx, self.cy = _intrinsics(K)
        self.X = np.asarray(obj, np.float32).astype(np.float64)
        self.obs = observations(K, dist, img)

    def residual(self, p):
        P = self.X @ rodrigues(p[:3]).T + p[3:]
        return np.concatenate([self.fx * P[:, 0] / P[:, 2] + self.cx - self.obs[:, 0],
                               self.fy * P[:, 1] / P[:, 2] + self.cy - self.obs[:, 1]])

    def cost_at(self, rvec, tvec):
        r = self.residual(np.concatenate([np.asarray(rvec, np.float64), np.asarray(tvec, np.float64)]))
        return 0.5 * float(r @ r)

    def minimum_from(self, rvec0, tvec0):
        """scipy's minimum of the residual from the EPnP pose.  Central differences: with forward differences scipy's own
        minimum is off by a few 1e-6 rad on 16- to 24-point markers, more than the 1e-6 it is used to measure."""
        return least_squares(self.residual, np.concatenate([rvec0, tvec0]), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                             x_scale="jac", jac="3-point")


last_stats = {}  # worst figures of the most recent check_pose_records call, for reports


def check_pose_records(records, detection_records, model, camera, planted=None, degenerate=None, max_minimum_checks=None):
    """Asserts that `records` (pose records in batch order) are the poses of `detection_records` under `model` and
    `camera` = (K, dist):

      1. one record per marker of every CTAG_OK frame, in order; status, model_index, frame, marker, n_points equal the
         statement's.  DEGENERATE is accepted exactly where degenerate(frame, marker, model_index) says so; there, and for
         every other status but OK, the pose fields are zero.
      2. status OK: |cost0 - cost_at(rvec0, tvec0)| and |cost - cost_at(rvec, tvec)| <= 1e-9 * max(1, cost);
         cost <= cost0; 0 <= iterations <= 50.
      3. status OK and n_points >= 16: cost <= min.cost * (1 + 1e-9) + 1e-12, |rvec - min.x[:3]| < 1e-6,
         |tvec - min.x[3:]| < 1e-4 * max|t|, min = minimum_from(rvec0, tvec0).  At most max_minimum_checks records, spread
         evenly over the eligible ones, get this check (None: all).
      4. planted[frame][marker] = (model_index, rvec, tvec) given (noise-free input, no distortion), n_points >= 16:
         |R(rvec0) - R(planted)| < 2e-4 per entry, |tvec0 - planted| < 0.2.

    Returns how many records got check 3."""
    K, dist = camera
    degenerate = degenerate or (lambda frame, marker, model_index: False)
    want_index = [(f, m) for f, r in enumerate(detection_records) for m in range(marker_count(r))]
    assert len(records) == len(want_index), "%d records for %d markers" % (len(records), len(want_index))
    problems = {}
    for w, (f, m) in enumerate(want_index):
        P = records[w]
        what = "record %d (frame %d marker %d)" % (w, f, m)
        st, mi, n, obj, img = expected_record(detection_records[f], m, model)
        assert (int(P["frame"]), int(P["marker"])) == (f, m), what
        assert int(P["model_index"]) == mi, (what, int(P["model_index"]), mi)
        if st == OK and degenerate(f, m, mi):
            st = DEGENERATE
        assert int(P["status"]) == st, (what, "status", int(P["status"]), st)
        assert int(P["n_points"]) == n, (what, "n_points", int(P["n_points"]), n)
        if st != OK:
            for k in POSE_FIELDS:
                assert not np.any(P[k]), (what, k, "set on status %d" % st)
        else:
            problems[w] = Problem(K, dist, obj, img)
    stats = {"records": len(records), "ok": len(problems), "cost_rel": 0.0, "min_cost_excess": 0.0, "drvec": 0.0,
             "dtvec_rel": 0.0, "minimum_checks": 0}
    for w, pb in problems.items():
        P = records[w]
        what = "record %d (frame %d marker %d)" % (w, int(P["frame"]), int(P["marker"]))
        assert 0 <= int(P["iterations"]) <= 50, what
        assert P["cost"] <= P["cost0"], (what, float(P["cost"]), float(P["cost0"]))
        for ck, rk, tk_ in (("cost0", "rvec0", "tvec0"), ("cost", "rvec", "tvec")):
            d = abs(pb.cost_at(P[rk], P[tk_]) - float(P[ck])) / max(1.0, float(P["cost"]))
            stats["cost_rel"] = max(stats["cost_rel"], d)
            assert d <= 1e-9, (what, ck, d)
    eligible = [w for w in problems if int(records[w]["n_points"]) >= MIN_POINTS_FOR_MINIMUM]
    if max_minimum_checks is not None and len(eligible) > max_minimum_checks:
        pick = np.unique(np.linspace(0, len(eligible) - 1, max_minimum_checks).round().astype(int))
        eligible = [eligible[i] for i in pick]
    for w in eligible:
        P, pb = records[w], problems[w]
        what = "record %d (frame %d marker %d, %d points)" % (w, int(P["frame"]), int(P["marker"]), int(P["n_points"]))
        sol = pb.minimum_from(P["rvec0"], P["tvec0"])
        dr = float(np.abs(P["rvec"] - sol.x[:3]).max())
        dt = float(np.abs(P["tvec"] - sol.x[3:]).max() / np.abs(P["tvec"]).max())
        stats["min_cost_excess"] = max(stats["min_cost_excess"], (float(P["cost"]) - sol.cost) / max(sol.cost, 1e-300))
        stats["drvec"], stats["dtvec_rel"] = max(stats["drvec"], dr), max(stats["dtvec_rel"], dt)
        assert P["cost"] <= sol.cost * (1 + 1e-9) + 1e-12, (what, float(P["cost"]), sol.cost)
        assert dr < 1e-6, (what, "rvec", dr)
        assert dt < 1e-4, (what, "tvec", dt)
        stats["minimum_checks"] += 1
    if planted is not None:
        n_planted = 0
        for w in problems:
            P = records[w]
            if int(P["n_points"]) < MIN_POINTS_FOR_MINIMUM:
                continue
            mi, rv, tv = planted[int(P["frame"])][int(P["marker"])]
            assert mi == int(P["model_index"])
            what = "record %d (frame %d marker %d)" % (w, int(P["frame"]), int(P["marker"]))
            assert np.abs(rodrigues(P["rvec0"]) - rodrigues(rv)).max() < 2e-4, (what, "EPnP rotation")
            assert np.abs(P["tvec0"] - tv).max() < 0.2, (what, "EPnP translation")
            n_planted += 1
        stats["planted_checks"] = n_planted
    last_stats.clear()
    last_stats.update(stats)
    return stats["minimum_checks"]
