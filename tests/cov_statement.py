"""An independent statement of the pose covariance (k_pose_cov.hip; include/ctag_pose.h, pose covariance, rules 1-5), in numpy only.

Nothing here comes from oracle/, cylindertag_amd/csrc or testkit.  The correspondences, the observations and the residuals the
Jacobians are held against come from pose_statement.py, rig_statement.py and mv_statement.py; a detection record is read through
the field names of its dtype, a model is {"ids", "size", "corners"}, a camera (K 3x3, dist[n_dist]), a camera pose (rvec, tvec).

  parts_of_*         rule 2: the points of a source record rebuilt from the detection record(s), or None (CTAG_COV_BAD_RECORD)
  rotation           R(rvec) and its three derivatives in either parametrisation (rule 4); the Rodrigues derivative in the closed
                     form of Gallego & Yezzi (2015): dR/dr_k = (r_k [r]x + [r x (I - R) e_k]x) R / |r|^2
  residual_jacobian  rule 3: residuals and the analytic Jacobian of every point, per part the u rows, then the v rows (the order
                     of pose_statement.Problem.residual and mv_statement.MvProblem.residual)
  covariance         rules 1 and 5 from those
  expected_*         the ctag_pose_cov_rec of one source record of each kind
  check_cov_records  what the records of the device must satisfy

Every step from the observations on runs in the float type `ft`: np.float64, or np.longdouble for the figure the comparison bar
comes from.  The observations themselves are data of the problem (float32 values, rule 3), the same in both.

The comparison bar.  deviation(a, b) of two records is the largest of |d cov_ij| / sqrt(cov_ii cov_jj), the relative differences
of cost, sigma2_hat, sigma2_used and max_residual_px, and |d min_pivot| (pivots of a unit-diagonal matrix).  The worst deviation
of the float64 statement from the longdouble statement over every record of every batch of tests/cov_shapes.py, in both
parametrisations, is MEASURED_F64_DEVIATION (tests/test_cov_statement_cpu.py measures it again and holds it against this
figure); it is worst on 4-point records.  The device sums in another order, which moves rounding by a small multiple: BAR is 16
times that figure."""
import numpy as np

import mv_statement as ms
import pose_statement as ps

COV_OK, COV_NO_POSE, COV_BAD_RECORD, COV_SINGULAR = 0, 1, 2, 3
TANGENT, RVEC = 0, 1
MIN_PIVOT = 1e-12
RIG_MAX_POINTS = 800
POSE_COV_DT = np.dtype([("status", "<i4"), ("n_points", "<i4"), ("dof", "<i4"), ("worst_point", "<i4"), ("n_outliers", "<i4"), ("param", "<i4"),
                        ("cost", "<f8"), ("sigma2_hat", "<f8"), ("sigma2_used", "<f8"), ("max_residual_px", "<f8"), ("min_pivot", "<f8"),
                        ("cov", "<f8", (6, 6))])
assert POSE_COV_DT.itemsize == 352
DOUBLE_FIELDS = ("cost", "sigma2_hat", "sigma2_used", "max_residual_px", "min_pivot", "cov")

MEASURED_F64_DEVIATION = 8e-9  # measured 7.88e-09, on a 4-point record
BAR = 16 * MEASURED_F64_DEVIATION

IDENTITY_POSE = (np.zeros(3), np.zeros(3))


def default_opts(param=TANGENT, sigma_px=0.0, outlier_k=3.0):
    return {"param": param, "sigma_px": sigma_px, "outlier_k": outlier_k}


# ---- rule 2: the points ----------------------------------------------------------------------------------------------------------

def _marker_count(rec):
    return min(max(int(rec["n_markers"]), 0), ps.MAX_MARKERS)


def _pose_ok(P, n):
    return n == int(P["n_points"]) and n >= 4 and bool(np.all(np.isfinite(P["rvec"])) and np.all(np.isfinite(P["tvec"])))


def parts_of_marker(P, recs, model):
    """[(camera 0, obj, img)] of per-marker pose record P, or None."""
    f, m, mi = int(P["frame"]), int(P["marker"]), int(P["model_index"])
    if not 0 <= f < len(recs) or int(recs[f]["status"]) != 0:
        return None
    if not 0 <= m < _marker_count(recs[f]) or not 0 <= mi < len(model["ids"]):
        return None
    st, obj, img = ps.correspondences(recs[f], m, model, mi)
    if st != ps.OK or not _pose_ok(P, len(obj)):
        return None
    return [(0, obj, img)]


def _members(rec, mask, model, total):
    """The members of one detection record by a member mask, in marker order: (obj, img) or None."""
    if int(rec["status"]) != 0:
        return None
    objs, imgs = [], []
    for k in range(128):
        if not (int(mask[k >> 5]) >> (k & 31)) & 1:
            continue
        if k >= _marker_count(rec):
            return None
        mi = ps.model_lookup(model, int(rec["markers"][k]["marker_id"]))
        if mi < 0:
            return None
        st, obj, img = ps.correspondences(rec, k, model, mi)
        total += len(obj)
        if st != ps.OK or total > RIG_MAX_POINTS:
            return None
        objs.append(obj)
        imgs.append(img)
    if not objs:
        return np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    return np.concatenate(objs), np.concatenate(imgs)


def parts_of_rig(P, recs, model):
    f = int(P["frame"])
    if not 0 <= f < len(recs):
        return None
    got = _members(recs[f], P["member_mask"], model, 0)
    if got is None or not _pose_ok(P, len(got[0])):
        return None
    return [(0, got[0], got[1])]


def parts_of_mv(P, recs_per_camera, model):
    """recs_per_camera[c][f]; parts in camera order."""
    f = int(P["frame"])
    if not 0 <= f < len(recs_per_camera[0]):
        return None
    parts, total = [], 0
    for c in range(ms.MAX_CAMERAS):
        mask = P["member_mask"][c]
        if not np.any(mask):
            continue
        if c >= len(recs_per_camera):
            return None
        got = _members(recs_per_camera[c][f], mask, model, total)
        if got is None:
            return None
        total += len(got[0])
        parts.append((c, got[0], got[1]))
    if not _pose_ok(P, total):
        return None
    return parts


# ---- rules 3 and 4: residual and Jacobian ----------------------------------------------------------------------------------------

def skew(v, ft=np.float64):
    z = ft(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], ft)


def rotation(rvec, param, ft=np.float64):
    """R(rvec) and [dR/d unknown_k, k = 0 1 2]: the unknowns are rvec itself (RVEC) or dw of R <- Exp(dw) R (TANGENT)."""
    r = np.asarray(rvec, ft)
    th2 = r @ r
    eye = np.eye(3, dtype=ft)
    if th2 > 0:
        th = np.sqrt(th2)
        w = r / th
        R = np.cos(th) * eye + np.sin(th) * skew(w, ft) + (ft(1) - np.cos(th)) * np.outer(w, w)
    else:
        R = eye.copy()
    if param == TANGENT:
        return R, [skew(eye[k], ft) @ R for k in range(3)]
    if th2 > 0:
        rx = skew(r, ft)
        return R, [(r[k] * rx + skew(np.cross(r, (eye - R) @ eye[k]), ft)) @ R / th2 for k in range(3)]
    return R, [skew(eye[k], ft) for k in range(3)]


class Camera:
    def __init__(self, camera, camera_pose, ft):
        fx, fy, cx, cy = ps._intrinsics(camera[0])
        self.fx, self.fy, self.cx, self.cy = ft(fx), ft(fy), ft(cx), ft(cy)
        self.Rc = rotation(camera_pose[0], TANGENT, ft)[0]
        self.tc = np.asarray(camera_pose[1], ft)


def problem_parts(parts, cameras, camera_poses, ft=np.float64):
    """[(Camera, X [n,3], obs [n,2])] in `ft`; the observations are pose_statement.observations' float32 values."""
    out = []
    for c, obj, img in parts:
        obs = ps.observations(cameras[c][0], cameras[c][1], img)
        out.append((Camera(cameras[c], camera_poses[c], ft), np.asarray(obj, np.float32).astype(ft), obs.astype(ft)))
    return out


def residual_jacobian(pparts, rvec, tvec, param, ft=np.float64):
    """(r [2n], J [2n,6], norms [n]): per part the u rows then the v rows; norms in point order."""
    R, dR = rotation(rvec, param, ft)
    t = np.asarray(tvec, ft)
    rs, Js, norms = [], [], []
    for cam, X, obs in pparts:
        Q = (X @ R.T + t) @ cam.Rc.T + cam.tc
        iz = ft(1) / Q[:, 2]
        ru = cam.fx * Q[:, 0] * iz + cam.cx - obs[:, 0]
        rv = cam.fy * Q[:, 1] * iz + cam.cy - obs[:, 1]
        dQ = [(X @ dR[k].T) @ cam.Rc.T for k in range(3)] + [np.broadcast_to(cam.Rc[:, m], Q.shape) for m in range(3)]
        Ju = np.stack([cam.fx * (d[:, 0] * iz - Q[:, 0] * iz * iz * d[:, 2]) for d in dQ], 1)
        Jv = np.stack([cam.fy * (d[:, 1] * iz - Q[:, 1] * iz * iz * d[:, 2]) for d in dQ], 1)
        rs += [ru, rv]
        Js += [Ju, Jv]
        norms.append(np.sqrt(ru * ru + rv * rv))
    return np.concatenate(rs), np.concatenate(Js), np.concatenate(norms)


# ---- rules 1 and 5 ----------------------------------------------------------------------------------------------------------------

def scaled_inverse(H, ft=np.float64):
    """Rule 5: (cov / sigma2_used, min_pivot), or (None, None) for CTAG_COV_SINGULAR."""
    h = np.diag(H)
    if not (np.all(np.isfinite(h)) and np.all(h > 0)):
        return None, None
    d = ft(1) / np.sqrt(h)
    C = d[:, None] * H * d[None, :]
    L = np.zeros((6, 6), ft)
    min_pivot = None
    for j in range(6):
        p = C[j, j] - L[j, :j] @ L[j, :j]
        min_pivot = p if min_pivot is None or not p >= min_pivot else min_pivot
        if not p > MIN_PIVOT:
            return None, None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 6):
            L[i, j] = (C[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    W = np.zeros((6, 6), ft)  # L^-1
    for j in range(6):
        W[j, j] = ft(1) / L[j, j]
        for i in range(j + 1, 6):
            W[i, j] = -(L[i, j:i] @ W[j:i, j]) / L[i, i]
    return d[:, None] * (W.T @ W) * d[None, :], min_pivot


def covariance(pparts, rvec, tvec, opts, ft=np.float64):
    """Rules 3-5 at the pose (rvec, tvec): a dict of the record's fields in `ft` ("status" alone unless it is COV_OK)."""
    with np.errstate(all="ignore"):
        r, J, norms = residual_jacobian(pparts, rvec, tvec, opts["param"], ft)
        n = len(norms)
        cost = ft(0.5) * (r @ r)
        scaled, min_pivot = scaled_inverse(J.T @ J, ft)
        if scaled is None or not np.isfinite(cost):
            return {"status": COV_SINGULAR}
        dof = 2 * n - 6
        s2_hat = 2 * cost / dof
        s2 = ft(opts["sigma_px"]) ** 2 if opts["sigma_px"] > 0 else s2_hat
        worst = int(np.argmax(norms))  # the first of equal maxima
        n_out = int(np.count_nonzero(norms > ft(opts["outlier_k"]) * np.sqrt(s2))) if opts["outlier_k"] > 0 else 0
        return {"status": COV_OK, "n_points": n, "dof": dof, "worst_point": worst, "n_outliers": n_out, "param": opts["param"], "cost": cost,
                "sigma2_hat": s2_hat, "sigma2_used": s2, "max_residual_px": norms[worst], "min_pivot": min_pivot, "cov": np.triu(s2 * scaled) + np.triu(s2 * scaled, 1).T}


def expected(P, parts, cameras, camera_poses, opts, ft=np.float64):
    """The fields of the covariance record of source record P whose rebuilt points are `parts` (None: rule 2 failed)."""
    if int(P["status"]) != 0:
        return {"status": COV_NO_POSE}
    if parts is None:
        return {"status": COV_BAD_RECORD}
    return covariance(problem_parts(parts, cameras, camera_poses, ft), P["rvec"], P["tvec"], opts, ft)


def expected_marker(P, recs, model, camera, opts, ft=np.float64):
    parts = parts_of_marker(P, recs, model) if int(P["status"]) == 0 else None
    return expected(P, parts, [camera], [IDENTITY_POSE], opts, ft)


def expected_rig(P, recs, model, camera, opts, ft=np.float64):
    parts = parts_of_rig(P, recs, model) if int(P["status"]) == 0 else None
    return expected(P, parts, [camera], [IDENTITY_POSE], opts, ft)


def expected_mv(P, recs_per_camera, model, cameras, camera_poses, opts, ft=np.float64):
    parts = parts_of_mv(P, recs_per_camera, model) if int(P["status"]) == 0 else None
    return expected(P, parts, cameras, camera_poses, opts, ft)


def to_record(e):
    """The dict of expected() as a POSE_COV_DT record (rule 1: zero but for the status unless it is COV_OK)."""
    R = np.zeros((), POSE_COV_DT)
    for k, v in e.items():
        R[k] = np.asarray(v, np.float64) if k in DOUBLE_FIELDS else v
    return R


# ---- comparison ---------------------------------------------------------------------------------------------------------------------

def deviation(a, b):
    """The comparison figure of two COV_OK records / dicts (see the module's text); b is the reference."""
    cb = np.asarray(b["cov"], np.longdouble)
    da = np.abs(np.asarray(a["cov"], np.longdouble) - cb)
    s = np.sqrt(np.diag(cb))
    worst = float((da / np.outer(s, s)).max())
    for k in ("cost", "sigma2_hat", "sigma2_used", "max_residual_px"):
        va, vb = np.longdouble(a[k]), np.longdouble(b[k])
        if vb != 0 or va != 0:
            worst = max(worst, float(abs(va - vb) / abs(vb)))
    return max(worst, float(abs(np.longdouble(a["min_pivot"]) - np.longdouble(b["min_pivot"]))))


def check_cov_records(got, want, sources, bar=None, what=""):
    """Asserts that the device's records `got` are the statement's `want` (dicts of expected()) for the source records `sources`:
    status and every integer field equal; every status but COV_OK: all other bytes zero; COV_OK: |cost - source cost| <= 1e-9 *
    max(1, cost) (check_pose_records' bar), cov symmetric bit for bit, deviation(got, want) <= bar.  Returns the worst deviation."""
    bar = BAR if bar is None else bar
    assert len(got) == len(want) == len(sources), (what, len(got), len(want), len(sources))
    worst = 0.0
    for w, (G, E, P) in enumerate(zip(got, want, sources)):
        at = "%s record %d" % (what, w)
        assert int(G["status"]) == E["status"], (at, "status", int(G["status"]), E["status"])
        if E["status"] != COV_OK:
            assert G.tobytes()[4:] == bytes(POSE_COV_DT.itemsize - 4), (at, "fields set on status %d" % E["status"])
            continue
        for k in ("n_points", "dof", "worst_point", "n_outliers", "param"):
            assert int(G[k]) == int(E[k]), (at, k, int(G[k]), int(E[k]))
        assert abs(float(G["cost"]) - float(P["cost"])) <= 1e-9 * max(1.0, float(P["cost"])), (at, "cost", float(G["cost"]), float(P["cost"]))
        assert G["cov"].tobytes() == np.ascontiguousarray(G["cov"].T).tobytes(), (at, "cov is not symmetric bit for bit")
        d = deviation(G, E)
        worst = max(worst, d)
        assert d <= bar, (at, "deviation", d, bar)
    return worst
