"""An independent statement of the multi-view rig pose (include/ctag_pose.h, rules 1-5), in numpy / scipy only.

Nothing here comes from oracle/, cylindertag_amd/csrc or testkit.  It reuses pose_statement.py's correspondences, undistort12
(through observations / Problem), rodrigues and Problem.  A camera is (K 3x3, dist[n_dist]), a camera pose (rvec, tvec) with
X_cam = R(rvec) X_ref + tvec, a model {"ids", "size", "corners"}; one instant is a list of detection records, one per camera.

  membership        rule 1: cameras in order, per camera the rig rule (first model with the id, rig_of_model, the first marker
                    with a model index claims it, builder rejection), the 800-point bound over ALL cameras
  start_camera      rule 2: the most points, the lowest index on a tie
  to_reference      rule 4: R_start = Rc^T R(rvec_cam), t_start = Rc^T (tvec_cam - tc)
  MvProblem         rule 5: residual of point i of camera c under the rig pose (R, t): Q = Rc (R X + t) + tc, through camera c's
                    intrinsics, against camera c's own undistorted observation
  solve_instant     rules 1-5 with a caller-given stage 1 (EPnP + PoseBA are not restated here) and scipy's minimum for stage 2
  check_mv_records  what ctag_mv_pose_rec records must satisfy

EPnP and the LM loop are NOT restated step by step: check_mv_records states what they must reach."""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

from pose_statement import MIN_POINTS_FOR_MINIMUM, Problem, correspondences, model_lookup, project12, rodrigues

OK, TOO_FEW, DEGENERATE, NOT_SEEN = 0, 2, 4, 5
MAX_CAMERAS = 8
MAX_MARKERS = 100
RIG_MAX_POINTS = 800
MV_POSE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("n_cameras", "<i4"), ("start_camera", "<i4"),
                       ("n_members", "<i4"), ("n_excluded", "<i4"), ("n_points", "<i4"), ("iterations", "<i4"), ("iterations_cam", "<i4"),
                       ("points_of_camera", "<i4", (MAX_CAMERAS,)), ("member_mask", "<u4", (MAX_CAMERAS, 4)), ("reserved", "<i4", (2,)),
                       ("rvec_epnp", "<f8", (3,)), ("tvec_epnp", "<f8", (3,)), ("rvec_cam", "<f8", (3,)), ("tvec_cam", "<f8", (3,)),
                       ("cost_cam0", "<f8"), ("cost_cam", "<f8"), ("rvec_start", "<f8", (3,)), ("tvec_start", "<f8", (3,)), ("cost0", "<f8"),
                       ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("cost", "<f8")])
POSE_FIELDS = ("iterations", "iterations_cam", "rvec_epnp", "tvec_epnp", "rvec_cam", "tvec_cam", "cost_cam0", "cost_cam", "rvec_start",
               "tvec_start", "cost0", "rvec", "tvec", "cost")
HEADER_FIELDS = ("status", "rig", "frame", "n_cameras", "start_camera", "n_members", "n_excluded", "n_points", "points_of_camera",
                 "member_mask", "reserved")


def rotvec(R):
    """The way back from a rotation matrix (angles well inside (0, pi) here)."""
    return Rotation.from_matrix(np.asarray(R, np.float64)).as_rotvec()


def membership(records, model, rig_of_model, g):
    """Rule 1 for rig g at one instant.  Returns per camera (members [marker indices], obj float32 [n,3], img float32 [n,2]) and
    the number of excluded markers."""
    per_camera, excluded, total = [], 0, 0
    for rec in records:
        members, objs, imgs = [], [], []
        if int(rec["status"]) == 0:
            claimed = set()
            for k in range(min(max(int(rec["n_markers"]), 0), MAX_MARKERS)):
                mi = model_lookup(model, int(rec["markers"][k]["marker_id"]))
                if mi < 0 or int(rig_of_model[mi]) != g:
                    continue
                dup = mi in claimed
                claimed.add(mi)
                if dup:
                    excluded += 1
                    continue
                st, obj, img = correspondences(rec, k, model, mi)
                if st != OK or total + len(obj) > RIG_MAX_POINTS:
                    excluded += 1
                    continue
                members.append(k)
                objs.append(obj)
                imgs.append(img)
                total += len(obj)
        per_camera.append((members, np.concatenate(objs) if objs else np.zeros((0, 3), np.float32),
                           np.concatenate(imgs) if imgs else np.zeros((0, 2), np.float32)))
    return per_camera, excluded


def start_camera(points_of_camera):
    """Rule 2: the most points, the lowest index on a tie."""
    best = 0
    for c, n in enumerate(points_of_camera):
        if n > points_of_camera[best]:
            best = c
    return best


def to_reference(rvec_cam, tvec_cam, camera_pose):
    """Rule 4: the pose of the rig in the reference frame from its pose in a camera's frame."""
    Rc, tc = rodrigues(camera_pose[0]), np.asarray(camera_pose[1], np.float64)
    if not np.any(camera_pose[0]) and not np.any(camera_pose[1]):
        return np.array(rvec_cam, np.float64), np.array(tvec_cam, np.float64)
    return rotvec(Rc.T @ rodrigues(rvec_cam)), Rc.T @ (np.asarray(tvec_cam, np.float64) - tc)


class MvProblem:
    """Rule 5: the least-squares problem of stage 2.  parts = [(camera index, obj, img)] in camera order."""

    def __init__(self, cameras, camera_poses, parts):
        self.parts = []
        for c, obj, img in parts:
            if len(obj):
                K, dist = cameras[c]
                self.parts.append((Problem(K, dist, obj, img), rodrigues(camera_poses[c][0]), np.asarray(camera_poses[c][1], np.float64)))
        self.n_points = sum(len(p.X) for p, _, _ in self.parts)

    def residual(self, p):
        R, t = rodrigues(p[:3]), np.asarray(p[3:], np.float64)
        out = []
        for pb, Rc, tc in self.parts:
            Q = (pb.X @ R.T + t) @ Rc.T + tc
            out.append(pb.fx * Q[:, 0] / Q[:, 2] + pb.cx - pb.obs[:, 0])
            out.append(pb.fy * Q[:, 1] / Q[:, 2] + pb.cy - pb.obs[:, 1])
        return np.concatenate(out)

    def cost_at(self, rvec, tvec):
        r = self.residual(np.concatenate([np.asarray(rvec, np.float64), np.asarray(tvec, np.float64)]))
        return 0.5 * float(r @ r)

    def minimum_from(self, rvec0, tvec0):
        """scipy's minimum from the stage-2 start, with pose_statement.Problem.minimum_from's settings."""
        return least_squares(self.residual, np.concatenate([rvec0, tvec0]), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                             x_scale="jac", jac="3-point")


def expected_header(records, model, rig_of_model, g, frame, start_rule=start_camera):
    """The integer fields of the record of (frame, rig g), and its membership."""
    per_camera, excluded = membership(records, model, rig_of_model, g)
    H = np.zeros((), MV_POSE_DT)
    H["rig"], H["frame"], H["n_excluded"] = g, frame, excluded
    for c, (members, obj, _) in enumerate(per_camera):
        H["points_of_camera"][c] = len(obj)
        for k in members:
            H["member_mask"][c][k >> 5] |= np.uint32(1 << (k & 31))
    H["n_members"] = sum(len(m) for m, _, _ in per_camera)
    H["n_cameras"] = sum(1 for m, _, _ in per_camera if m)
    H["n_points"] = int(H["points_of_camera"].sum())
    H["start_camera"] = start_rule([int(v) for v in H["points_of_camera"][:len(records)]])
    if H["n_members"] == 0:
        H["status"] = NOT_SEEN
    elif H["points_of_camera"][H["start_camera"]] < 4:
        H["status"] = TOO_FEW
    return H, per_camera


def solve_instant(records, model, rig_of_model, n_rigs, cameras, camera_poses, stage1, frame=0, start_rule=start_camera):
    """Rules 1-5 for one instant -> n_rigs MV_POSE_DT records.  stage1(K, dist, obj, img) -> None for a degenerate problem, else
    (rvec_epnp, tvec_epnp, rvec_cam, tvec_cam, cost_cam0, cost_cam, iterations_cam): the one-camera EPnP + PoseBA, which this
    statement does not restate.  Stage 2 is scipy's minimum (iterations is set to 1 where it ran)."""
    out = np.zeros(n_rigs, MV_POSE_DT)
    for g in range(n_rigs):
        H, per_camera = expected_header(records, model, rig_of_model, g, frame, start_rule)
        out[g] = H
        if H["status"] != OK:
            continue
        sc = int(H["start_camera"])
        s1 = stage1(cameras[sc][0], cameras[sc][1], per_camera[sc][1], per_camera[sc][2])
        if s1 is None:
            out[g]["status"] = DEGENERATE
            continue
        R = out[g]
        R["rvec_epnp"], R["tvec_epnp"], R["rvec_cam"], R["tvec_cam"], R["cost_cam0"], R["cost_cam"], R["iterations_cam"] = s1
        R["rvec_start"], R["tvec_start"] = to_reference(R["rvec_cam"], R["tvec_cam"], camera_poses[sc])
        if int(H["n_points"]) == int(H["points_of_camera"][sc]):
            R["rvec"], R["tvec"], R["cost0"], R["cost"] = R["rvec_start"], R["tvec_start"], R["cost_cam"], R["cost_cam"]
            continue
        pb = MvProblem(cameras, camera_poses, [(c, o, i) for c, (_, o, i) in enumerate(per_camera)])
        sol = pb.minimum_from(R["rvec_start"], R["tvec_start"])
        R["cost0"] = pb.cost_at(R["rvec_start"], R["tvec_start"])
        R["rvec"], R["tvec"], R["iterations"] = sol.x[:3], sol.x[3:], 1
        R["cost"] = min(pb.cost_at(sol.x[:3], sol.x[3:]), float(R["cost0"]))
    return out


last_stats = {}  # worst figures of the most recent check_mv_records call, for reports


def check_mv_records(got, records, model, rig_of_model, n_rigs, cameras, camera_poses, degenerate=None, planted=None, minimum=True):
    """Asserts that `got` (n_frames * n_rigs ctag_mv_pose_rec records) are the multi-view rig poses of records[c][f] (camera c,
    frame f):

      1. every integer field of the header, points_of_camera, member_mask and start_camera equal the statement's.  DEGENERATE is
         accepted exactly where degenerate(frame, rig) says so; there, and for every status but OK, the pose fields are zero.
      2. status OK: cost_cam0 / cost_cam against the start camera's own problem at (rvec_epnp, tvec_epnp) / (rvec_cam, tvec_cam),
         cost0 / cost against the stage-2 problem at (rvec_start, tvec_start) / (rvec, tvec): |difference| <= 1e-9 * max(1, cost);
         cost <= cost0, cost_cam <= cost_cam0; 0 <= iterations, iterations_cam <= 50.
      3. status OK: (rvec_start, tvec_start) equal numpy's move of (rvec_cam, tvec_cam) to 1e-12, and are its bytes when the start
         camera's pose is zero.  Every point with the start camera: iterations = 0, cost0 = cost = cost_cam, (rvec, tvec) are the
         bytes of (rvec_start, tvec_start).
      4. status OK, n_points >= 16 (`minimum`): against min = scipy's minimum from (rvec_start, tvec_start):
         cost <= min.cost * (1 + 1e-9) + 1e-12, |rvec - min.x[:3]| < 1e-6, |tvec - min.x[3:]| < 1e-4 * max|tvec|.
      5. planted[frame][rig] = (rvec, tvec) given (noise-free input): the same two bars of 4 against the planted pose.

    Returns (OK records, records that got check 4)."""
    n_cam = len(cameras)
    n_frames = len(records[0])
    degenerate = degenerate or (lambda frame, rig: False)
    assert len(got) == n_frames * n_rigs, "%d records for %d items" % (len(got), n_frames * n_rigs)
    stats = {"ok": 0, "minimum_checks": 0, "cost_rel": 0.0, "move_r": 0.0, "move_t": 0.0, "min_cost_excess": 0.0, "drvec": 0.0,
             "dtvec_rel": 0.0, "planted_drvec": 0.0, "planted_dtvec_rel": 0.0}
    for f in range(n_frames):
        inst = [records[c][f] for c in range(n_cam)]
        for g in range(n_rigs):
            P = got[f * n_rigs + g]
            what = "frame %d rig %d" % (f, g)
            H, per_camera = expected_header(inst, model, rig_of_model, g, f)
            st = int(H["status"])
            if st == OK and degenerate(f, g):
                st = DEGENERATE
            assert int(P["status"]) == st, (what, "status", int(P["status"]), st)
            for k in HEADER_FIELDS[1:]:
                assert np.array_equal(P[k], H[k]), (what, k, P[k], H[k])
            if st != OK:
                for k in POSE_FIELDS:
                    assert not np.any(P[k]), (what, k, "set on status %d" % st)
                continue
            stats["ok"] += 1
            sc = int(H["start_camera"])
            one = Problem(cameras[sc][0], cameras[sc][1], per_camera[sc][1], per_camera[sc][2])
            pb = MvProblem(cameras, camera_poses, [(c, o, i) for c, (_, o, i) in enumerate(per_camera)])
            assert pb.n_points == int(P["n_points"])
            assert 0 <= int(P["iterations"]) <= 50 and 0 <= int(P["iterations_cam"]) <= 50, what
            assert P["cost"] <= P["cost0"] and P["cost_cam"] <= P["cost_cam0"], what
            for prob, ck, rk, tk, ref in ((one, "cost_cam0", "rvec_epnp", "tvec_epnp", "cost_cam"), (one, "cost_cam", "rvec_cam", "tvec_cam", "cost_cam"),
                                          (pb, "cost0", "rvec_start", "tvec_start", "cost"), (pb, "cost", "rvec", "tvec", "cost")):
                d = abs(prob.cost_at(P[rk], P[tk]) - float(P[ck])) / max(1.0, float(P[ref]))
                stats["cost_rel"] = max(stats["cost_rel"], d)
                assert d <= 1e-9, (what, ck, d)
            rs, ts = to_reference(P["rvec_cam"], P["tvec_cam"], camera_poses[sc])
            if not np.any(camera_poses[sc][0]) and not np.any(camera_poses[sc][1]):
                assert P["rvec_start"].tobytes() == P["rvec_cam"].tobytes() and P["tvec_start"].tobytes() == P["tvec_cam"].tobytes(), what
            mr, mt = float(np.abs(P["rvec_start"] - rs).max()), float(np.abs(P["tvec_start"] - ts).max())
            stats["move_r"], stats["move_t"] = max(stats["move_r"], mr), max(stats["move_t"], mt)
            assert mr <= 1e-12 and mt <= 1e-12, (what, "move", mr, mt)
            if int(P["n_points"]) == int(P["points_of_camera"][sc]):
                assert int(P["iterations"]) == 0 and P["cost0"] == P["cost"] == P["cost_cam"], what
                assert P["rvec"].tobytes() == P["rvec_start"].tobytes() and P["tvec"].tobytes() == P["tvec_start"].tobytes(), what
            bars = []
            if minimum and int(P["n_points"]) >= MIN_POINTS_FOR_MINIMUM:
                sol = pb.minimum_from(P["rvec_start"], P["tvec_start"])
                stats["min_cost_excess"] = max(stats["min_cost_excess"], (float(P["cost"]) - sol.cost) / max(sol.cost, 1e-300))
                assert P["cost"] <= sol.cost * (1 + 1e-9) + 1e-12, (what, float(P["cost"]), sol.cost)
                bars.append(("drvec", "dtvec_rel", sol.x[:3], sol.x[3:]))
                stats["minimum_checks"] += 1
            if planted is not None and int(P["n_points"]) >= MIN_POINTS_FOR_MINIMUM:
                bars.append(("planted_drvec", "planted_dtvec_rel", planted[f][g][0], planted[f][g][1]))
            for kr, kt, rv, tv in bars:
                dr = float(np.abs(P["rvec"] - rv).max())
                dt = float(np.abs(P["tvec"] - tv).max() / np.abs(P["tvec"]).max())
                stats[kr], stats[kt] = max(stats[kr], dr), max(stats[kt], dt)
                assert dr < 1e-6, (what, kr, dr)
                assert dt < 1e-4, (what, kt, dt)
    last_stats.clear()
    last_stats.update(stats)
    return stats["ok"], stats["minimum_checks"]


# ---- synthetic instants ------------------------------------------------------------------------------------------------------

def ring_poses(centre, angles_deg, shifts=None):
    """Cameras round the point `centre` (reference coordinates): camera c is turned by angles_deg[c] about the axis through
    `centre` parallel to y and keeps `centre` at the same place in its own frame, plus shifts[c]."""
    centre = np.asarray(centre, np.float64)
    out = []
    for c, a in enumerate(angles_deg):
        rv = np.array([0.0, np.radians(a), 0.0])
        tv = centre - rodrigues(rv) @ centre + (np.asarray(shifts[c], np.float64) if shifts is not None else 0.0)
        out.append((rv, tv))  # an angle of 0 without a shift is the reference itself: exactly zero
    return out


def project_camera(camera, camera_pose, rvec, tvec, X):
    """Pixels of the model points X under the rig pose (rvec, tvec) in the reference frame, seen by one camera of the set."""
    Q = (np.asarray(X, np.float64) @ rodrigues(rvec).T + np.asarray(tvec, np.float64)) @ rodrigues(camera_pose[0]).T + np.asarray(camera_pose[1], np.float64)
    return project12(camera[0], camera[1], np.zeros(3), np.zeros(3), Q)
