"""An independent statement of the camera set fit (include/ctag_pose.h, camera set fit, rules 1-6), in numpy / scipy only.  Nothing
here comes from oracle/, cylindertag_amd/csrc or testkit; the membership of an instant is mv_statement's, the correspondences, the
undistortion and the float32 observations are pose_statement's.  What is stated:

  rig_records        rule 1: every camera's own rig pose of every (instant, rig) item, by scipy's minimum from a given start (EPnP and
                     the Ceres loop are NOT restated: check what they must reach), and whether it counts for the start
  initial_assembly   rule 2: shared-item counts, anchor, tree, edge transforms, the poses in the anchor's frame
  Observations       rule 3: the items that take part, all their points in one flat list, and the residual of rule 4 in any
                     floating-point type
  reduced_system     S = sum (Q Jc)^T (Q Jc), g = sum (Q Jc)^T r with Q = I - Jp (Jp^T Jp)^-1 Jp^T, Jacobians by central differences of
                     the statement's own residual
  step               (S + lambda diag S) delta = -g with the anchor's rows dropped
  fit                the Levenberg-Marquardt loop of rule 4 in double
  joint_minimum      scipy.optimize.least_squares over the camera poses AND the rig poses together

A camera state is (R [C, 3, 3], t [C, 3]) with X_cam = R X_anchor + t.  The bars the device is held to are the constants at the end;
tests/test_cam_fit_statement_cpu.py measures them again on every run, DESIGN.md section 17 says where each came from."""
import numpy as np
from scipy import sparse
from scipy.optimize import least_squares

import mv_statement as mv
import pose_statement as ps

OK, NOT_SEEN = 0, 5
TRANSLATION_STEP = 100.0   # central-difference step of a translation, in units of the rotation's (mm against radians at ~1000 mm)
DENSE_RECORDS = 200        # joint_minimum: more records than this take scipy's sparse trust-region solver


def step_of(T):
    """Central-difference step for a type: eps^(1/3)."""
    return T(np.finfo(T).eps) ** (T(1) / T(3))


def rot_many(rv, T=np.float64):
    """Rodrigues' formula for rotation vectors [m, 3] in type T -> [m, 3, 3]."""
    rv = np.asarray(rv, T).reshape(-1, 3)
    th = np.sqrt((rv * rv).sum(1))
    small = th < T(1e-12)
    ths = np.where(small, T(1), th)
    a = np.where(small, T(1), np.sin(ths) / ths)
    b = np.where(small, T(0.5), T(2) * np.sin(ths / 2) ** 2 / (ths * ths))
    K = np.zeros((len(rv), 3, 3), T)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -rv[:, 2], rv[:, 1], rv[:, 2], -rv[:, 0], -rv[:, 1], rv[:, 0]
    return np.eye(3, dtype=T) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def rot(rv, T=np.float64):
    return rot_many(rv, T)[0]


def compose(d, R, t, wrong=None):
    """Exp(d) o (R, t): R <- Exp(w) R, t <- Exp(w) t + v, for every camera (d [C, 6]), in R's type."""
    T = R.dtype.type
    d = np.asarray(d, T).reshape(-1, 6)
    E = rot_many(-d[:, :3] if wrong == "cross sign" else d[:, :3], T)
    tn = t + d[:, 3:] if wrong == "update without Exp(w) tc" else np.einsum("cij,cj->ci", E, t) + d[:, 3:]
    return E @ R, tn


# ---------------------------------------------------------------------------------------------------------------------
# rule 1
# ---------------------------------------------------------------------------------------------------------------------
def rig_records(records, model, rig_of_model, n_rigs, cameras, start_of, min_points=8, wrong=None):
    """records[c][f].  {(camera, item): dict(pose [6], n_points, counted)} of every item (item = f * n_rigs + g) in which camera c has
    a member and at least 4 points: the minimum from start_of(camera, frame, rig) of that camera's own problem."""
    out = {}
    for c in range(len(records)):
        K, dist = cameras[0 if wrong == "camera 0's coefficients" else c][0], cameras[0 if wrong == "camera 0's coefficients" else c][1]
        for f, rec in enumerate(records[c]):
            for g in range(n_rigs):
                (members, obj, img), = mv.membership([rec], model, rig_of_model, g)[0]
                if not members or len(obj) < 4:
                    continue
                r0, t0 = start_of(c, f, g)
                sol = ps.Problem(K, dist, obj, img).minimum_from(np.asarray(r0, np.float64), np.asarray(t0, np.float64))
                out[(c, f * n_rigs + g)] = {"pose": sol.x, "n_points": len(obj), "counted": len(obj) >= min_points}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rule 2
# ---------------------------------------------------------------------------------------------------------------------
def shared_counts(rr, n_cameras, n_items):
    seen = np.array([[(c, i) in rr and rr[(c, i)]["counted"] for c in range(n_cameras)] for i in range(n_items)], np.int64).reshape(n_items, n_cameras)
    cnt = seen.T @ seen
    np.fill_diagonal(cnt, 0)
    return cnt


def initial_assembly(rr, n_cameras, n_items, min_items=2, wrong=None):
    """Rule 2.  Returns dict(anchor (-1: none), placed [camera indices, ascending], parent {camera: camera}, n_with_parent, T {camera:
    (R, t)}, counts).  wrong: "edge direction", "tie order", "per-item rotation" -- planted errors for the statement's own tests."""
    cnt = shared_counts(rr, n_cameras, n_items)
    out = {"anchor": -1, "placed": [], "parent": {}, "n_with_parent": {}, "T": {}, "counts": cnt}
    ok = [a for a in range(n_cameras) if cnt[a].max() >= min_items]
    if not ok:
        return out
    a0 = ok[0]
    out["anchor"] = a0
    placed = [a0]
    out["T"][a0] = (np.eye(3), np.zeros(3))
    while True:
        best = None
        for b in range(n_cameras):
            if b in placed:
                continue
            for a in sorted(placed):
                if cnt[a, b] >= min_items and (best is None or cnt[a, b] > best[0] or (wrong == "tie order" and cnt[a, b] == best[0])):
                    best = (cnt[a, b], a, b)
        if best is None:
            break
        n, a, b = best
        items = [i for i in range(n_items) if (a, i) in rr and (b, i) in rr and rr[(a, i)]["counted"] and rr[(b, i)]["counted"]]
        sR = np.zeros((3, 3))
        for i in items:
            Ra, Rb = rot(rr[(a, i)]["pose"][:3]), rot(rr[(b, i)]["pose"][:3])
            sR += Ra.T @ Rb if wrong == "edge direction" else Rb @ Ra.T
        U, _, Vt = np.linalg.svd(sR)
        Rbar = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
        st = np.zeros(3)
        for i in items:
            pa, pb = rr[(a, i)]["pose"], rr[(b, i)]["pose"]
            Ri = rot(pb[:3]) @ rot(pa[:3]).T if wrong == "per-item rotation" else Rbar
            st += pb[3:] - Ri @ pa[3:]
        Ta = out["T"][a]
        out["T"][b] = (Rbar @ Ta[0], Rbar @ Ta[1] + st / n)
        out["parent"][b], out["n_with_parent"][b] = a, int(n)
        placed.append(b)
    out["placed"] = sorted(placed)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rule 3 and the residual of rule 4
# ---------------------------------------------------------------------------------------------------------------------
class Observations:
    """The observation records of a call over the cameras `placed` (slot k = camera placed[k]): every item in which at least two of
    them have members and the start camera (the most points, the lowest slot on a tie) has at least 4 points, and ok_of(item) if given
    (the device's record is CTAG_POSE_OK).  All points in one flat list in camera, marker, builder order."""

    def __init__(self, records, model, rig_of_model, n_rigs, cameras, placed, ok_of=None, dtype=np.float64, wrong=None):
        T = self.dtype = dtype
        self.placed = list(placed)
        self.items, self.n_points, self.points_of_camera = [], [], []
        X, obs, cam, rec = [], [], [], []
        n_frames = len(records[0])
        for f in range(n_frames):
            inst = [records[c][f] for c in self.placed]
            for g in range(n_rigs):
                per_camera, _ = mv.membership(inst, model, rig_of_model, g)
                pts = [len(o) for _, o, _ in per_camera]
                if sum(1 for m, _, _ in per_camera if m) < 2 or max(pts) < 4 or (ok_of is not None and not ok_of(f * n_rigs + g)):
                    continue
                r = len(self.items)
                self.items.append(f * n_rigs + g)
                self.n_points.append(sum(pts))
                self.points_of_camera.append(pts)
                for k, (_, o, im) in enumerate(per_camera):
                    if len(o):
                        K, dist = cameras[self.placed[0 if wrong == "camera 0's coefficients" else k]]
                        X.append(np.asarray(o, np.float32).astype(np.float64))
                        obs.append(ps.observations(K, dist, im))
                        cam.append(np.full(len(o), k))
                        rec.append(np.full(len(o), r))
        self.R = len(self.items)
        self.X = np.concatenate(X).astype(T) if X else np.zeros((0, 3), T)
        self.obs = np.concatenate(obs).astype(T) if obs else np.zeros((0, 2), T)
        self.cam = np.concatenate(cam).astype(np.int64) if cam else np.zeros(0, np.int64)
        self.rec = np.concatenate(rec).astype(np.int64) if rec else np.zeros(0, np.int64)
        intr = np.array([ps._intrinsics(cameras[c][0]) for c in self.placed], T)
        self.f = intr[self.cam][:, :2]
        self.c = intr[self.cam][:, 2:]

    def residual(self, Rc, tc, poses):
        """[n, 2]: point i of camera c under the rig pose of its record: Q = Rc (R X + t) + tc through camera c's intrinsics."""
        T = self.dtype
        poses = np.asarray(poses, T)
        Rp = rot_many(poses[:, :3], T)
        P = np.einsum("nij,nj->ni", Rp[self.rec], self.X) + poses[self.rec, 3:]
        Q = np.einsum("nij,nj->ni", np.asarray(Rc, T)[self.cam], P) + np.asarray(tc, T)[self.cam]
        return self.f * Q[:, :2] / Q[:, 2:3] + self.c - self.obs

    def costs(self, Rc, tc, poses):
        r = self.residual(Rc, tc, poses)
        return 0.5 * np.bincount(self.rec, (r * r).sum(1).astype(np.float64), self.R)

    def jac_pose(self, Rc, tc, poses, h):
        """[n, 2, 6]: d residual / d (rvec, tvec) of the point's record."""
        T = self.dtype
        poses = np.asarray(poses, T)
        J = np.zeros((len(self.X), 2, 6), T)
        for a in range(6):
            s = h * (T(TRANSLATION_STEP) if a >= 3 else T(1))
            d = np.zeros(6, T)
            d[a] = s
            J[:, :, a] = (self.residual(Rc, tc, poses + d) - self.residual(Rc, tc, poses - d)) / (2 * s)
        return J

    def jac_camera(self, Rc, tc, poses, h, wrong=None):
        """[n, 2, 6]: d residual / d (w, v) of the point's camera at (w, v) = 0."""
        T = self.dtype
        Rc, tc = np.asarray(Rc, T), np.asarray(tc, T)
        J = np.zeros((len(self.X), 2, 6), T)
        for a in range(6):
            s = h * (T(TRANSLATION_STEP) if a >= 3 else T(1))
            d = np.zeros((len(Rc), 6), T)
            d[:, a] = s
            J[:, :, a] = (self.residual(*compose(d, Rc, tc, wrong), poses) - self.residual(*compose(-d, Rc, tc, wrong), poses)) / (2 * s)
        if wrong == "camera dropped":
            J[self.cam == len(Rc) - 1] = 0
        return J

    def solve_poses(self, Rc, tc, poses0, iters=30):
        """Every record's rig pose under the cameras: Gauss-Newton from poses0 (float64)."""
        assert self.dtype == np.float64
        poses = np.array(poses0, np.float64)
        h = step_of(np.float64)
        for _ in range(iters):
            r = self.residual(Rc, tc, poses)
            J = self.jac_pose(Rc, tc, poses, h)
            H = np.zeros((self.R, 6, 6))
            b = np.zeros((self.R, 6))
            np.add.at(H, self.rec, np.einsum("nka,nkb->nab", J, J))
            np.add.at(b, self.rec, np.einsum("nka,nk->na", J, r))
            d = np.linalg.solve(H, -b[..., None])[..., 0]
            poses = poses + d
            if np.abs(d).max() < 1e-13 * max(1.0, np.abs(poses).max()):
                break
        return poses


# ---------------------------------------------------------------------------------------------------------------------
# the reduced system: the unknowns of slot k are 6k .. 6k+5 (w, v) of camera placed[k]
# ---------------------------------------------------------------------------------------------------------------------
def _solve_spd(A, B):
    """A^-1 B for a symmetric positive definite A by Cholesky, in A's type (numpy.linalg has no long double).  Returns (X, positive definite?)."""
    T = A.dtype.type
    n = len(A)
    L = np.zeros((n, n), T)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            return np.zeros_like(B), False
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.array(B, T)
    for i in range(n):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y, True


def reduced_system(O, Rc, tc, poses, reverse=False, wrong=None):
    """S [6C, 6C], g [6C] at (Rc, tc, poses) over ALL camera slots (the anchor's included): the sum over the records, in record order
    (reversed: the other way round), of (Q Jc)^T (Q Jc) and (Q Jc)^T r."""
    T = O.dtype
    h = step_of(T)
    C = len(Rc)
    N = 6 * C
    Jp = O.jac_pose(Rc, tc, poses, h)
    Jc = O.jac_camera(Rc, tc, poses, h, wrong)
    res = O.residual(Rc, tc, poses)
    S, g = np.zeros((N, N), T), np.zeros(N, T)
    order = np.argsort(O.rec, kind="stable")
    bounds = np.searchsorted(O.rec[order], np.arange(O.R + 1))
    for r in (range(O.R - 1, -1, -1) if reverse else range(O.R)):
        idx = order[bounds[r]:bounds[r + 1]]
        n = len(idx)
        A = Jp[idx].reshape(2 * n, 6)
        B = np.zeros((n, 2, N), T)
        for a in range(6):
            B[np.arange(n), :, 6 * O.cam[idx] + a] = Jc[idx, :, a]
        B = B.reshape(2 * n, N)
        X, pd = _solve_spd(A.T @ A, A.T @ B)
        assert pd
        M = B - A @ X
        S += M.T @ M
        g += M.T @ res[idx].reshape(2 * n)
    return S, g


def step(S, g, anchor, lam):
    """(S + lambda diag S) delta = -g without the anchor slot's rows (0 there).  Returns (delta, positive definite?)."""
    T = S.dtype.type
    N = len(g)
    keep = np.array([i // 6 != anchor for i in range(N)])
    A = S[np.ix_(keep, keep)].copy()
    A[np.diag_indices_from(A)] += T(lam) * np.diag(A)
    d, pd = _solve_spd(A, -g[keep])
    out = np.zeros(N, T)
    if pd:
        out[keep] = d
    return out, pd


def system_deviation(S, g, d, S_ref, g_ref, d_ref, cost):
    """Scaled deviations: S entries over sqrt(S_ii S_jj), g entries over sqrt(S_ii) |r| (|r| = sqrt(2 cost)), delta over its largest entry."""
    S_ref, g_ref, d_ref = (np.asarray(v, np.longdouble) for v in (S_ref, g_ref, d_ref))
    sd = np.sqrt(np.diag(S_ref))
    sd = np.where(sd > 0, sd, 1)
    eS = float((np.abs(np.asarray(S, np.longdouble) - S_ref) / np.outer(sd, sd)).max())
    eg = float((np.abs(np.asarray(g, np.longdouble) - g_ref) / (sd * max(np.sqrt(2 * cost), 1e-300))).max())
    ed = float(np.abs(np.asarray(d, np.longdouble) - d_ref).max() / max(float(np.abs(d_ref).max()), 1e-300))
    return eS, eg, ed


# ---------------------------------------------------------------------------------------------------------------------
# the loop of rule 4 and the joint minimum
# ---------------------------------------------------------------------------------------------------------------------
def fit(O, Rc0, tc0, anchor, poses0, max_rounds=30, lambda0=1e-3, lambda_max=1e6, rel_tol=1e-12, wrong=None):
    """Rule 4 from the state (Rc0, tc0): returns dict(R, t, poses, cost_init, cost, rounds, lam).  wrong: "cross sign", "update without
    Exp(w) tc" (in the update only), "anchor at 0", "camera dropped" -- planted errors for the statement's own tests."""
    Rc, tc = np.array(Rc0, np.float64), np.array(tc0, np.float64)
    poses = O.solve_poses(Rc, tc, poses0)
    cost = cost_init = float(O.costs(Rc, tc, poses).sum())
    lam, rounds = lambda0, 0
    dropped = 0 if wrong == "anchor at 0" else anchor
    while rounds < max_rounds:
        rounds += 1
        S, g = reduced_system(O, Rc, tc, poses, wrong=wrong if wrong in ("cross sign", "camera dropped") else None)
        d, pd = step(S, g, dropped, lam)
        good = False
        if pd:
            Rt, tt = compose(d.reshape(-1, 6), Rc, tc, wrong if wrong == "update without Exp(w) tc" else None)
            tp = O.solve_poses(Rt, tt, poses)
            c = float(O.costs(Rt, tt, tp).sum())
            good = c < cost
        if good:
            drop, cost, Rc, tc, poses = cost - c, c, Rt, tt, tp
            lam = max(lam / 3, 1e-9)
            if drop < rel_tol * cost:
                break
        else:
            lam *= 4
            if lam > lambda_max:
                break
    return {"R": Rc, "t": tc, "poses": poses, "cost_init": cost_init, "cost": cost, "rounds": rounds, "lam": lam}


def joint_minimum(O, Rc0, tc0, anchor, poses0):
    """The minimum over the camera poses AND the rig poses together by scipy.optimize.least_squares from (Rc0, tc0, poses0); the
    anchor's pose stays.  Unknowns: d_c with (R_c, t_c) = Exp(d_c) o (Rc0, tc0), and the poses.  Returns dict(R, t, poses, cost)."""
    Rc0, tc0 = np.array(Rc0, np.float64), np.array(tc0, np.float64)
    C, R = len(Rc0), O.R
    free = [k for k in range(C) if k != anchor]
    col_of = -np.ones(C, np.int64)
    col_of[free] = 6 * np.arange(len(free))
    nd = 6 * len(free)
    h = step_of(np.float64)
    big = R > DENSE_RECORDS

    def unpack(v):
        d = np.zeros((C, 6))
        d[free] = v[:nd].reshape(-1, 6)
        Rc, tc = compose(d, Rc0, tc0)
        return Rc, tc, v[nd:].reshape(R, 6)

    def fun(v):
        return O.residual(*unpack(v)).ravel()

    def jac(v):
        Rc, tc, poses = unpack(v)
        Jp = O.jac_pose(Rc, tc, poses, h)
        # the camera columns at d: Exp(e) Exp(d) o T0, to first order in e the tangent at the current state
        Jc = O.jac_camera(Rc, tc, poses, h)
        n = len(O.X)
        rows = np.broadcast_to(2 * np.arange(n)[:, None, None] + np.arange(2)[None, :, None], (n, 2, 6))
        cp = np.broadcast_to(nd + 6 * O.rec[:, None, None] + np.arange(6)[None, None, :], (n, 2, 6))
        moving = col_of[O.cam] >= 0
        cc = np.broadcast_to(col_of[O.cam][:, None, None] + np.arange(6)[None, None, :], (n, 2, 6))
        J = sparse.coo_matrix((np.concatenate([Jp.ravel(), Jc[moving].ravel()]),
                               (np.concatenate([rows.ravel(), rows[moving].ravel()]), np.concatenate([cp.ravel(), cc[moving].ravel()]))),
                              shape=(2 * n, nd + 6 * R)).tocsr()
        return J if big else J.toarray()

    poses0 = O.solve_poses(Rc0, tc0, poses0)
    v0 = np.concatenate([np.zeros(nd), poses0.ravel()])
    # jac() gives the tangent at the current state, not d/dv of Exp(v) o T0; the two agree to first order in v, which stays below 1e-2 here
    sol = least_squares(fun, v0, jac=jac, method="trf", tr_solver="lsmr" if big else "exact", xtol=1e-14, ftol=1e-14, gtol=1e-13, x_scale=1.0, max_nfev=60)
    Rc, tc, poses = unpack(sol.x)
    poses = O.solve_poses(Rc, tc, poses)
    return {"R": Rc, "t": tc, "poses": poses, "cost": float(O.costs(Rc, tc, poses).sum())}


def pose_distance(Ra, ta, Rb, tb, distance):
    """(the largest rotation angle between two camera states, rad; the largest translation difference relative to `distance`)."""
    dr = max(float(np.linalg.norm(mv.rotvec(Ra[k] @ Rb[k].T))) for k in range(len(Ra)))
    dt = float(np.abs(np.asarray(ta) - np.asarray(tb)).max()) / distance
    return dr, dt


# The float64 statement against the same computation in numpy.longdouble -- from the cameras' (rvec, tvec) on, at the rule-2 start with
# every record's rig pose at its minimum -- worst over the shapes, AS MEASURED (three digits).  g is the largest: it is taken relative to
# the residual, and the noise-free cases' residual at that state is the float32 rounding of the pixels, 1e-8 of a pixel coordinate;
# tests/test_cam_fit_statement_cpu.py::test_measured_bars measures them again on every run and fails when a figure here is off by
# more than 2 %.  The device is allowed 16 x these.
SYSTEM_ERR = {"S": 2.95e-10, "g": 3.26e-9, "delta": 5.21e-8}
SYSTEM_BAR = {k: 16 * v for k, v in SYSTEM_ERR.items()}
CAMERA_DISTANCE_MM = 1000.0
# the distance between two joint minima from different starts and the move float32 rounding of the pixel coordinates alone causes on the
# noise-free shapes, (rotation rad, translation relative to the camera distance), as measured
MINIMA_DISTANCE = (6.36e-10, 4.93e-10)
F32_PIXEL_MOVE = (2.79e-7, 1.84e-7)
POSE_BAR = tuple(16 * max(a, b) for a, b in zip(MINIMA_DISTANCE, F32_PIXEL_MOVE))
# the relative change of rule 3's cost when the returned set of a 0.1 px case is re-solved by the public multi-view call after a one-ulp
# change of one camera pose entry, worst over the cases and entries, as tools/cam_fit_rel_tol.py measures it on the device (it needs the
# device's inner solves, so no CPU test can measure it again); the default rel_tol is 4 x
REL_TOL_ULP = 1.535e-13
