"""An independent statement of the model reconstruction (include/ctag_pose.h, model reconstruction, rules 1-8), in numpy / scipy
only.  Nothing here comes from oracle/, cylindertag_amd/csrc or testkit; the observation rule is pose_statement's (correspondences,
undistortion, float32 observations).  What is stated:

  observations       the records of a batch that take part, each as (model index, corner ids in the builder's order, observations)
  held               corners seen by fewer than min_obs records
  solve_poses        every record's pose at a model (best_poses: from several starts): Gauss-Newton on the reprojection residual, numerical Jacobians, all records
                     at once (EPnP and the Ceres loop are NOT restated: check what they must reach)
  reduced_system     S = sum (Q Jx)^T (Q Jx), g = sum (Q Jx)^T r with Q = I - Jp (Jp^T Jp)^-1 Jp^T from central differences, in any
                     floating-point type (float64, or numpy.longdouble to measure float64's own error)
  step               (S + lambda diag S) delta = -g on the fitted corners
  gauge, metric_scale   rules 5 and 6
  fit                the Levenberg-Marquardt loop of rule 4 on the variable-projection cost
  joint_minimum      scipy.optimize.least_squares over fitted corners AND poses together, the gauge applied afterwards

The bars the device is held to are the constants at the end; tests/test_model_fit_statement_cpu.py measures them again on every run,
DESIGN.md section 15 says where each came from."""
import numpy as np
from scipy.optimize import least_squares

import pose_statement as ps

OK, NOT_SEEN = 0, 5


# ---------------------------------------------------------------------------------------------------------------------
# observations
# ---------------------------------------------------------------------------------------------------------------------
def _index_model(model):
    """The same model list with corner c of every model at (c, 0, 0): correspondences() then returns corner ids as points."""
    n, P = len(model["ids"]), int(model["size"]) * 8
    idx = np.zeros((n, P, 3), np.float32)
    idx[:, :, 0] = np.arange(P, dtype=np.float32)
    return {"ids": model["ids"], "size": model["size"], "corners": idx}


def observations(recs, seed, camera, ok_of=None):
    """Rule 1.  One entry per marker of every CTAG_OK frame, in record order: dict(w, frame, marker, model, ids [n], obs [n, 2])
    for the records that take part, None for the others.  ok_of(w) -> bool says whether pose record w is CTAG_POSE_OK under the
    seed (None: whenever the builder gives at least 4 points, i.e. no degenerate EPnP).  A record with a repeated model position
    is left out."""
    K, dist = camera
    idx = _index_model(seed)
    out, w = [], 0
    for f, rec in enumerate(recs):
        for m in range(ps.marker_count(rec)):
            st, mi, n, obj, img = ps.expected_record(rec, m, idx)
            entry = None
            if st == ps.OK and (ok_of is None or ok_of(w)):
                ids = obj[:, 0].astype(np.int64)
                if len(set(ids.tolist())) == len(ids):
                    entry = {"w": w, "frame": f, "marker": m, "model": mi, "ids": ids, "obs": ps.observations(K, dist, img)}
            out.append(entry)
            w += 1
    return out


def seen_counts(obs, n_models, P):
    c = np.zeros((n_models, P), np.int64)
    for o in obs:
        if o is not None:
            c[o["model"], o["ids"]] += 1
    return c


def held_mask(obs, n_models, P, min_obs=2):
    """Rule 2: [n_models, P] bool."""
    return seen_counts(obs, n_models, P) < min_obs


# ---------------------------------------------------------------------------------------------------------------------
# residuals of many records at once, in any floating-point type
# ---------------------------------------------------------------------------------------------------------------------
def _rot(rv):
    """Rodrigues of rv [R, 3] -> [R, 3, 3], in rv's own type."""
    T = rv.dtype.type
    th2 = (rv * rv).sum(1)
    th = np.sqrt(th2)
    small = th < T(1e-12)
    ths = np.where(small, T(1), th)
    w = rv / ths[:, None]
    c, s = np.cos(ths), np.sin(ths)
    Wx = np.zeros((len(rv), 3, 3), rv.dtype)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    Rm = c[:, None, None] * np.eye(3, dtype=rv.dtype) + s[:, None, None] * Wx + (T(1) - c)[:, None, None] * (w[:, :, None] * w[:, None, :])
    Rm[small] = np.eye(3, dtype=rv.dtype)
    return Rm


class Batch:
    """The observation records of ONE model, padded to a common point count: ids [R, n], obs [R, n, 2], mask [R, n]."""

    def __init__(self, obs, model_index, camera, dtype=np.float64):
        self.recs = [o for o in obs if o is not None and o["model"] == model_index]
        self.fx, self.fy, self.cx, self.cy = (dtype(v) for v in ps._intrinsics(camera[0]))
        R, n = len(self.recs), max([len(o["ids"]) for o in self.recs] + [1])
        self.ids = np.zeros((R, n), np.int64)
        self.obs = np.zeros((R, n, 2), dtype)
        self.mask = np.zeros((R, n), bool)
        for r, o in enumerate(self.recs):
            k = len(o["ids"])
            self.ids[r, :k], self.obs[r, :k], self.mask[r, :k] = o["ids"], o["obs"], True
        self.dtype = dtype

    def residual_at(self, Xp, poses):
        """Xp [R, n, 3] points, poses [R, 6] -> residuals [R, n, 2] (0 where masked)."""
        P = np.einsum("rij,rnj->rni", _rot(poses[:, :3]), Xp) + poses[:, None, 3:]
        u = self.fx * P[..., 0] / P[..., 2] + self.cx - self.obs[..., 0]
        v = self.fy * P[..., 1] / P[..., 2] + self.cy - self.obs[..., 1]
        return np.stack([u, v], -1) * self.mask[..., None]

    def residual(self, X, poses):
        return self.residual_at(np.asarray(X, self.dtype)[self.ids], np.asarray(poses, self.dtype))

    def costs(self, X, poses):
        r = self.residual(X, poses)
        return 0.5 * (r * r).sum((1, 2))

    def jac_pose(self, X, poses, h):
        """[R, n, 2, 6] by central differences of step h (relative to max(1, |x|))."""
        poses = np.asarray(poses, self.dtype)
        J = np.zeros(self.mask.shape + (2, 6), self.dtype)
        for a in range(6):
            d = np.zeros_like(poses)
            d[:, a] = h * np.maximum(1, np.abs(poses[:, a]))
            J[..., a] = (self.residual(X, poses + d) - self.residual(X, poses - d)) / (2 * d[:, a])[:, None, None]
        return J

    def jac_point(self, X, poses, h):
        """[R, n, 2, 3]: d residual of a point / d its own model point."""
        Xp = np.asarray(X, self.dtype)[self.ids]
        poses = np.asarray(poses, self.dtype)
        J = np.zeros(self.mask.shape + (2, 3), self.dtype)
        for a in range(3):
            d = np.zeros_like(Xp)
            d[..., a] = h * np.maximum(1, np.abs(Xp[..., a]))
            J[..., a] = (self.residual_at(Xp + d, poses) - self.residual_at(Xp - d, poses)) / (2 * d[..., a])[..., None]
        return J


def step_of(dtype):
    """Central-difference step for a type: eps^(1/3)."""
    return dtype(np.finfo(dtype).eps) ** (dtype(1) / dtype(3))


def solve_poses(batch, X, poses0, iters=40):
    """Every record's pose at model X from poses0 [R, 6]: damped Gauss-Newton, numerical Jacobians; stops when no pose moves by
    more than 1e-13 relative."""
    poses = np.array(poses0, batch.dtype)
    h = step_of(batch.dtype)
    lam = np.full(len(poses), 1e-6)
    cost = batch.costs(X, poses)
    for _ in range(iters):
        J = batch.jac_pose(X, poses, h).reshape(len(poses), -1, 6)
        r = batch.residual(X, poses).reshape(len(poses), -1)
        H = np.einsum("rka,rkb->rab", J, J)
        g = np.einsum("rka,rk->ra", J, r)
        D = np.einsum("raa->ra", H)
        step = np.linalg.solve(H + lam[:, None, None] * (np.eye(6) * D[:, None, :]), -g[..., None])[..., 0]
        trial = poses + step
        c = batch.costs(X, trial)
        better = c < cost
        poses[better], cost[better] = trial[better], c[better]
        lam = np.where(better, lam / 10, lam * 10).clip(1e-12, 1e6)
        if (np.abs(step) <= 1e-13 * np.maximum(1, np.abs(poses))).all():
            break
    return poses


def _rvec_of(Rm):
    """Rotation vectors of rotation matrices [R, 3, 3] (angles below pi)."""
    c = np.clip((np.einsum("rii->r", Rm) - 1) / 2, -1, 1)
    th = np.arccos(c)
    ax = np.stack([Rm[:, 2, 1] - Rm[:, 1, 2], Rm[:, 0, 2] - Rm[:, 2, 0], Rm[:, 1, 0] - Rm[:, 0, 1]], 1)
    n = np.linalg.norm(ax, axis=1)
    return np.where(n[:, None] > 1e-12, ax / np.maximum(n, 1e-300)[:, None] * th[:, None], 0.0)


def best_poses(batch, X, *starts):
    """solve_poses from each of the given starts [R, 6]; the better minimum per record.  A small, nearly flat patch of a model
    has a mirrored pose that is a local minimum of its own, and a model that is off can make it the one a single start finds."""
    best = cost = None
    for p0 in starts:
        p = solve_poses(batch, X, p0)
        c = batch.costs(X, p)
        if best is None:
            best, cost = p, c
        else:
            better = c < cost
            best[better], cost[better] = p[better], c[better]
    return best


def moved_poses(sim, poses):
    """The poses of a model after the similarity X' = s R X + t has been applied to it: the camera sees the same image from
    (Rp R^T, s tp - Rp R^T t)."""
    sc, Rs, ts = sim
    Rp = _rot(np.asarray(poses, np.float64)[:, :3])
    Rn = np.einsum("rij,kj->rik", Rp, Rs)
    t = sc * np.asarray(poses, np.float64)[:, 3:] - np.einsum("rij,j->ri", Rn, ts)
    return np.concatenate([_rvec_of(Rn), t], 1)


# ---------------------------------------------------------------------------------------------------------------------
# the reduced system
# ---------------------------------------------------------------------------------------------------------------------
def reduced_system(batch, X, poses, P, reverse=False):
    """S [3P, 3P], g [3P] of one model at (X [P, 3], poses [R, 6]): sum over its records, in record order (reversed: the same sums
    the other way round), of (Q Jx)^T (Q Jx) and (Q Jx)^T r, Q = I - Jp (Jp^T Jp)^-1 Jp^T."""
    T = batch.dtype
    h = step_of(T)
    Jp = batch.jac_pose(X, poses, h)
    Jx = batch.jac_point(X, poses, h)
    res = batch.residual(X, poses)
    S, g = np.zeros((3 * P, 3 * P), T), np.zeros(3 * P, T)
    order = range(len(batch.recs) - 1, -1, -1) if reverse else range(len(batch.recs))
    for r in order:
        n = int(batch.mask[r].sum())
        A = Jp[r, :n].reshape(2 * n, 6)
        Jfull = np.zeros((2 * n, 3 * n), T)
        for i in range(n):
            Jfull[2 * i:2 * i + 2, 3 * i:3 * i + 3] = Jx[r, i]
        U = A.T @ A
        Q = np.eye(2 * n, dtype=T) - A @ _inv(U) @ A.T
        M = Q @ Jfull
        cols = (3 * batch.ids[r, :n, None] + np.arange(3)).ravel()
        S[np.ix_(cols, cols)] += M.T @ M
        g[cols] += M.T @ res[r, :n].reshape(2 * n)
    return S, g


def _inv(U):
    """Inverse of a small symmetric positive definite matrix in its own type (numpy.linalg has no long double)."""
    n = len(U)
    L = np.zeros_like(U)
    for j in range(n):
        L[j, j] = np.sqrt(U[j, j] - (L[j, :j] ** 2).sum())
        for i in range(j + 1, n):
            L[i, j] = (U[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    Li = np.zeros_like(U)
    for j in range(n):
        Li[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(L[i, j:i] * Li[j:i, j]).sum() / L[i, i]
    return Li.T @ Li


def step(S, g, held, lam):
    """(S + lambda diag S) delta = -g on the fitted corners, 0 on the held ones.  Returns (delta [3P], positive definite?)."""
    T = S.dtype.type
    free = np.repeat(~np.asarray(held, bool), 3)
    A = S[np.ix_(free, free)].copy()
    A[np.diag_indices_from(A)] += T(lam) * np.diag(A)
    d = np.zeros(len(g), S.dtype)
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):  # Cholesky in the matrix's own type
        piv = A[j, j] - (L[j, :j] ** 2).sum()
        if not piv > 0:
            return d, False
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, S.dtype)
    b = -g[free]
    for j in range(n):
        y[j] = (b[j] - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros(n, S.dtype)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    d[free] = x
    return d, True


# ---------------------------------------------------------------------------------------------------------------------
# gauge and scale
# ---------------------------------------------------------------------------------------------------------------------
def similarity(X, Y):
    """Umeyama: (s, R, t) minimising sum |Y - (s R X + t)|^2."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    mx, my = X.mean(0), Y.mean(0)
    C = (Y - my).T @ (X - mx)
    U, sv, Vt = np.linalg.svd(C)
    D = np.diag([1, 1, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    Rm = U @ D @ Vt
    s = (sv * np.diag(D)).sum() / ((X - mx) ** 2).sum()
    return s, Rm, my - s * Rm @ mx


def apply_similarity(sim, X):
    s, Rm, t = sim
    return s * np.asarray(X, np.float64) @ Rm.T + t


def gauge(X, seed, held):
    """Rule 5: the fitted corners of X carried onto the seed's by the best similarity; held corners are the seed's."""
    out = np.array(seed, np.float64)
    fit = ~np.asarray(held, bool)
    if fit.sum() >= 3:
        out[fit] = apply_similarity(similarity(np.asarray(X, np.float64)[fit], out[fit]), np.asarray(X, np.float64)[fit])
    return out


VERTICAL_EDGES = ((0, 5), (1, 4))


def metric_scale(X, held, strip_height):
    """Rule 6 -> (X scaled about the centroid of its fitted corners, factor, centroid); factor None when no feature has its four
    ends fitted."""
    X = np.array(X, np.float64)
    fit = ~np.asarray(held, bool)
    lengths = [np.linalg.norm(X[8 * f + a] - X[8 * f + b]) for f in range(len(X) // 8) if fit[[8 * f, 8 * f + 1, 8 * f + 4, 8 * f + 5]].all()
               for a, b in VERTICAL_EDGES]
    if not lengths:
        return X, None, None
    factor, c = strip_height / np.mean(lengths), X[fit].mean(0)
    X[fit] = c + factor * (X[fit] - c)
    return X, factor, c


# ---------------------------------------------------------------------------------------------------------------------
# the loop of rule 4 and the joint minimum
# ---------------------------------------------------------------------------------------------------------------------
def fit(batch, seed, held, poses0, max_rounds=30, lambda0=1e-3, lambda_max=1e6, rel_tol=1e-6, round_float=True, wrong=None):
    """Rule 4 for one model: returns dict(X, poses, cost0, cost, rounds, lam).  wrong="free gauge": a planted error for the
    statement's own tests, rule 5 skipped."""
    P = len(seed)
    seed = np.asarray(seed, np.float64)
    X = seed.copy()
    poses = solve_poses(batch, X, poses0)
    cost = cost0 = float(batch.costs(X, poses).sum())
    lam, rounds = lambda0, 0
    while rounds < max_rounds:
        rounds += 1
        S, g = reduced_system(batch, X, poses, P)
        d, pd = step(S, g, held, lam)
        good = False
        if pd:
            T = X + d.reshape(P, 3)
            if wrong != "free gauge":
                T = gauge(T, seed, held)
            if round_float:
                T = T.astype(np.float32).astype(np.float64)
            tp = best_poses(batch, T, poses, poses0)   # the previous round's and the first start: the better per record
            c = float(batch.costs(T, tp).sum())
            good = c < cost
        if good:
            drop, cost, X, poses = cost - c, c, T, tp
            lam = max(lam / 3, 1e-9)
            if drop < rel_tol * cost:
                break
        else:
            lam *= 4
            if lam > lambda_max:
                break
    return {"X": X, "poses": poses, "cost0": cost0, "cost": cost, "rounds": rounds, "lam": lam}


def joint_minimum(batch, X0, seed, held, poses0):
    """The minimum over the fitted corners AND the poses together by scipy.optimize.least_squares from (X0, poses0), the gauge applied
    afterwards.  Held corners are the seed's throughout.  Returns dict(X, poses, cost)."""
    seed = np.asarray(seed, np.float64)
    fit_ = ~np.asarray(held, bool)
    nf, R = int(fit_.sum()), len(batch.recs)

    def unpack(v):
        X = seed.copy()
        X[fit_] = v[:3 * nf].reshape(nf, 3)
        return X, v[3 * nf:].reshape(R, 6)

    def fun(v):
        X, poses = unpack(v)
        return batch.residual(X, poses)[batch.mask].ravel()

    # the Jacobian from the same central differences as the reduced system: a residual depends on its own point (if fitted) and
    # on its own record's pose
    col_of = -np.ones(len(seed), np.int64)
    col_of[fit_] = np.arange(nf)
    rr, nn = np.nonzero(batch.mask)
    pc = col_of[batch.ids[rr, nn]]
    h = step_of(np.float64)

    def jac(v):
        X, poses = unpack(v)
        Jp, Jx = batch.jac_pose(X, poses, h)[rr, nn], batch.jac_point(X, poses, h)[rr, nn]  # [k, 2, 6], [k, 2, 3]
        J = np.zeros((len(rr), 2, 3 * nf + 6 * R))
        k = np.arange(len(rr))
        for a in range(6):
            J[k, :, 3 * nf + 6 * rr + a] = Jp[:, :, a]
        on = pc >= 0
        for a in range(3):
            J[k[on], :, 3 * pc[on] + a] = Jx[on][:, :, a]
        return J.reshape(2 * len(rr), -1)

    poses0 = solve_poses(batch, X0, poses0)
    v0 = np.concatenate([np.asarray(X0, np.float64)[fit_].ravel(), np.asarray(poses0, np.float64).ravel()])
    sol = least_squares(fun, v0, jac=jac, method="trf", tr_solver="exact", xtol=1e-12, ftol=1e-13, gtol=1e-12, x_scale=1.0, max_nfev=40)  # xtol: 5e-10 mm of 500
    X, poses = unpack(sol.x)
    Xg = gauge(X, seed, held)
    pg = solve_poses(batch, Xg, poses)  # the similarity moved the frame: the poses follow
    return {"X": Xg, "poses": pg, "cost": float(batch.costs(Xg, pg).sum())}


# ---------------------------------------------------------------------------------------------------------------------
# comparisons and the measured bars (DESIGN.md section 15 holds the figures and where each came from)
# ---------------------------------------------------------------------------------------------------------------------
def system_deviation(S, g, d, S_ref, g_ref, d_ref, held, cost):
    """Scale-free deviations of (S, g, delta) from a reference: S entries over sqrt(S_ii S_jj), g entries over sqrt(S_ii) * |r|
    (the Cauchy-Schwarz bound of an entry of (Q Jx)^T r), delta over its largest entry; over the fitted corners for S and delta."""
    S_ref, g_ref, d_ref = (np.asarray(a, np.float64) for a in (S_ref, g_ref, d_ref))
    dg = np.sqrt(np.abs(np.diag(S_ref)))
    seen = dg > 0
    sc = np.outer(dg[seen], dg[seen])
    dS = float(np.abs((np.asarray(S, np.float64) - S_ref)[np.ix_(seen, seen)] / sc).max())
    rn = np.sqrt(2 * max(cost, 1e-300))
    dgv = float(np.abs((np.asarray(g, np.float64) - g_ref)[seen] / (dg[seen] * rn)).max())
    dd = float(np.abs(np.asarray(d, np.float64) - d_ref).max() / max(np.abs(d_ref).max(), 1e-300))
    return dS, dgv, dd


def check_result(X, seed, held, minimum_X, what=""):
    """What a returned model must be (rules 2, 5 and the minimum): held corners bit-equal to the seed's float32; the fitted corners
    in the seed's gauge -- the best similarity onto the seed's is the identity to within the bar; and within CORNER_BAR_MM of the
    joint minimum.  Returns the largest distance to the minimum, mm."""
    X32, seed32 = np.asarray(X, np.float32), np.asarray(seed, np.float32)
    held = np.asarray(held, bool)
    assert X32[held].tobytes() == seed32[held].tobytes(), (what, "held corners moved")
    fit_ = ~held
    if not fit_.any():
        return 0.0
    Xf, Sf = X32[fit_].astype(np.float64), seed32[fit_].astype(np.float64)
    drift = float(np.abs(apply_similarity(similarity(Xf, Sf), Xf) - Xf).max())
    assert drift <= CORNER_BAR_MM, (what, "not in the seed's gauge", drift)
    dist = float(np.abs(Xf - np.asarray(minimum_X, np.float64)[fit_]).max())
    assert dist <= CORNER_BAR_MM, (what, "away from the joint minimum", dist)
    return dist


# The float64 statement against the same computation in numpy.longdouble, worst over the shapes batches, AS MEASURED (three digits);
# tests/test_model_fit_statement_cpu.py::test_measured_bars measures them again on every run and fails when a figure here is off by
# more than 2 %.  The device is allowed 16 x these.  (Summation order reversed: 9e-16, 1e-16, 1e-13.)
SYSTEM_ERR = {"S": 1.21e-8, "g": 7.67e-10, "delta": 1.25e-7}
SYSTEM_BAR = {k: 16 * v for k, v in SYSTEM_ERR.items()}
F32_SPACING_MM = 500.0 * 2.0 ** -23   # float32 spacing of a coordinate near 500 mm
CORNER_ERR_MM = F32_SPACING_MM        # the larger of the spacing and the distance between two statement minima (measured: 1e-9 mm)
CORNER_BAR_MM = 16 * CORNER_ERR_MM
REL_TOL_F32 = 6.04e-8                 # relative cost change float32 rounding of the model alone causes (0.1 px batches), as measured
