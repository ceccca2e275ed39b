"""An independent statement of the intrinsics fit (include/ctag_pose.h, intrinsics fit, rules 1-8), in numpy / scipy only.  Nothing
here comes from oracle/, cylindertag_amd/csrc or testkit; the membership of a rig in a frame is mv_statement's.  What is stated:

  Views              rule 1: the observation records, all their points in one flat list (model point, pixel as detected, record)
  residual           rule 2: the forward model of cv::projectPoints without tilt, in any floating-point type
  jacobians          its analytic derivatives in the view pose (rvec, tvec) and in the sixteen camera parameters
  solve_poses        rule 4's minimum: every record's pose given the camera, Gauss-Newton from a start
  reduced_system     rule 5: S = sum Jc^T Jc - Z^T Z, g = sum Jc^T r - Z^T y per record, in record order
  step               (S + lambda diag S) delta = -g over the free rows
  fit                the Levenberg-Marquardt loop of rule 5, with rule 3's float32 camera (round_float)
  joint_minimum      scipy.optimize.least_squares over the camera AND all view poses together
  sigma              rule 6

A camera is its parameter vector p[16] = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (PARAMS); a mask is an int, bit i = parameter
i is free; tie is None or the ratio fy / fx that stays.  The bars the device is held to are the constants at the end;
tests/test_intr_fit_statement_cpu.py measures them again on every run, DESIGN.md section 18 says where each came from."""
import numpy as np
from scipy import sparse
from scipy.optimize import least_squares

import mv_statement as mv

PARAMS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "s1", "s2", "s3", "s4")
N = 16
OK, TOO_FEW, DEGENERATE, NOT_SEEN = 0, 2, 4, 5
TILE = 64


def camera_vector(K, dist, T=np.float64):
    """p[16] of a 3 x 3 matrix and a coefficient list (float32 values, as the calls read them)."""
    K = np.asarray(K, np.float32).reshape(3, 3).astype(T)
    p = np.zeros(N, T)
    p[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    d = np.asarray(dist, np.float32).ravel()[:12].astype(T)
    p[4:4 + len(d)] = d
    return p


def camera_of(p, K, n_dist):
    """(K, dist) float32 of a parameter vector: K's other entries are kept."""
    K = np.array(K, np.float32).reshape(3, 3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = p[:4]
    return K, np.asarray(p[4:4 + min(n_dist, 12)], np.float32)


def default_mask(n_dist):
    return (1 << (4 + min(n_dist, 12))) - 1


def free_rows(mask, tie=None):
    return [i for i in range(N) if (mask >> i) & 1 and not (tie is not None and i == 1)]


def round_camera(p, n_dist):
    """Rule 3: the doubles rounded to the camera's floats; coefficients at or beyond n_dist stay zero."""
    q = np.asarray(p, np.float64).astype(np.float32).astype(np.float64)
    q[4 + min(n_dist, 12):] = 0.0
    return q


def usable_camera(p):
    return bool(np.isfinite(p).all() and p[0] > 0 and p[1] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# Rodrigues' formula and its derivative, in any type
# ---------------------------------------------------------------------------------------------------------------------
def _hat(v, T):
    K = np.zeros(v.shape[:-1] + (3, 3), T)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 2], v[..., 1], v[..., 2], -v[..., 0], -v[..., 1], v[..., 0]
    return K


def rot_many(rv, T=np.float64):
    """[m, 3] rotation vectors -> [m, 3, 3]."""
    rv = np.asarray(rv, T).reshape(-1, 3)
    th = np.sqrt((rv * rv).sum(1))
    small = th < T(1e-10)
    ths = np.where(small, T(1), th)
    a = np.where(small, T(1), np.sin(ths) / ths)
    b = np.where(small, T(0.5), T(2) * np.sin(ths / 2) ** 2 / (ths * ths))
    K = _hat(rv, T)
    return np.eye(3, dtype=T) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def drot_many(rv, T=np.float64):
    """[m, 3] -> [m, 3(k), 3, 3]: d R / d rv_k = (rv_k [rv]x + [rv x (I - R) e_k]x) R / |rv|^2  (Gallego, Yezzi 2015); [e_k]x at 0."""
    rv = np.asarray(rv, T).reshape(-1, 3)
    R = rot_many(rv, T)
    th2 = (rv * rv).sum(1)
    small = th2 < T(1e-20)
    th2s = np.where(small, T(1), th2)
    out = np.zeros((len(rv), 3, 3, 3), T)
    Kx = _hat(rv, T)
    I = np.eye(3, dtype=T)
    for k in range(3):
        w = np.cross(rv, (I - R)[:, :, k])
        out[:, k] = (rv[:, k, None, None] * Kx + _hat(w, T)) @ R / th2s[:, None, None]
        out[small, k] = _hat(I[k], T)
    return out


def rotvec(R):
    return mv.rotvec(R)


# ---------------------------------------------------------------------------------------------------------------------
# rule 1
# ---------------------------------------------------------------------------------------------------------------------
class Views:
    """The observation records of a call: every item f * n_rigs + g in which rig g has members and at least max(4, min_points) points,
    and ok_of(item) if given (the device's seed record is CTAG_POSE_OK).  All points in one flat list, marker order then the builder's."""

    def __init__(self, records, model, rig_of_model, n_rigs, min_points=8, ok_of=None):
        self.items, self.n_points = [], []
        X, uv, rec = [], [], []
        for f, r in enumerate(records):
            if int(r["status"]) != 0:
                continue
            for g in range(n_rigs):
                (members, obj, img), = mv.membership([r], model, rig_of_model, g)[0]
                item = f * n_rigs + g
                if not members or len(obj) < max(4, min_points) or (ok_of is not None and not ok_of(item)):
                    continue
                X.append(np.asarray(obj, np.float32).astype(np.float64))
                uv.append(np.asarray(img, np.float32).astype(np.float64))
                rec.append(np.full(len(obj), len(self.items)))
                self.items.append(item)
                self.n_points.append(len(obj))
        self.R = len(self.items)
        self.X = np.concatenate(X) if X else np.zeros((0, 3))
        self.uv = np.concatenate(uv) if uv else np.zeros((0, 2))
        self.rec = np.concatenate(rec).astype(np.int64) if rec else np.zeros(0, np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.n_points)]).astype(np.int64)

    def with_pixels(self, uv):
        """The same views with other pixels (the float32 rounding study)."""
        import copy
        V = copy.copy(self)
        V.uv = np.asarray(uv, np.float64)
        return V


# ---------------------------------------------------------------------------------------------------------------------
# rule 2 and its derivatives
# ---------------------------------------------------------------------------------------------------------------------
def _distort(p, a, b, wrong=None):
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = p[4:]
    if wrong == "p1 p2 swapped":
        p1, p2 = p2, p1
    r2 = a * a + b * b
    r4, r6 = r2 * r2, r2 * r2 * r2
    num = 1 + k1 * r2 + k2 * r4 + k3 * r6
    den = 1 + k4 * r2 + k5 * r4 + k6 * r6
    rad = num / den
    xd = a * rad + 2 * p1 * a * b + p2 * (r2 + 2 * a * a) + s1 * r2 + s2 * r4
    yd = b * rad + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b + s3 * r2 + s4 * r4
    return r2, r4, r6, num, den, rad, xd, yd


def residual(V, p, poses, T=np.float64, wrong=None):
    """[n, 2] and the mask of unusable points (Z <= 0, denominator <= 0, not finite)."""
    p, poses = np.asarray(p, T), np.asarray(poses, T).reshape(-1, 6)
    Rm = rot_many(poses[:, :3], T)
    P = np.einsum("nij,nj->ni", Rm[V.rec], V.X.astype(T)) + poses[V.rec, 3:]
    with np.errstate(all="ignore"):
        a, b = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        r2, r4, r6, num, den, rad, xd, yd = _distort(p, a, b, wrong)
        r = np.stack([p[0] * xd + p[2] - V.uv[:, 0].astype(T), p[1] * yd + p[3] - V.uv[:, 1].astype(T)], 1)
    bad = ~(P[:, 2] > 0) | ~(den > 0) | ~np.isfinite(r).all(1)
    return r, bad


def record_costs(V, p, poses, T=np.float64):
    r, bad = residual(V, p, poses, T)
    c = 0.5 * np.bincount(V.rec, (r * r).sum(1).astype(np.float64), V.R)
    return c, not bad.any()


def total_cost(costs):
    """Rule 2: the record costs summed in record order."""
    s = 0.0
    for c in costs:
        s += float(c)
    return s


def jacobians(V, p, poses, T=np.float64, tie=None, wrong=None):
    """(r [n, 2], Jp [n, 2, 6], Jc [n, 2, 16]) analytically; with tie the fx column carries tie x the fy column."""
    p, poses = np.asarray(p, T), np.asarray(poses, T).reshape(-1, 6)
    fx, fy = p[0], p[1]
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = p[4:]
    Rm, dRm = rot_many(poses[:, :3], T), drot_many(poses[:, :3], T)
    X = V.X.astype(T)
    P = np.einsum("nij,nj->ni", Rm[V.rec], X) + poses[V.rec, 3:]
    iz = 1 / P[:, 2]
    a, b = P[:, 0] * iz, P[:, 1] * iz
    r2, r4, r6, num, den, rad, xd, yd = _distort(p, a, b)
    r = np.stack([fx * xd + p[2] - V.uv[:, 0].astype(T), fy * yd + p[3] - V.uv[:, 1].astype(T)], 1)
    drad = ((k1 + 2 * k2 * r2 + 3 * k3 * r4) * den - num * (k4 + 2 * k5 * r2 + 3 * k6 * r4)) / (den * den)
    dxa = rad + 2 * a * a * drad + 2 * p1 * b + 6 * p2 * a + 2 * s1 * a + 4 * s2 * r2 * a
    dxb = 2 * a * b * drad + 2 * p1 * a + 2 * p2 * b + 2 * s1 * b + 4 * s2 * r2 * b
    dya = 2 * a * b * drad + 2 * p1 * a + 2 * p2 * b + 2 * s3 * a + 4 * s4 * r2 * a
    dyb = rad + 2 * b * b * drad + 6 * p1 * b + 2 * p2 * a + 2 * s3 * b + 4 * s4 * r2 * b
    n = len(X)
    dP = np.zeros((n, 2, 3), T)   # d residual / d P
    dP[:, 0] = np.stack([fx * dxa * iz, fx * dxb * iz, -fx * (dxa * a + dxb * b) * iz], 1)
    dP[:, 1] = np.stack([fy * dya * iz, fy * dyb * iz, -fy * (dya * a + dyb * b) * iz], 1)
    Jp = np.zeros((n, 2, 6), T)
    for k in range(3):
        Jp[:, :, k] = np.einsum("nci,ni->nc", dP, np.einsum("nij,nj->ni", dRm[V.rec, k], X))
    Jp[:, :, 3:] = dP
    Jc = np.zeros((n, 2, N), T)
    z, o = np.zeros(n, T), np.ones(n, T)
    cols = {0: (xd, z), 1: (z, yd), 2: (o, z), 3: (z, o),
            4: (fx * a * r2 / den, fy * b * r2 / den), 5: (fx * a * r4 / den, fy * b * r4 / den), 8: (fx * a * r6 / den, fy * b * r6 / den),
            9: (-fx * a * rad * r2 / den, -fy * b * rad * r2 / den), 10: (-fx * a * rad * r4 / den, -fy * b * rad * r4 / den),
            11: (-fx * a * rad * r6 / den, -fy * b * rad * r6 / den),
            6: (fx * 2 * a * b, fy * (r2 + 2 * b * b)), 7: (fx * (r2 + 2 * a * a), fy * 2 * a * b),
            12: (fx * r2, z), 13: (fx * r4, z), 14: (z, fy * r2), 15: (z, fy * r4)}
    if wrong == "p1 p2 swapped":
        cols[6], cols[7] = cols[7], cols[6]
    for i, (c0, c1) in cols.items():
        Jc[:, 0, i], Jc[:, 1, i] = c0, c1
    if tie is not None and wrong != "tied fy missing":
        Jc[:, :, 0] = Jc[:, :, 0] + T(tie) * Jc[:, :, 1]
    return r, Jp, Jc


def numeric_jacobians(V, p, poses, h=1e-6):
    """Central differences of residual(): the check of jacobians()."""
    p, poses = np.asarray(p, np.float64), np.asarray(poses, np.float64).reshape(-1, 6)
    Jp = np.zeros((len(V.X), 2, 6))
    Jc = np.zeros((len(V.X), 2, N))
    for a in range(6):
        s = h * (100.0 if a >= 3 else 1.0)
        d = np.zeros(6)
        d[a] = s
        Jp[:, :, a] = (residual(V, p, poses + d)[0] - residual(V, p, poses - d)[0]) / (2 * s)
    for i in range(N):
        s = h * max(1.0, abs(p[i]))
        d = np.zeros(N)
        d[i] = s
        Jc[:, :, i] = (residual(V, p + d, poses)[0] - residual(V, p - d, poses)[0]) / (2 * s)
    return Jp, Jc


# ---------------------------------------------------------------------------------------------------------------------
# rule 4
# ---------------------------------------------------------------------------------------------------------------------
def solve_poses(V, p, poses0, iters=40):
    """Every record's pose under camera p: Gauss-Newton from poses0 (float64), the step halved while the record's cost rises."""
    poses = np.array(poses0, np.float64).reshape(-1, 6)
    cost = record_costs(V, p, poses)[0]
    for _ in range(iters):
        r, Jp, _ = jacobians(V, p, poses)
        H = np.zeros((V.R, 6, 6))
        b = np.zeros((V.R, 6))
        np.add.at(H, V.rec, np.einsum("nka,nkb->nab", Jp, Jp))
        np.add.at(b, V.rec, np.einsum("nka,nk->na", Jp, r))
        d = np.linalg.solve(H, -b[..., None])[..., 0]
        for _ in range(20):
            c, _ = record_costs(V, p, poses + d)
            worse = ~(c <= cost)
            if not worse.any():
                break
            d[worse] *= 0.5
        poses = poses + d
        cost = record_costs(V, p, poses)[0]
        if np.abs(d).max() < 1e-13 * max(1.0, np.abs(poses).max()):
            break
    return poses


# ---------------------------------------------------------------------------------------------------------------------
# rule 5
# ---------------------------------------------------------------------------------------------------------------------
def _solve_spd(A, B):
    """A^-1 B for a symmetric positive definite A by Cholesky, in A's type.  Returns (X, positive definite?)."""
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


def reduced_system(V, p, poses, tie=None, T=np.float64, wrong=None):
    """S [16, 16], g [16] over ALL sixteen parameters at (p, poses): the sums over the records, in record order, of rule 5's S_r, g_r.
    wrong: planted errors for the statement's own tests."""
    r, Jp, Jc = jacobians(V, p, poses, T, tie, wrong)
    S, g = np.zeros((N, N), T), np.zeros(N, T)
    for k in range(V.R):
        idx = np.arange(V.start[k], V.start[k + 1])
        if wrong == "a tile one point short":
            idx = idx[(idx - V.start[k]) % TILE != TILE - 1]
        A = Jp[idx].reshape(-1, 6)
        B = Jc[idx].reshape(-1, N)
        q = r[idx].reshape(-1)
        U, W = A.T @ A, A.T @ B
        X, pd = _solve_spd(U, np.concatenate([W, (A.T @ q)[:, None]], 1))
        assert pd
        ZtZ, Zty = W.T @ X[:, :N], W.T @ X[:, N]
        if wrong == "ZtZ added":
            S += B.T @ B + ZtZ
        else:
            S += B.T @ B - ZtZ
        g += B.T @ q - Zty
    return S, g


def step(S, g, mask, lam, tie=None, wrong=None):
    """(S + lambda diag S) delta = -g over the free rows (0 elsewhere).  Returns (delta, positive definite?)."""
    T = S.dtype.type
    rows = free_rows(mask, tie)
    A = S[np.ix_(rows, rows)].copy()
    if wrong == "damping on S":
        A = A + T(lam) * A
    else:
        A[np.diag_indices_from(A)] += T(lam) * np.diag(A)
    d, pd = _solve_spd(A, -g[rows])
    out = np.zeros(N, T)
    if pd:
        out[rows] = d
    return out, pd


def sigma(S, mask, cost, n_points, n_records, tie=None, wrong=None):
    """Rule 6: (sigma [16], sigma2_hat) from the undamped S at the returned state."""
    rows = free_rows(mask, tie)
    s2 = 2.0 * cost / (2 * n_points - 6 * n_records - len(rows))
    A = np.asarray(S, np.float64)[np.ix_(rows, rows)]
    inv, pd = _solve_spd(A, np.eye(len(rows)))
    assert pd
    out = np.zeros(N)
    out[rows] = np.sqrt((1.0 if wrong == "sigma without sigma2_hat" else s2) * np.diag(inv))
    if tie is not None:
        out[1] = tie * out[0]
    return out, s2


def system_deviation(S, g, d, S_ref, g_ref, d_ref, cost, rows):
    """Scaled deviations over the free rows: S entries over sqrt(S_ii S_jj), g entries over sqrt(S_ii) |r| (|r| = sqrt(2 cost)), delta
    entries over the parameter's own scale sqrt(1 / S_ii) |r| ... taken relative to the largest |delta_i| sqrt(S_ii)."""
    S_ref, g_ref, d_ref = (np.asarray(v, np.longdouble) for v in (S_ref, g_ref, d_ref))
    ix = np.ix_(rows, rows)
    sd = np.sqrt(np.diag(S_ref)[rows])
    eS = float((np.abs(np.asarray(S, np.longdouble)[ix] - S_ref[ix]) / np.outer(sd, sd)).max())
    eg = float((np.abs(np.asarray(g, np.longdouble)[rows] - g_ref[rows]) / (sd * max(np.sqrt(2 * cost), 1e-300))).max())
    scale = float((np.abs(d_ref[rows]) * sd).max())
    ed = float((np.abs(np.asarray(d, np.longdouble)[rows] - d_ref[rows]) * sd).max() / max(scale, 1e-300))
    return eS, eg, ed


# ---------------------------------------------------------------------------------------------------------------------
# the loop of rule 5 and the joint minimum
# ---------------------------------------------------------------------------------------------------------------------
def apply_step(p, d, mask, tie, n_dist, round_float):
    q = np.array(p, np.float64)
    rows = free_rows(mask, tie)
    q[rows] += np.asarray(d, np.float64)[rows]
    if tie is not None:
        q[1] = q[0] * tie
    return round_camera(q, n_dist) if round_float else q


def fit(V, p0, n_dist, mask, tie, poses0, max_rounds=30, lambda0=1e-3, lambda_max=1e6, rel_tol=1e-12, round_float=True, wrong=None):
    """Rule 5 from the seed p0: dict(p, poses, cost0, cost, rounds, lam, S).  wrong: a planted error of reduced_system / step."""
    p = round_camera(p0, n_dist) if round_float else np.array(p0, np.float64)
    poses = solve_poses(V, p, poses0)
    cost = cost0 = total_cost(record_costs(V, p, poses)[0])
    lam, rounds = lambda0, 0
    while rounds < max_rounds:
        rounds += 1
        S, g = reduced_system(V, p, poses, tie, wrong=wrong)
        d, pd = step(S, g, mask, lam, tie, wrong)
        good = False
        if pd:
            pt = apply_step(p, d, mask, tie, n_dist, round_float)
            if usable_camera(pt):
                tp = solve_poses(V, pt, poses)
                cs, ok = record_costs(V, pt, tp)
                c = total_cost(cs)
                good = ok and c < cost
        if good:
            drop, cost, p, poses = cost - c, c, pt, tp
            lam = max(lam / 3, 1e-9)
            if drop < rel_tol * cost:
                break
        else:
            lam *= 4
            if lam > lambda_max:
                break
    return {"p": p, "poses": poses, "cost0": cost0, "cost": cost, "rounds": rounds, "lam": lam, "S": reduced_system(V, p, poses, tie)[0]}


def joint_minimum(V, p0, mask, tie, poses0):
    """The minimum over the free camera parameters AND all view poses together by scipy.optimize.least_squares from (p0, poses0).
    Returns dict(p, poses, cost)."""
    p0 = np.array(p0, np.float64)
    rows = free_rows(mask, tie)
    nf, R, n = len(rows), V.R, len(V.X)

    def unpack(v):
        p = p0.copy()
        p[rows] = v[:nf]
        if tie is not None:
            p[1] = p[0] * tie
        return p, v[nf:].reshape(R, 6)

    def fun(v):
        p, poses = unpack(v)
        return residual(V, p, poses)[0].ravel()

    prow = np.broadcast_to(2 * np.arange(n)[:, None, None] + np.arange(2)[None, :, None], (n, 2, 6))
    pcol = np.broadcast_to(nf + 6 * V.rec[:, None, None] + np.arange(6)[None, None, :], (n, 2, 6))
    crow = np.broadcast_to(2 * np.arange(n)[:, None, None] + np.arange(2)[None, :, None], (n, 2, nf))
    ccol = np.broadcast_to(np.arange(nf)[None, None, :], (n, 2, nf))

    def jac(v):
        p, poses = unpack(v)
        _, Jp, Jc = jacobians(V, p, poses, tie=tie)
        J = sparse.coo_matrix((np.concatenate([Jc[:, :, rows].ravel(), Jp.ravel()]),
                               (np.concatenate([crow.ravel(), prow.ravel()]), np.concatenate([ccol.ravel(), pcol.ravel()]))), shape=(2 * n, nf + 6 * R)).tocsr()
        return J if R > 100 else J.toarray()

    poses0 = solve_poses(V, p0, poses0)
    v = np.concatenate([p0[rows], poses0.ravel()])
    for _ in range(3):   # restarted so that x_scale follows the Jacobian at the current point
        sol = least_squares(fun, v, jac=jac, method="trf", tr_solver="lsmr" if R > 100 else "exact", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=100)
        v = sol.x
    p, poses = unpack(v)
    # the last digits: Gauss-Newton on the reduced system at scipy's answer, in double
    for _ in range(3):
        poses = solve_poses(V, p, poses)
        S, g = reduced_system(V, p, poses, tie)
        d, pd = step(S, g, mask, 0.0, tie)
        if not pd:
            break
        pt = apply_step(p, d, mask, tie, 12, False)
        tp = solve_poses(V, pt, poses)
        if total_cost(record_costs(V, pt, tp)[0]) <= total_cost(record_costs(V, p, poses)[0]):
            p, poses = pt, tp
    return {"p": p, "poses": poses, "cost": total_cost(record_costs(V, p, poses)[0])}


def half_spacing(p):
    """Half the float32 spacing at each parameter's value."""
    return 0.5 * np.spacing(np.abs(np.asarray(p, np.float64)).astype(np.float32)).astype(np.float64)


def camera_bar(p, noise_free):
    """Per parameter: 16 x the largest of half the float32 spacing at its value, the distance between two joint minima from different
    starts and, for a noise-free case, the move float32 rounding of the pixels causes in the joint minimum (absolute figures per
    parameter, as measured below)."""
    m = np.maximum(half_spacing(p), MINIMA_DISTANCE)
    if noise_free:
        m = np.maximum(m, F32_PIXEL_MOVE)
    return 16.0 * m


# The float64 statement against the same computation in numpy.longdouble at the planted camera with every record's pose at its
# minimum, worst over the shapes and masks of tests/intr_fit_shapes.py, AS MEASURED (three digits); tests/test_intr_fit_statement_cpu.py::
# test_measured_bars measures them again on every run and fails when a figure here is off by more than 2 %.  The device is allowed 16 x.
SYSTEM_ERR = {"S": 1.03e-09, "g": 1.58e-10, "delta": 4.24e-09, "sigma": 7.69e-10, "pose": 1.17e-09}
SYSTEM_BAR = {k: 16 * v for k, v in SYSTEM_ERR.items()}
# (sigma is taken over the shapes that are fitted end to end, a-e, the ones the device's sigmas are held to: c12, the system probe's
# shape with all sixteen parameters free on 27 records, has an S conditioned accordingly -- 8.64e-4 there -- and is never fitted.)
# per parameter (PARAMS order), worst over the shapes held to the joint minimum (a-e; k4 .. s4 are free in none of them): the distance between two statement joint minima from different starts, and the move
# float32 rounding of the pixel coordinates alone causes in the joint minimum of the noise-free shapes
MINIMA_DISTANCE = np.array([1.62e-06, 1.89e-06, 7.69e-06, 1.23e-05, 5.77e-10, 9.08e-09, 2.04e-11, 3.16e-12, 9.97e-08, 0, 0, 0, 0, 0, 0, 0])
F32_PIXEL_MOVE = np.array([0.00443, 0.00441, 0.00402, 0.000717, 2.11e-06, 4.04e-05, 3.59e-08, 8.69e-09, 0.000933, 0, 0, 0, 0, 0, 0, 0])
# the relative change of the cost when one field of the returned camera of a 0.1 px case moves by one float32 ulp and the view poses are
# solved again, worst over the cases and fields, as tools/intr_fit_rate.py measures it on the device (it needs the device's view poses, so
# no CPU test can measure it again); the default rel_tol is 4 x
REL_TOL_ULP = 1.928e-9
