"""The track smoother of include/ctag_pose.h (track smoothing, rules 1-8) stated independently in numpy / scipy, in float64 and in
longdouble.  Nothing here comes from csrc, oracle or testkit.  The formulation differs from the kernels' on purpose: every term is a
residual with a dense 12-column Jacobian and an information matrix, the Gauss-Newton matrix is the sum of J^T M J, the system is solved
as one block-tridiagonal chain over the whole piece (or densely, for short pieces), and the marginals come from the plain inverse (short
pieces) or from the chain's backward recursion (long ones).  The kernels cut a piece into segments; this file never does.

A batch is a dict (tests/track_shapes.py): n_frames, n_rigs, times (array or None), opts (dict of ctag_track_opts fields), pose_status,
rvec, tvec [n_frames, n_rigs, ...], cov_status, cov_param, cov [n_frames, n_rigs, 6, 6], rec_rig, rec_frame (the records' own fields).

Bars.  MEASURED_F64_DEVIATION is the worst deviation between this statement in float64 and in longdouble over every batch of
track_shapes.BATCHES, per field, in the units in which cov_statement.py scales: poses and velocities in units of their own sigma
(sqrt of the diagonal of the longdouble result's cov / vel_sigma), cov entries over sqrt(cov_ii cov_jj), vel_sigma, mahalanobis2
(over 1 + its value), weights and costs relative.  tests/test_track_statement_cpu.py measures it again (test_f64_deviation) and prints
it; the figures below are that test's output.  BAR = 16 x the figure: the kernels run the same float64 arithmetic in another order (a
segmented elimination instead of one chain), and a different order of n roundings moves the result by up to a small multiple of what the
float64 run itself is off the longdouble one; 16 is the allowance cov_statement.py gives for the same reason."""
import numpy as np

OK, NOT_TRACKED, BAD_INPUT, SINGULAR = 0, 1, 2, 3
LOSS_HUBER, LOSS_CAUCHY, LOSS_NONE = 0, 1, 2
FLAG_MEASURED, FLAG_DOWNWEIGHTED = 1, 2
REL_TOL, LAMBDA_MAX = 1e-12, 1e6
DENSE_MAX_FRAMES = 24  # pieces up to this length: the dense route; longer: the chain

DEFAULTS = dict(loss=LOSS_NONE, max_iterations=10, max_gap=5, segment_frames=0, dt=1.0 / 30.0, q_rot=0.1, q_trans=3000.0, vel0_sigma_rot=10.0,
                vel0_sigma_trans=1000.0, loss_scale=4.0, lambda0=1e-3)

# measured by tests/test_track_statement_cpu.py::test_f64_deviation (python -m pytest -s tests/test_track_statement_cpu.py -k deviation), which
# prints both dicts.  _STEP: one undamped Gauss-Newton step (max_iterations = 1, lambda0 = 0) on every batch, `long` included; the other
# one: that and the full loop on every batch but `long` (8200 frames in longdouble once is what the test can afford).  The loop's figure is
# three orders above the step's because the loop's last rounds are decided by cost differences at the rounding of the cost: the float64
# and the longdouble run stop a few rounds apart (61 against 56 rounds over the eleven pieces of `lengths`).
MEASURED_F64_DEVIATION_STEP = {"pose": 1.05e-9, "vel": 1.18e-10, "cov": 1.06e-11, "vel_sigma": 1.70e-12, "mahalanobis2": 8.88e-11, "weight": 3.46e-14,
                               "cost": 8.23e-14}
MEASURED_F64_DEVIATION = {"pose": 1.98e-7, "vel": 1.54e-7, "cov": 2.47e-11, "vel_sigma": 1.70e-12, "mahalanobis2": 2.35e-8, "weight": 3.46e-14,
                          "cost": 8.23e-14}
BAR_STEP = {k: 16.0 * v for k, v in MEASURED_F64_DEVIATION_STEP.items()}  # what the single step is held to: never above BAR
BAR = {k: 16.0 * v for k, v in MEASURED_F64_DEVIATION.items()}
# The distance, in units of the smoothed cov (pose) and of vel_sigma (velocities), between this statement's own LM result and scipy's
# minimum over track_shapes.SCIPY_BATCHES (test_track_statement_cpu.py::test_lm_reaches_scipy_minimum prints it: huber 6.29e-6, cauchy
# 8.88e-6, noise 1.79e-7, mv 1.19e-8; the costs agree to 3e-13), and 16 x that for the kernels.  It is what scipy's stop at a
# finite-difference Jacobian leaves, not what the loop leaves.
MEASURED_LM_TO_SCIPY = 8.88e-6
SCIPY_BAR = 16.0 * MEASURED_LM_TO_SCIPY


# ---- small dense linear algebra in any float type (numpy.linalg has no longdouble) ---------------------------------------------------------
def chol(A):
    """lower L with A = L L^T, or None when a pivot is not positive"""
    A = np.array(A, copy=True)
    n = A.shape[0]
    for j in range(n):
        p = A[j, j]
        if not p > 0:
            return None
        s = np.sqrt(p)
        A[j, j] = s
        A[j + 1:, j] /= s
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def fsub(L, B):
    """L^-1 B"""
    X = np.array(B, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def bsub(L, B):
    """L^-T B"""
    X = np.array(B, copy=True)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


# ---- SO(3) ----------------------------------------------------------------------------------------------------------------------------------
def hat(p):
    z = p.dtype.type(0)
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], p.dtype)


def so3_exp(r):
    T = r.dtype.type
    t2 = r @ r
    if t2 > T(2.220446049250313e-16):
        th = np.sqrt(t2)
        K = hat(r / th)
        return np.eye(3, dtype=r.dtype) + np.sin(th) * K + (T(1) - np.cos(th)) * (K @ K)
    return np.eye(3, dtype=r.dtype) + hat(r)


def so3_log(R):
    T = R.dtype.type
    v = T(0.5) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], R.dtype)
    s2 = v @ v
    c = T(0.5) * (np.trace(R) - T(1))
    if s2 < T(1e-8):
        if c < 0:  # next to a half turn: R + R^T = 2 c I + 2 (1 - c) a a^T gives the axis, v = sin(theta) a its sign
            B = (T(0.5) * (R + R.T) - c * np.eye(3, dtype=R.dtype)) / (T(1) - c)
            m = int(np.argmax(np.diag(B)))
            a = B[m] / np.sqrt(B[m, m])
            return (T(-1) if v @ a < 0 else T(1)) * np.arctan2(np.sqrt(s2), c) * a
        k = T(1) + s2 * (T(1) / T(6) + s2 * (T(3) / T(40)))
    else:
        s = np.sqrt(s2)
        k = np.arctan2(s, c) / s
    return k * v


def so3_jlinv(p):
    T = p.dtype.type
    t2 = p @ p
    if t2 < T(1e-4):
        c = T(1) / T(12) + t2 * (T(1) / T(720) + t2 * (T(1) / T(30240)))
    else:
        th = np.sqrt(t2)
        c = T(1) / t2 - (T(1) + np.cos(th)) / (T(2) * th * np.sin(th))
    H = hat(p)
    return np.eye(3, dtype=p.dtype) - T(0.5) * H + c * (H @ H)


def loss(kind, a, s):
    """rho(s), rho'(s)"""
    T = type(s)
    if kind == LOSS_NONE:
        return s, T(1)
    a = T(a)
    if kind == LOSS_HUBER:
        if s <= a * a:
            return s, T(1)
        q = np.sqrt(s)
        return T(2) * a * q - a * a, a / q
    q = T(1) + s / (a * a)
    return a * a * np.log(q), T(1) / q


# ---- rules 1 and 2 ----------------------------------------------------------------------------------------------------------------------------
def measurement(batch, f, g, T):
    """(Rm, tm, W) of rule 1, or None"""
    if batch["pose_status"][f, g] != 0 or batch["cov_status"][f, g] != 0 or batch["cov_param"][f, g] != 0:
        return None
    cov = np.asarray(batch["cov"][f, g], T)
    rv, tv = np.asarray(batch["rvec"][f, g], T), np.asarray(batch["tvec"][f, g], T)
    d = np.diag(cov)
    if not (np.all(np.isfinite(d)) and np.all(d > 0) and np.all(np.isfinite(rv)) and np.all(np.isfinite(tv))):
        return None
    d = T(1) / np.sqrt(d)
    C = cov * np.outer(d, d)
    A = np.array(C, copy=True)
    for j in range(6):  # the pivots of rule 1
        p = A[j, j]
        if not p > T(1e-12):
            return None
        A[j + 1:, j] /= np.sqrt(p)
        A[j, j] = np.sqrt(p)
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    L = np.tril(A)
    Li = fsub(L, np.eye(6, dtype=T))
    return so3_exp(rv), tv, (Li.T @ Li) * np.outer(d, d)


def bad_input(batch, g):
    nf = batch["n_frames"]
    for f in range(nf):
        if batch["rec_rig"][f, g] != g or batch["rec_frame"][f, g] != f:
            return True
        if batch["cov_status"][f, g] == 0 and batch["cov_param"][f, g] == 1:
            return True
    return False


def pieces(measured, max_gap):
    """[(a, b)] of rule 2 from the measured flags of one rig"""
    out, idx = [], [f for f, m in enumerate(measured) if m]
    if not idx:
        return out
    a = prev = idx[0]
    for f in idx[1:]:
        if f - prev > max_gap:
            out.append((a, prev))
            a = f
        prev = f
    out.append((a, prev))
    return out


# ---- a piece ------------------------------------------------------------------------------------------------------------------------------------
class Piece:
    """frames a .. b of one rig: meas[k] is None or (Rm, tm, W); t[k] the times; the state is R[k], x[k] = (t, w, v) as a 9-vector"""

    def __init__(self, meas, t, opts, T):
        self.meas, self.t, self.o, self.T, self.n = meas, np.asarray(t, T), opts, T, len(meas)

    def prior_at(self):
        """the frame of the velocity prior: the piece's first"""
        return 0

    def start(self):
        T, n = self.T, self.n
        R, tr = [None] * n, [None] * n
        known = [k for k in range(n) if self.meas[k] is not None]
        for k in range(n):
            if self.meas[k] is not None:
                R[k], tr[k] = self.meas[k][0], self.meas[k][1]
            else:
                p = max(j for j in known if j < k)
                q = min(j for j in known if j > k)
                s = (self.t[k] - self.t[p]) / (self.t[q] - self.t[p])
                Rp, Rq = self.meas[p][0], self.meas[q][0]
                R[k] = so3_exp(s * so3_log(Rq @ Rp.T)) @ Rp
                tr[k] = self.meas[p][1] + s * (self.meas[q][1] - self.meas[p][1])
        w, v = [np.zeros(3, T)] * n, [np.zeros(3, T)] * n
        for k in range(n - 1):
            dt = self.t[k + 1] - self.t[k]
            w[k] = so3_log(R[k + 1] @ R[k].T) / dt
            v[k] = (tr[k + 1] - tr[k]) / dt
        if n > 1:
            w[n - 1], v[n - 1] = w[n - 2], v[n - 2]
        return [np.array(r, T) for r in R], [np.concatenate([tr[k], w[k], v[k]]) for k in range(n)]

    def motion_info(self, dt):
        T, o = self.T, self.o
        M = np.zeros((12, 12), T)
        for k in range(6):
            q = T(o["q_rot"] if k < 3 else o["q_trans"])
            M[k, k] = T(12) / (q * dt ** 3)
            M[k, 6 + k] = M[6 + k, k] = -T(6) / (q * dt ** 2)
            M[6 + k, 6 + k] = T(4) / (q * dt)
        return M

    def motion_residual(self, R, x, k):
        dt = self.t[k + 1] - self.t[k]
        psi = so3_log(R[k + 1] @ R[k].T)
        a = np.concatenate([psi - dt * x[k][3:6], x[k + 1][0:3] - x[k][0:3] - dt * x[k][6:9]])
        b = np.concatenate([x[k + 1][3:6] - x[k][3:6], x[k + 1][6:9] - x[k][6:9]])
        return dt, psi, np.concatenate([a, b])

    def prior_info(self):
        T, o = self.T, self.o
        return np.diag(np.array([T(1) / T(o["vel0_sigma_rot"]) ** 2] * 3 + [T(1) / T(o["vel0_sigma_trans"]) ** 2] * 3, T))

    def meas_residual(self, R, x, k):
        Rm, tm, W = self.meas[k]
        e = np.concatenate([so3_log(R[k] @ Rm.T), x[k][0:3] - tm])
        return e, e @ W @ e

    def cost(self, R, x):
        """rule 4, and per frame (mahalanobis2, weight)"""
        T, o = self.T, self.o
        c, per = T(0), []
        for k in range(self.n):
            if self.meas[k] is None:
                per.append((T(0), T(1)))
                continue
            e, m2 = self.meas_residual(R, x, k)
            rho, wt = loss(o["loss"], o["loss_scale"], m2)
            c += rho
            per.append((m2, wt))
        for k in range(self.n - 1):
            dt, _, r = self.motion_residual(R, x, k)
            c += r @ self.motion_info(dt) @ r
        wv = x[self.prior_at()][3:9]
        c += wv @ self.prior_info() @ wv
        return T(0.5) * c, per

    def linearise(self, R, x):
        """D [n, 12, 12], C [n - 1, 12, 12] (rows frame k + 1, columns frame k), gradient [n, 12]; unknown order theta, t, w, v"""
        T, n = self.T, self.n
        D, C, g = np.zeros((n, 12, 12), T), np.zeros((max(n - 1, 0), 12, 12), T), np.zeros((n, 12), T)
        I3 = np.eye(3, dtype=T)
        for k in range(n):
            if self.meas[k] is None:
                continue
            e, m2 = self.meas_residual(R, x, k)
            _, wt = loss(self.o["loss"], self.o["loss_scale"], m2)
            J = np.zeros((6, 12), T)
            J[0:3, 0:3] = so3_jlinv(e[0:3])
            J[3:6, 3:6] = I3
            W = wt * self.meas[k][2]
            D[k] += J.T @ W @ J
            g[k] += J.T @ W @ e
        for k in range(n - 1):
            dt, psi, r = self.motion_residual(R, x, k)
            M = self.motion_info(dt)
            A = so3_jlinv(psi)
            J0, J1 = np.zeros((12, 12), T), np.zeros((12, 12), T)
            J0[0:3, 0:3] = -A.T          # d Log(R1 (Exp(d) R0)^T) = -Jr^-1(psi) d, Jr^-1 = Jl^-1 ^T
            J0[0:3, 6:9] = -dt * I3
            J0[3:6, 3:6] = -I3
            J0[3:6, 9:12] = -dt * I3
            J0[6:9, 6:9] = -I3
            J0[9:12, 9:12] = -I3
            J1[0:3, 0:3] = A
            J1[3:6, 3:6] = I3
            J1[6:9, 6:9] = I3
            J1[9:12, 9:12] = I3
            D[k] += J0.T @ M @ J0
            D[k + 1] += J1.T @ M @ J1
            C[k] += J1.T @ M @ J0
            g[k] += J0.T @ M @ r
            g[k + 1] += J1.T @ M @ r
        P = self.prior_info()
        D[self.prior_at()][6:12, 6:12] += P
        g[self.prior_at()][6:12] += P @ x[self.prior_at()][3:9]
        return D, C, g

    def solve(self, D, C, g, lam, want_cov, dense=None):
        """delta of (A + lam diag A) delta = -g and, when asked, the 12x12 marginal blocks of A^-1; None when a pivot is not positive"""
        T, n = self.T, self.n
        if dense is None:
            dense = n <= DENSE_MAX_FRAMES
        damp = T(1) + T(lam)
        if dense:
            A = np.zeros((12 * n, 12 * n), T)
            for k in range(n):
                A[12 * k:12 * k + 12, 12 * k:12 * k + 12] = D[k]
                if k + 1 < n:
                    A[12 * k + 12:12 * k + 24, 12 * k:12 * k + 12] = C[k]
                    A[12 * k:12 * k + 12, 12 * k + 12:12 * k + 24] = C[k].T
            A[np.diag_indices(12 * n)] *= damp
            L = chol(A)
            if L is None:
                return None
            delta = bsub(L, fsub(L, -g.reshape(-1))).reshape(n, 12)
            if not want_cov:
                return delta, None
            Li = fsub(L, np.eye(12 * n, dtype=T))
            S = Li.T @ Li
            return delta, [S[12 * k:12 * k + 12, 12 * k:12 * k + 12] for k in range(n)]
        Ls, Zs, ys = [], [], []
        di = np.diag_indices(12)
        sub, rhs = np.zeros((12, 12), T), -g[0]
        for k in range(n):
            Dt = np.array(D[k], copy=True)
            Dt[di] *= damp
            L = chol(Dt - sub)
            if L is None:
                return None
            y = fsub(L, rhs)
            Ls.append(L)
            ys.append(y)
            if k + 1 < n:
                Z = fsub(L, C[k].T)
                Zs.append(Z)
                sub = Z.T @ Z
                rhs = -g[k + 1] - Z.T @ y
        delta, S = [None] * n, [None] * n
        for k in range(n - 1, -1, -1):
            Li = fsub(Ls[k], np.eye(12, dtype=T))
            if k == n - 1:
                delta[k] = bsub(Ls[k], ys[k])
                S[k] = Li.T @ Li
            else:
                delta[k] = bsub(Ls[k], ys[k] - Zs[k] @ delta[k + 1])
                if want_cov:
                    G = bsub(Ls[k], Zs[k])
                    S[k] = Li.T @ Li + G @ S[k + 1] @ G.T
        return np.array(delta), (S if want_cov else None)

    def apply(self, R, x, delta):
        return [so3_exp(delta[k][0:3]) @ R[k] for k in range(self.n)], [x[k] + delta[k][3:12] for k in range(self.n)]

    def run(self, dense=None):
        """rules 5-7 -> dict of the piece's result"""
        T, o = self.T, self.o
        R, x = self.start()
        cost, _ = self.cost(R, x)
        cost0, lam, rounds, active = cost, T(o["lambda0"]), 0, True
        while active:
            D, C, g = self.linearise(R, x)
            sol = self.solve(D, C, g, lam, False, dense)
            usable, ct = False, None
            if sol is not None:
                Rt, xt = self.apply(R, x, sol[0])
                ct, _ = self.cost(Rt, xt)
                usable = bool(np.isfinite(ct))
            rounds += 1
            if usable and ct < cost:
                drop = cost - ct
                cost, R, x = ct, Rt, xt
                lam = max(lam / T(3), T(1e-9))
                if drop < T(REL_TOL) * cost:
                    active = False
            else:
                lam = lam * T(4)
                if lam > T(LAMBDA_MAX):
                    active = False
            if rounds >= o["max_iterations"]:
                active = False
        return self.report(R, x, cost0, cost, rounds, dense)

    def report(self, R, x, cost0, cost, rounds, dense=None):
        D, C, g = self.linearise(R, x)
        sol = self.solve(D, C, g, 0, True, dense)
        _, per = self.cost(R, x)
        ok = sol is not None and bool(np.isfinite(cost))
        return dict(ok=ok, R=R, x=x, S=sol[1] if ok else None, per=per, cost0=cost0, cost=cost, rounds=rounds)


# ---- a batch --------------------------------------------------------------------------------------------------------------------------------------
def batch_opts(batch):
    o = dict(DEFAULTS)
    o.update(batch.get("opts", {}))
    return o


def batch_times(batch, T):
    if batch.get("times") is not None:
        return np.asarray(batch["times"], T)
    return np.arange(batch["n_frames"]).astype(T) * T(batch_opts(batch)["dt"])


def batch_pieces(batch, T=np.float64):
    """per rig: None for bad input, else (measurements [n_frames], [(a, b)])"""
    o, out = batch_opts(batch), []
    for g in range(batch["n_rigs"]):
        if bad_input(batch, g):
            out.append(None)
            continue
        meas = [measurement(batch, f, g, T) for f in range(batch["n_frames"])]
        out.append((meas, pieces([m is not None for m in meas], o["max_gap"])))
    return out


def smooth(batch, T=np.float64, dense=None, runner=None):
    """The whole call: dict of arrays shaped like ctag_track_rec's fields [n_frames, n_rigs] and ctag_track_stat's [n_rigs]."""
    nf, nr, o = batch["n_frames"], batch["n_rigs"], batch_opts(batch)
    t = batch_times(batch, T)
    rec = dict(status=np.full((nf, nr), NOT_TRACKED, np.int32), flags=np.zeros((nf, nr), np.uint32), rvec=np.zeros((nf, nr, 3), T),
               tvec=np.zeros((nf, nr, 3), T), w=np.zeros((nf, nr, 3), T), v=np.zeros((nf, nr, 3), T), cov=np.zeros((nf, nr, 6, 6), T),
               vel_sigma=np.zeros((nf, nr, 6), T), mahalanobis2=np.zeros((nf, nr), T), weight=np.zeros((nf, nr), T))
    stat = dict(status=np.zeros(nr, np.int32), n_measured=np.zeros(nr, np.int32), n_pieces=np.zeros(nr, np.int32), n_tracked=np.zeros(nr, np.int32),
                longest_piece=np.zeros(nr, np.int32), rounds=np.zeros(nr, np.int32), cost0=np.zeros(nr, T), cost=np.zeros(nr, T))
    table = []
    for g, entry in enumerate(batch_pieces(batch, T)):
        if entry is None:
            rec["status"][:, g] = BAD_INPUT
            stat["status"][g] = BAD_INPUT
            table.append(None)
            continue
        meas, pcs = entry
        table.append(pcs)
        stat["n_measured"][g] = sum(m is not None for m in meas)
        stat["n_pieces"][g] = len(pcs)
        for a, b in pcs:
            P = Piece(meas[a:b + 1], t[a:b + 1], o, T)
            res = runner(P) if runner else P.run(dense)
            stat["n_tracked"][g] += b - a + 1
            stat["longest_piece"][g] = max(stat["longest_piece"][g], b - a + 1)
            stat["rounds"][g] += res["rounds"]
            stat["cost0"][g] += res["cost0"]
            stat["cost"][g] += res["cost"]
            for k in range(b - a + 1):
                f = a + k
                rec["status"][f, g] = OK if res["ok"] else SINGULAR
                rec["rvec"][f, g] = so3_log(res["R"][k])
                rec["tvec"][f, g], rec["w"][f, g], rec["v"][f, g] = res["x"][k][0:3], res["x"][k][3:6], res["x"][k][6:9]
                m2, wt = res["per"][k]
                rec["weight"][f, g] = wt
                if meas[f] is not None:
                    rec["mahalanobis2"][f, g] = m2
                    rec["flags"][f, g] = FLAG_MEASURED | (FLAG_DOWNWEIGHTED if wt < 1 else 0)
                if res["ok"]:
                    S = res["S"][k]
                    rec["cov"][f, g] = np.triu(S[0:6, 0:6]) + np.triu(S[0:6, 0:6], 1).T
                    rec["vel_sigma"][f, g] = np.sqrt(np.diag(S)[6:12])
    return rec, stat, table


# ---- the independent minimum: scipy.optimize.least_squares on the whitened residual vector of rule 4 ----------------------------------------------
def scipy_minimum(P):
    """The minimum of piece P's cost (float64) by scipy's trust-region least squares on the residual vector, started from rule 5's start;
    -> the same dict Piece.run returns.  The state is a chart round the start: R = Exp(d) R0."""
    from scipy.optimize import least_squares
    T, n, o = P.T, P.n, P.o
    assert T is np.float64
    R0, x0 = P.start()
    Lp = np.sqrt(np.diag(P.prior_info()))

    def state(z):
        z = z.reshape(n, 12)
        return [so3_exp(z[k][0:3]) @ R0[k] for k in range(n)], [x0[k] + z[k][3:12] for k in range(n)]

    Lw = {k: np.linalg.cholesky(P.meas[k][2]).T for k in range(n) if P.meas[k] is not None}
    Lm = [np.linalg.cholesky(P.motion_info(P.t[k + 1] - P.t[k])).T for k in range(n - 1)]
    rf = []  # the frames each residual row reads
    for k in range(n):
        if P.meas[k] is not None:
            rf += [(k, k)] * 6
    for k in range(n - 1):
        rf += [(k, k + 1)] * 12
    rf += [(0, 0)] * 6
    row_frames = np.array(rf)

    def fun(z):
        R, x = state(z)
        out = []
        for k in range(n):
            if P.meas[k] is not None:
                e, m2 = P.meas_residual(R, x, k)
                rho, _ = loss(o["loss"], o["loss_scale"], np.float64(m2))
                out.append((Lw[k] @ e) * (np.sqrt(rho / m2) if m2 > 0 else 1.0))
        for k in range(n - 1):
            out.append(Lm[k] @ P.motion_residual(R, x, k)[2])
        out.append(Lp * x[0][3:9])
        return np.concatenate(out)

    def jac(z):
        """central differences, the columns 36 apart together: a residual reads two neighbouring frames, 24 consecutive columns"""
        J = np.zeros((len(row_frames), 12 * n))
        h = 1e-6
        for c0 in range(min(36, 12 * n)):
            cols = np.arange(c0, 12 * n, 36)
            d = np.zeros(12 * n)
            d[cols] = h
            diff = (fun(z + d) - fun(z - d)) / (2 * h)
            for c in cols:  # a row belongs to the one column of the group whose frame it reads
                rows = (row_frames[:, 0] <= c // 12) & (c // 12 <= row_frames[:, 1])
                J[rows, c] = diff[rows]
        return J

    z = np.zeros(12 * n)
    sol = least_squares(fun, z, jac=jac, method="trf", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=100)
    R, x = state(sol.x)
    c0, _ = P.cost(R0, x0)
    c, _ = P.cost(R, x)
    return P.report(R, x, c0, c, int(sol.nfev))


# ---- comparison in the units of the bars ---------------------------------------------------------------------------------------------------------
def deviation(got, want, want_stat=None, got_stat=None):
    """{field: worst deviation} of the records `got` from `want` (dicts as smooth returns), over the frames whose status is OK in both"""
    ok = (np.asarray(got["status"]) == OK) & (np.asarray(want["status"]) == OK)
    out = {k: 0.0 for k in MEASURED_F64_DEVIATION}
    if ok.any():
        W = {k: np.asarray(v, np.longdouble) for k, v in want.items() if k not in ("status", "flags")}
        G = {k: np.asarray(v, np.longdouble) for k, v in got.items() if k not in ("status", "flags")}
        sd = np.sqrt(np.einsum("fgii->fgi", W["cov"]))
        with np.errstate(invalid="ignore", divide="ignore"):
            pose = np.abs(np.concatenate([G["rvec"] - W["rvec"], G["tvec"] - W["tvec"]], -1)) / sd
            vel = np.abs(np.concatenate([G["w"] - W["w"], G["v"] - W["v"]], -1)) / W["vel_sigma"]
            cov = np.abs(G["cov"] - W["cov"]) / (sd[..., :, None] * sd[..., None, :])
            vs = np.abs(G["vel_sigma"] - W["vel_sigma"]) / W["vel_sigma"]
            m2 = np.abs(G["mahalanobis2"] - W["mahalanobis2"]) / (1 + W["mahalanobis2"])
            wt = np.abs(G["weight"] - W["weight"]) / W["weight"]
        for name, arr in (("pose", pose), ("vel", vel), ("cov", cov), ("vel_sigma", vs), ("mahalanobis2", m2), ("weight", wt)):
            out[name] = float(np.max(arr[ok]))
    if want_stat is not None:
        for k in ("cost0", "cost"):
            w_, g_ = np.asarray(want_stat[k], np.longdouble), np.asarray(got_stat[k], np.longdouble)
            nz = w_ != 0
            if nz.any():
                out["cost"] = max(out["cost"], float(np.max(np.abs(g_[nz] - w_[nz]) / np.abs(w_[nz]))))
    return out
