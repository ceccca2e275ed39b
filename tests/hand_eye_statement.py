"""The hand-eye fit of include/ctag_pose.h (hand-eye calibration, rules 1-8) stated independently in numpy / scipy, in float64 and in
longdouble.  Nothing here comes from csrc, oracle or testkit.  The formulation differs from the kernels' on purpose: a dense 6 x 12
Jacobian per frame, the Gauss-Newton matrix as a plain sum over the frames in frame order, the start's 6 x 6 normal matrix as the plain
sum of J^T J, the nearest rotation from the eigenvectors of S^T S, and the covariance by Gauss-Jordan inversion.  The kernels sum in
chunks of 64 and factor by Cholesky; this file never does either for a result.

A batch is a dict (tests/hand_eye_shapes.py): n_frames, n_rigs, opts (dict of ctag_hand_eye_opts fields), links_rvec, links_tvec
[n_frames, 3], pose_status, rvec, tvec [n_frames, n_rigs, ...], cov_status, cov_param, cov [n_frames, n_rigs, 6, 6], rec_rig, rec_frame.

Bars.  MEASURED_F64_DEVIATION(_STEP) is the worst deviation between this statement in float64 and in longdouble over the batches of
hand_eye_shapes.BATCHES, per field, in the units of deviation() below: P and Q in units of their own sigma (sqrt of the diagonal of the
longdouble result's cov), cov entries over sqrt(cov_ii cov_jj), frame residuals in units of the frame's input sigma, mahalanobis2 over
1 + its value, weights, costs, sigma2_hat and min_pivot relative.  tests/test_hand_eye_statement_cpu.py measures it again
(-k deviation) and prints it; the figures below are that test's output.  BAR = 16 x the figure, the project's margin: the kernels run
the same float64 arithmetic in another order."""
import numpy as np

OK, TOO_FEW, BAD_INPUT, SINGULAR = 0, 1, 2, 3
LOSS_HUBER, LOSS_CAUCHY, LOSS_NONE = 0, 1, 2
CAMERA_ON_LINK, RIG_ON_LINK = 0, 1
FLAG_USED, FLAG_DOWNWEIGHTED = 1, 2
REL_TOL, LAMBDA_MAX, MIN_PIVOT, MAX_ANGLE = 1e-12, 1e6, 1e-12, 3.0

DEFAULTS = dict(mode=CAMERA_ON_LINK, loss=LOSS_NONE, max_iterations=20, loss_scale=4.0, lambda0=1e-3)

# measured by tests/test_hand_eye_statement_cpu.py::test_f64_deviation (python -m pytest -s tests/test_hand_eye_statement_cpu.py -k deviation),
# which prints both dicts.  _STEP: one undamped Gauss-Newton step from the start on every batch; the other one: that and the full loop.
# The loop's pose figure is three orders above the step's because its last rounds are decided by cost differences at the rounding of
# the cost: next to the minimum a trial is accepted or rejected by the last bits of two sums, and a rejected one leaves the state where
# it was (the float64 and the longdouble run take a different number of rounds in 66 of the 200 problems of `chi2`).
MEASURED_F64_DEVIATION_STEP = {"pose": 6.90e-11, "cov": 2.88e-13, "e": 4.32e-12, "mahalanobis2": 6.66e-12, "weight": 2.04e-13, "cost": 4.32e-13,
                               "sigma2_hat": 3.25e-13, "min_pivot": 1.90e-13}
MEASURED_F64_DEVIATION = {"pose": 1.23e-7, "cov": 3.94e-11, "e": 3.68e-8, "mahalanobis2": 1.58e-8, "weight": 2.36e-13, "cost": 4.32e-13,
                          "sigma2_hat": 3.25e-13, "min_pivot": 2.71e-11}
BAR_STEP = {k: 16.0 * v for k, v in MEASURED_F64_DEVIATION_STEP.items()}
BAR = {k: 16.0 * v for k, v in MEASURED_F64_DEVIATION.items()}
# the distance, in units of the result's own sigma, between this statement's LM result and scipy's minimum over
# hand_eye_shapes.SCIPY_BATCHES (test_lm_reaches_scipy_minimum prints it: huber 1.06e-7, cauchy 2.69e-5, mode1 6.01e-10, mv 2.80e-9,
# illscaled 1.29e-8; the costs agree to 3e-12), and 16 x that for the kernels.  It is what scipy's stop leaves, not what the loop leaves.
MEASURED_LM_TO_SCIPY = 2.69e-5
SCIPY_BAR = 16.0 * MEASURED_LM_TO_SCIPY


# ---- small dense linear algebra in any float type (numpy.linalg has no longdouble) ---------------------------------------------------------
def chol(A):
    """(lower L with A = L L^T or None at a pivot that is not above 0, the smallest pivot met)"""
    A = np.array(A, copy=True)
    n = A.shape[0]
    mp = A[0, 0]
    for j in range(n):
        p = A[j, j]
        if not p >= mp:
            mp = p
        if not p > 0:
            return None, mp
        s = np.sqrt(p)
        A[j, j] = s
        A[j + 1:, j] /= s
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A), mp


def solve_chol(L, b):
    y = np.array(b, copy=True)
    n = len(b)
    for i in range(n):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def inverse(A):
    """Gauss-Jordan with partial pivoting"""
    n = A.shape[0]
    M = np.concatenate([np.array(A, copy=True), np.eye(n, dtype=A.dtype)], 1)
    for j in range(n):
        p = j + int(np.argmax(np.abs(M[j:, j])))
        M[[j, p]] = M[[p, j]]
        M[j] = M[j] / M[j, j]
        for i in range(n):
            if i != j:
                M[i] = M[i] - M[i, j] * M[j]
    return M[:, n:]


def eig_sym3(A):
    """eigenvalues (descending) and eigenvectors (columns) of a symmetric 3x3 by cyclic Jacobi"""
    T = A.dtype.type
    A = np.array(A, copy=True)
    V = np.eye(3, dtype=A.dtype)
    for _ in range(60):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        if off <= np.finfo(A.dtype).tiny or off <= np.finfo(A.dtype).eps * T(1e-3) * np.trace(np.abs(A)):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p, q] == 0:
                continue
            th = (A[q, q] - A[p, p]) / (T(2) * A[p, q])
            t = np.sign(th) / (abs(th) + np.sqrt(th * th + T(1))) if th != 0 else T(1)
            c = T(1) / np.sqrt(t * t + T(1))
            s = t * c
            G = np.eye(3, dtype=A.dtype)
            G[p, p] = G[q, q] = c
            G[p, q], G[q, p] = s, -s
            A = G.T @ A @ G
            V = V @ G
    w = np.diag(A)
    order = np.argsort(-w, kind="stable")
    return w[order], V[:, order]


def nearest_rotation(S):
    """U diag(1, 1, det(U V^T)) V^T of S = U diag(s) V^T: the two leading singular pairs and their cross products"""
    _, V = eig_sym3(S.T @ S)
    v1, v2 = V[:, 0], V[:, 1]
    u1 = S @ v1
    u1 = u1 / np.sqrt(u1 @ u1)
    u2 = S @ v2
    u2 = u2 - (u2 @ u1) * u1
    u2 = u2 / np.sqrt(u2 @ u2)
    return np.outer(u1, v1) + np.outer(u2, v2) + np.outer(np.cross(u1, u2), np.cross(v1, v2))


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
        if c < 0:  # next to a half turn: the axis from the symmetric part, its sign from the antisymmetric one
            B = (T(0.5) * (R + R.T) - c * np.eye(3, dtype=R.dtype)) / (T(1) - c)
            m = int(np.argmax(np.diag(B)))
            a = B[m] / np.sqrt(B[m, m])
            return (T(-1) if v @ a < 0 else T(1)) * np.arctan2(np.sqrt(s2), c) * a
        return (T(1) + s2 * (T(1) / T(6) + s2 * (T(3) / T(40)))) * v
    s = np.sqrt(s2)
    return (np.arctan2(s, c) / s) * v


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


# ---- rule 1 -------------------------------------------------------------------------------------------------------------------------------------
def measurement(batch, f, g, T, identity_weight=False):
    """(Rm, tm, W) of rule 1, or None.  identity_weight is a planted error of the CPU test."""
    if batch["pose_status"][f, g] != 0 or batch["cov_status"][f, g] != 0 or batch["cov_param"][f, g] != 0:
        return None
    cov = np.asarray(batch["cov"][f, g], T)
    rv, tv = np.asarray(batch["rvec"][f, g], T), np.asarray(batch["tvec"][f, g], T)
    d = np.diag(cov)
    if not (np.all(np.isfinite(d)) and np.all(d > 0) and np.all(np.isfinite(rv)) and np.all(np.isfinite(tv))):
        return None
    d = T(1) / np.sqrt(d)
    L, _ = chol(cov * np.outer(d, d))
    if L is None or not np.all(np.diag(L) ** 2 > T(MIN_PIVOT)):
        return None
    W = inverse(cov * np.outer(d, d)) * np.outer(d, d)
    W = T(0.5) * (W + W.T)
    if identity_weight:
        W = np.eye(6, dtype=T)
    return so3_exp(rv), tv, W


def bad_input(batch, g):
    for f in range(batch["n_frames"]):
        if batch["rec_rig"][f, g] != g or batch["rec_frame"][f, g] != f:
            return True
        if batch["cov_status"][f, g] == 0 and batch["cov_param"][f, g] == 1:
            return True
    return False


def link_transforms(batch, T, mode=None, transpose_rc=False):
    """[(R_C, t_C) or None] per frame, as the mode says"""
    mode = batch_opts(batch)["mode"] if mode is None else mode
    out = []
    for f in range(batch["n_frames"]):
        rv, tv = np.asarray(batch["links_rvec"][f], T), np.asarray(batch["links_tvec"][f], T)
        if not (np.all(np.isfinite(rv)) and np.all(np.isfinite(tv))):
            out.append(None)
            continue
        R = so3_exp(rv)
        if mode == CAMERA_ON_LINK:
            R, tv = R.T, -(R.T @ tv)
        out.append((R.T if transpose_rc else R, tv))
    return out


def batch_opts(batch):
    o = dict(DEFAULTS)
    o.update(batch.get("opts") or {})
    return o


# ---- one problem ------------------------------------------------------------------------------------------------------------------------------
class Problem:
    """the used frames of one rig: C [(R_C, t_C)], M [(Rm, tm, W)], in frame order"""

    def __init__(self, C, M, opts, T, rvec_param=False):
        self.C, self.M, self.o, self.T, self.n, self.rvec_param = C, M, opts, T, len(C), rvec_param

    def start(self):
        """rule 5 -> (R_P, t_P, R_Q, t_Q) or None when the 6x6 meets a pivot that is not positive"""
        T = self.T
        S = np.zeros((3, 3), T)
        for k in range(self.n):
            a = so3_log(self.M[k][0] @ self.M[0][0].T)
            b = so3_log(self.C[k][0] @ self.C[0][0].T)
            if np.sqrt(a @ a) > T(MAX_ANGLE) or np.sqrt(b @ b) > T(MAX_ANGLE):
                continue
            S += np.outer(a, b)
        RP = nearest_rotation(S)
        S2 = np.zeros((3, 3), T)
        for (RC, _), (Rm, _, _) in zip(self.C, self.M):
            S2 += RC.T @ RP.T @ Rm
        RQ = nearest_rotation(S2)
        A, g = np.zeros((6, 6), T), np.zeros(6, T)
        for (RC, tC), (_, tm, _) in zip(self.C, self.M):
            J = np.concatenate([RP @ RC, np.eye(3, dtype=T)], 1)
            A += J.T @ J
            g += J.T @ (tm - RP @ tC)
        L, _ = chol(A)
        if L is None:
            return None
        x = solve_chol(L, g)
        return RP, x[3:6], RQ, x[0:3]

    def residual(self, st, k):
        RP, tP, RQ, tQ = st
        RC, tC = self.C[k]
        Rm, tm, _ = self.M[k]
        u = RP @ (RC @ tQ + tC)
        R = RP @ RC @ RQ
        rot = so3_log(R) - so3_log(Rm) if self.rvec_param else so3_log(R @ Rm.T)
        return np.concatenate([rot, u + tP - tm]), u

    def jacobian(self, st, k):
        """rule 4: the 6x12 Jacobian of frame k's residual in rule 2's coordinates"""
        T = self.T
        e, u = self.residual(st, k)
        B = st[0] @ self.C[k][0]
        Ji = so3_jlinv(e[0:3])
        J = np.zeros((6, 12), T)
        J[0:3, 0:3], J[0:3, 6:9] = Ji, Ji @ B
        J[3:6, 0:3], J[3:6, 3:6], J[3:6, 9:12] = -hat(u), np.eye(3, dtype=T), B
        return J

    def frame_terms(self, st, k):
        e, _ = self.residual(st, k)
        W = self.M[k][2]
        s = e @ W @ e
        rho, w = loss(self.o["loss"], self.o["loss_scale"], s)
        return e, s, rho, w

    def downweighted(self, s):
        """rule 8: the frame lies beyond the loss's scale"""
        return self.o["loss"] != LOSS_NONE and bool(s > self.T(self.o["loss_scale"]) ** 2)

    def cost(self, st):
        c = self.T(0)
        for k in range(self.n):
            c += self.T(0.5) * self.frame_terms(st, k)[2]
        return c

    def linearise(self, st):
        T = self.T
        A, g, c = np.zeros((12, 12), T), np.zeros(12, T), T(0)
        for k in range(self.n):
            e, _, rho, w = self.frame_terms(st, k)
            J = self.jacobian(st, k)
            WJ = self.M[k][2] @ J
            A += w * (J.T @ WJ)
            g += w * (WJ.T @ e)
            c += T(0.5) * rho
        return A, g, c

    @staticmethod
    def apply(st, d):
        return so3_exp(d[0:3]) @ st[0], st[1] + d[3:6], so3_exp(d[6:9]) @ st[2], st[3] + d[9:12]

    def run(self):
        """rules 5-8 -> dict(status, state, cost0, cost, lambda, rounds)"""
        T, o = self.T, self.o
        st = self.start()
        if st is None:
            return dict(status=SINGULAR, state=None)
        cost0 = cost = self.cost(st)
        lam, rounds, active = T(o["lambda0"]), 0, bool(np.isfinite(cost))
        while active:
            A, g, _ = self.linearise(st)
            L, _ = chol(A + lam * np.diag(np.diag(A)))
            usable, ct, trial = False, T(0), None
            if L is not None:
                trial = self.apply(st, solve_chol(L, -g))
                ct = self.cost(trial)
                usable = bool(np.isfinite(ct))
            rounds += 1
            if usable and ct < cost:
                drop = cost - ct
                cost, st = ct, trial
                lam = max(lam / T(3), T(1e-9))
                if drop < T(REL_TOL) * cost:
                    active = False
            else:
                lam = lam * T(4)
                if lam > T(LAMBDA_MAX):
                    active = False
            if rounds >= o["max_iterations"]:
                active = False
        return dict(status=OK, state=st, cost0=cost0, cost=cost, lam=lam, rounds=rounds)

    def report(self, r):
        """rule 8 from a run's (or scipy's) state"""
        T = self.T
        out = dict(status=r["status"], n_used=self.n, n_downweighted=0, rounds=0, dof=6 * self.n - 12, P_rvec=np.zeros(3, T), P_tvec=np.zeros(3, T),
                   Q_rvec=np.zeros(3, T), Q_tvec=np.zeros(3, T), cost0=T(0), cost=T(0), lam=T(0), sigma2_hat=T(0), min_pivot=T(0),
                   cov=np.zeros((12, 12), T), frames=None)
        st = r["state"]
        if st is None:
            return out
        out.update(P_rvec=so3_log(st[0]), P_tvec=st[1], Q_rvec=so3_log(st[2]), Q_tvec=st[3], cost0=r["cost0"], cost=r["cost"], lam=r["lam"],
                   rounds=r["rounds"])
        if out["dof"] > 0:
            out["sigma2_hat"] = T(2) * r["cost"] / T(out["dof"])
        A, _, _ = self.linearise(st)
        d = np.diag(A)
        good = bool(np.isfinite(r["cost"])) and bool(np.all(np.isfinite(d))) and bool(np.all(d > 0))
        if good:
            d = T(1) / np.sqrt(d)
            L, mp = chol(A * np.outer(d, d))
            out["min_pivot"] = mp
            good = L is not None and bool(np.all(np.diag(L) ** 2 > T(MIN_PIVOT)))
            if L is None or not good:  # the smallest pivot met up to the failing one
                piv = []
                Cm = np.array(A * np.outer(d, d), copy=True)
                for j in range(12):
                    piv.append(Cm[j, j])
                    if not Cm[j, j] > T(MIN_PIVOT):
                        break
                    Cm[j + 1:, j] /= np.sqrt(Cm[j, j])
                    Cm[j + 1:, j + 1:] -= np.outer(Cm[j + 1:, j], Cm[j + 1:, j])
                out["min_pivot"] = min(piv)
        if good:
            cov = inverse(A)
            out["cov"] = T(0.5) * (cov + cov.T)
        else:
            out["status"] = SINGULAR
        fr = []
        for k in range(self.n):
            e, s, _, w = self.frame_terms(st, k)
            fr.append((e, s, w))
        out["frames"] = fr
        out["n_downweighted"] = sum(1 for _, s, _ in fr if self.downweighted(s))
        return out


REC_FIELDS = ("status", "n_used", "n_downweighted", "rounds", "dof", "P_rvec", "P_tvec", "Q_rvec", "Q_tvec", "cost0", "cost", "lam", "sigma2_hat",
              "min_pivot", "cov")
FRAME_FIELDS = ("status", "flags", "e", "mahalanobis2", "weight")


def problems(batch, T=np.float64, mode=None, transpose_rc=False, identity_weight=False, rvec_param=False):
    """per rig: ('bad', None, None) or (None, Problem, used frame indices)"""
    o = batch_opts(batch)
    C = link_transforms(batch, T, mode, transpose_rc)
    out = []
    for g in range(batch["n_rigs"]):
        if bad_input(batch, g):
            out.append(("bad", None, None))
            continue
        used, Cs, Ms = [], [], []
        for f in range(batch["n_frames"]):
            m = measurement(batch, f, g, T, identity_weight) if C[f] is not None else None
            if m is not None:
                used.append(f)
                Cs.append(C[f])
                Ms.append(m)
        out.append((None, Problem(Cs, Ms, o, T, rvec_param), used))
    return out


def fit(batch, T=np.float64, runner=None, **planted):
    """-> (rec: {field: array over rigs}, frames: {field: array [n_frames, n_rigs]}) in the layout of the library's records"""
    nf, nr = batch["n_frames"], batch["n_rigs"]
    rec = dict(status=np.zeros(nr, np.int32), n_used=np.zeros(nr, np.int32), n_downweighted=np.zeros(nr, np.int32), rounds=np.zeros(nr, np.int32),
               dof=np.zeros(nr, np.int32), P_rvec=np.zeros((nr, 3), T), P_tvec=np.zeros((nr, 3), T), Q_rvec=np.zeros((nr, 3), T),
               Q_tvec=np.zeros((nr, 3), T), cost0=np.zeros(nr, T), cost=np.zeros(nr, T), lam=np.zeros(nr, T), sigma2_hat=np.zeros(nr, T),
               min_pivot=np.zeros(nr, T), cov=np.zeros((nr, 12, 12), T))
    frames = dict(status=np.zeros((nf, nr), np.int32), flags=np.zeros((nf, nr), np.uint32), e=np.zeros((nf, nr, 6), T),
                  mahalanobis2=np.zeros((nf, nr), T), weight=np.zeros((nf, nr), T))
    for g, (bad, P, used) in enumerate(problems(batch, T, **planted)):
        if bad:
            rec["status"][g] = BAD_INPUT
            continue
        if P.n < 3:
            rec["status"][g], rec["n_used"][g] = TOO_FEW, P.n
            continue
        with np.errstate(all="ignore"):   # a singular problem may run through non-finite numbers on its way to its status
            r = P.report((runner or Problem.run)(P))
        for k in REC_FIELDS:
            rec[k][g] = r[k]
        if r["frames"] is not None:
            for f, (e, s, w) in zip(used, r["frames"]):
                frames["status"][f, g] = r["status"]
                frames["flags"][f, g] = FLAG_USED | (FLAG_DOWNWEIGHTED if P.downweighted(s) else 0)
                frames["e"][f, g], frames["mahalanobis2"][f, g], frames["weight"][f, g] = e, s, w
    return rec, frames


# ---- the independent minimum: scipy.optimize.least_squares on the whitened residuals of rule 3 --------------------------------------------------
def scipy_minimum(P):
    """The minimum of problem P's cost (float64) from rule 5's start, in a chart round the start; -> what Problem.run returns."""
    from scipy.optimize import least_squares
    assert P.T is np.float64
    st0 = P.start()
    if st0 is None:
        return dict(status=SINGULAR, state=None)
    Lw = [np.linalg.cholesky(P.M[k][2]).T for k in range(P.n)]

    def fun(z):
        st = Problem.apply(st0, z)
        out = []
        for k in range(P.n):
            e, s, rho, _ = P.frame_terms(st, k)
            out.append((Lw[k] @ e) * (np.sqrt(rho / s) if s > 0 else 1.0))
        return np.concatenate(out)

    sol = least_squares(fun, np.zeros(12), jac="3-point", method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=200)
    st = Problem.apply(st0, sol.x)
    return dict(status=OK, state=st, cost0=P.cost(st0), cost=P.cost(st), lam=np.float64(0), rounds=int(sol.nfev))


# ---- comparison in the units of the bars ---------------------------------------------------------------------------------------------------------
def tangent_difference(got, want):
    """[n_rigs, 12]: (Log(R_P R_P'^T), t_P - t_P', Log(R_Q R_Q'^T), t_Q - t_Q') in longdouble"""
    L = np.longdouble
    nr = len(want["status"])
    d = np.zeros((nr, 12), L)
    for g in range(nr):
        for c, (rv, tv) in enumerate((("P_rvec", "P_tvec"), ("Q_rvec", "Q_tvec"))):
            Ra, Rb = so3_exp(np.asarray(got[rv][g], L)), so3_exp(np.asarray(want[rv][g], L))
            d[g, 6 * c:6 * c + 3] = so3_log(Ra @ Rb.T)
            d[g, 6 * c + 3:6 * c + 6] = np.asarray(got[tv][g], L) - np.asarray(want[tv][g], L)
    return d


def deviation(got, want, got_frames=None, want_frames=None, frame_sigma=None):
    """{field: worst deviation} of the records `got` from `want` over the problems that are OK in both"""
    L = np.longdouble
    ok = (np.asarray(got["status"]) == OK) & (np.asarray(want["status"]) == OK)
    out = {k: 0.0 for k in MEASURED_F64_DEVIATION}
    if not ok.any():
        return out
    Wc, Gc = np.asarray(want["cov"], L), np.asarray(got["cov"], L)
    sd = np.sqrt(np.einsum("gii->gi", Wc))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["pose"] = float(np.max((np.abs(tangent_difference(got, want)) / sd)[ok]))
        out["cov"] = float(np.max((np.abs(Gc - Wc) / (sd[:, :, None] * sd[:, None, :]))[ok]))
        for k in ("cost0", "cost"):
            w_, g_ = np.asarray(want[k], L)[ok], np.asarray(got[k], L)[ok]
            nz = w_ != 0
            if nz.any():
                out["cost"] = max(out["cost"], float(np.max(np.abs(g_[nz] - w_[nz]) / np.abs(w_[nz]))))
        for k in ("sigma2_hat", "min_pivot"):
            w_, g_ = np.asarray(want[k], L)[ok], np.asarray(got[k], L)[ok]
            nz = w_ != 0
            if nz.any():
                out[k] = float(np.max(np.abs(g_[nz] - w_[nz]) / np.abs(w_[nz])))
        if want_frames is not None:
            used = (np.asarray(want_frames["flags"]) & FLAG_USED).astype(bool) & ok[None, :]
            if used.any():
                We, Ge = np.asarray(want_frames["e"], L), np.asarray(got_frames["e"], L)
                out["e"] = float(np.max((np.abs(Ge - We) / np.asarray(frame_sigma, L))[used]))
                Wm, Gm = np.asarray(want_frames["mahalanobis2"], L), np.asarray(got_frames["mahalanobis2"], L)
                out["mahalanobis2"] = float(np.max((np.abs(Gm - Wm) / (1 + Wm))[used]))
                Ww, Gw = np.asarray(want_frames["weight"], L), np.asarray(got_frames["weight"], L)
                out["weight"] = float(np.max((np.abs(Gw - Ww) / Ww)[used]))
    return out


def frame_sigma(batch):
    """[n_frames, n_rigs, 6]: the square roots of the diagonals of the input covariances (1 where there is none)"""
    d = np.einsum("fgii->fgi", np.asarray(batch["cov"], np.float64))
    return np.where(d > 0, np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
