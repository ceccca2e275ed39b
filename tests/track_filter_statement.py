"""The track filter of include/ctag_pose.h (track filtering, rules 1-8) stated independently in numpy, in float64 and in longdouble,
from the header's rules.  Nothing here comes from csrc, oracle or testkit; the SO(3) functions, `measurement` and `loss` are
track_statement.py's.  The formulation differs from the kernel's on purpose: F, H, Q, K and the Joseph form are dense 12x12 / 6x12
matrices multiplied as such; the kernel uses their block structure.

A batch is track_statement.py's dict; opts holds ctag_track_filter_opts fields.  `Filter` keeps the state between calls as the library's
object does, so a batch can be given in one call or in pieces.

Bars.  MEASURED_F64_DEVIATION is the worst deviation between this statement in float64 and in longdouble over every batch of
track_filter_shapes.BATCHES, per field, in track_statement.deviation's units (poses and velocities in their own sigma, cov entries over
sqrt(cov_ii cov_jj), vel_sigma and weights relative, mahalanobis2 over 1 + its value).  tests/test_track_filter_statement_cpu.py
measures it again (-k deviation) and prints it; the figures below are that test's output.  BAR = 16 x the figure, the allowance
track_statement.py gives for the same reason: the kernel runs the same float64 arithmetic in another order.
MEASURED_LINK_DEVIATION is the same figure for the two statements (this one and track_statement.smooth) on the linear batches of the
link test, LINK_BAR = 16 x it."""
import numpy as np

import track_statement as ts

OK, NOT_TRACKED, BAD_INPUT, SINGULAR = 0, 1, 2, 3
FLAG_MEASURED, FLAG_DOWNWEIGHTED, FLAG_GATED, FLAG_STARTED = 1, 2, 4, 8
MIN_PIVOT = 1e-12

DEFAULTS = dict(loss=ts.LOSS_NONE, max_gap=5, dt=1.0 / 30.0, q_rot=0.1, q_trans=3000.0, vel0_sigma_rot=10.0, vel0_sigma_trans=1000.0,
                loss_scale=4.0, gate=0.0)

# python -m pytest -s tests/test_track_filter_statement_cpu.py -k deviation
MEASURED_F64_DEVIATION = {"pose": 2.77e-08, "vel": 2.1e-10, "cov": 1.89e-12, "vel_sigma": 1.22e-12, "mahalanobis2": 1.22e-10, "weight": 5.17e-14}
BAR = {k: 16.0 * v for k, v in MEASURED_F64_DEVIATION.items()}
# python -m pytest -s tests/test_track_filter_statement_cpu.py -k link
MEASURED_LINK_DEVIATION = {"pose": 5.64e-13, "vel": 2.97e-13, "cov": 3.67e-15, "vel_sigma": 2.16e-14}
LINK_BAR = {k: 16.0 * v for k, v in MEASURED_LINK_DEVIATION.items()}


def so3_jl(p):
    """the left Jacobian of SO(3)"""
    T = p.dtype.type
    t2 = p @ p
    if t2 < T(1e-2):
        b = T(1) / T(2) + t2 * (-T(1) / T(24) + t2 * (T(1) / T(720) + t2 * (-T(1) / T(40320) + t2 * (T(1) / T(3628800)))))
        c = T(1) / T(6) + t2 * (-T(1) / T(120) + t2 * (T(1) / T(5040) + t2 * (-T(1) / T(362880) + t2 * (T(1) / T(39916800)))))
    else:
        th = np.sqrt(t2)
        b = (T(1) - np.cos(th)) / t2
        c = (th - np.sin(th)) / (t2 * th)
    H = ts.hat(p)
    return np.eye(3, dtype=p.dtype) + b * H + c * (H @ H)


def sym_inverse(A):
    """A^-1 by rule 4's factorisation (unit diagonal, pivots above 1e-12), or None"""
    T = A.dtype.type
    d = np.diag(A)
    if not (np.all(np.isfinite(d)) and np.all(d > 0)):
        return None
    d = T(1) / np.sqrt(d)
    C = A * np.outer(d, d)
    n = A.shape[0]
    for j in range(n):
        p = C[j, j]
        if not p > T(MIN_PIVOT):
            return None
        C[j + 1:, j] /= np.sqrt(p)
        C[j, j] = np.sqrt(p)
        C[j + 1:, j + 1:] -= np.outer(C[j + 1:, j], C[j + 1:, j])
    Li = ts.fsub(np.tril(C), np.eye(n, dtype=A.dtype))
    return (Li.T @ Li) * np.outer(d, d)


def sym_upper(A):
    return np.triu(A) + np.triu(A, 1).T


def transition(w, D, o, T):
    """rule 3: E, F, Q for the step D at angular velocity w"""
    I3 = np.eye(3, dtype=T)
    E = ts.so3_exp(D * w)
    F = np.eye(12, dtype=T)
    F[0:3, 0:3] = E
    F[0:3, 6:9] = D * so3_jl(D * w)
    F[3:6, 9:12] = D * I3
    Q = np.zeros((12, 12), T)
    for k in range(6):
        q = T(o["q_rot"] if k < 3 else o["q_trans"])
        Q[k, k] = q * D ** 3 / T(3)
        Q[k, 6 + k] = Q[6 + k, k] = q * D * D / T(2)
        Q[6 + k, 6 + k] = q * D
    return E, F, Q


def observation(Rp, tp, Rm, tm, T):
    """rule 4: e and H"""
    phi = ts.so3_log(Rp @ Rm.T)
    H = np.zeros((6, 12), T)
    H[0:3, 0:3] = ts.so3_jlinv(phi)
    H[3:6, 3:6] = np.eye(3, dtype=T)
    return np.concatenate([phi, tp - tm]), H


class Track:
    def __init__(self):
        self.tracking, self.misses = False, 0
        self.R = self.t = self.w = self.v = self.P = self.tprev = None

    def copy(self):
        c = Track()
        c.__dict__.update(self.__dict__)
        return c


def predicted(s, t, o, T):
    """rule 3 applied to track s -> a new Track at time t"""
    D = T(t) - s.tprev
    E, F, Q = transition(s.w, D, o, T)
    n = s.copy()
    n.R, n.t, n.P, n.tprev = E @ s.R, s.t + D * s.v, sym_upper(F @ s.P @ F.T + Q), T(t)
    return n


def step(s, meas, t, o, T):
    """one frame of one rig: (new Track, record fields) by rules 2-6; meas is None or (Rm, tm, cov_f)"""
    zero = dict(status=NOT_TRACKED, flags=0, full=False, m2=T(0), wt=T(0))
    if not s.tracking:
        if meas is None:
            return s, zero
        n = Track()
        n.tracking, n.misses, n.tprev = True, 0, T(t)
        n.R, n.t, n.w, n.v = meas[0], meas[1], np.zeros(3, T), np.zeros(3, T)
        n.P = np.zeros((12, 12), T)
        n.P[0:6, 0:6] = meas[2]
        n.P[6:9, 6:9] = np.eye(3, dtype=T) * (T(o["vel0_sigma_rot"]) * T(o["vel0_sigma_rot"]))
        n.P[9:12, 9:12] = np.eye(3, dtype=T) * (T(o["vel0_sigma_trans"]) * T(o["vel0_sigma_trans"]))
        return n, dict(status=OK, flags=FLAG_MEASURED | FLAG_STARTED, full=True, m2=T(0), wt=T(1))
    p = predicted(s, t, o, T)
    flags, wt = 0, T(1)
    if meas is not None:
        flags = FLAG_MEASURED
        Rm, tm, cov = meas
        e, H = observation(p.R, p.t, Rm, tm, T)
        HPH = H @ p.P @ H.T
        Si = sym_inverse(HPH + cov)
        d2 = e @ Si @ e if Si is not None else None
        if Si is None or not np.isfinite(d2):
            return Track(), dict(status=SINGULAR, flags=FLAG_MEASURED, full=False, m2=T(0), wt=T(0))
        gate = T(o["gate"])
        if gate > 0 and d2 > gate * gate:
            flags |= FLAG_GATED
            wt = T(0)
        else:
            _, om = ts.loss(o["loss"], o["loss_scale"], d2)
            C = cov / om
            if om < 1:
                Si = sym_inverse(HPH + C)
                if Si is None:
                    return Track(), dict(status=SINGULAR, flags=FLAG_MEASURED, full=False, m2=T(0), wt=T(0))
                flags |= FLAG_DOWNWEIGHTED
            K = p.P @ H.T @ Si
            delta = -(K @ e)
            A = np.eye(12, dtype=T) - K @ H
            n = p.copy()
            n.R, n.t, n.w, n.v = ts.so3_exp(delta[0:3]) @ p.R, p.t + delta[3:6], p.w + delta[6:9], p.v + delta[9:12]
            n.P = sym_upper(A @ p.P @ A.T + K @ C @ K.T)
            n.misses = 0
            return n, dict(status=OK, flags=flags, full=True, m2=d2, wt=om)
    # rule 5
    if s.misses + 1 >= o["max_gap"]:
        return Track(), dict(status=NOT_TRACKED, flags=flags, full=False, m2=T(0), wt=T(0))
    p.misses = s.misses + 1
    return p, dict(status=OK, flags=flags, full=True, m2=T(0), wt=wt)


def filter_opts(batch):
    """the batch's options over the library's defaults; a batch that names no gate runs without one"""
    o = dict(DEFAULTS, gate=0.0)
    o.update({k: v for k, v in batch.get("opts", {}).items() if k in DEFAULTS})
    return o


def empty_records(nf, nr, T):
    return dict(status=np.full((nf, nr), NOT_TRACKED, np.int32), flags=np.zeros((nf, nr), np.uint32), rvec=np.zeros((nf, nr, 3), T),
                tvec=np.zeros((nf, nr, 3), T), w=np.zeros((nf, nr, 3), T), v=np.zeros((nf, nr, 3), T), cov=np.zeros((nf, nr, 6, 6), T),
                vel_sigma=np.zeros((nf, nr, 6), T), mahalanobis2=np.zeros((nf, nr), T), weight=np.zeros((nf, nr), T))


def put_record(rec, f, g, s, info):
    rec["status"][f, g], rec["flags"][f, g] = info["status"], info["flags"]
    if info["full"]:
        rec["rvec"][f, g], rec["tvec"][f, g], rec["w"][f, g], rec["v"][f, g] = ts.so3_log(s.R), s.t, s.w, s.v
        rec["cov"][f, g] = s.P[0:6, 0:6]
        rec["vel_sigma"][f, g] = np.sqrt(np.diag(s.P)[6:12])
        rec["mahalanobis2"][f, g], rec["weight"][f, g] = info["m2"], info["wt"]


class Filter:
    """the library's filter object: n_rigs tracks, the options, the frame count and the last time"""

    def __init__(self, n_rigs, opts, T=np.float64):
        self.o, self.T, self.n_rigs = dict(DEFAULTS, **opts), T, n_rigs
        self.reset()

    def reset(self):
        self.tracks, self.frames_given, self.last = [Track() for _ in range(self.n_rigs)], 0, None

    def call_times(self, n_frames, times):
        T = self.T
        if times is None:
            return np.array([T(self.frames_given + f) * T(self.o["dt"]) for f in range(n_frames)], T)
        return np.asarray(times, T)

    def run(self, batch, times=None):
        """one step call on the frames of `batch` (its own times and opts are not read) -> records [n_frames, n_rigs]"""
        T, nf, nr = self.T, batch["n_frames"], self.n_rigs
        t = self.call_times(nf, times)
        assert self.last is None or t[0] > self.last
        rec = empty_records(nf, nr, T)
        for g in range(nr):
            if ts.bad_input(batch, g):
                rec["status"][:, g] = BAD_INPUT
                continue
            s = self.tracks[g]
            for f in range(nf):
                m = ts.measurement(batch, f, g, T)
                if m is not None:  # cov_f itself, from its upper triangle
                    m = (m[0], m[1], sym_upper(np.asarray(batch["cov"][f, g], T)))
                s, info = step(s, m, t[f], self.o, T)
                put_record(rec, f, g, s, info)
            self.tracks[g] = s
        self.frames_given += nf
        self.last = t[-1]
        return rec

    def predict(self, t):
        """rule 7 -> records [1, n_rigs]"""
        T = self.T
        rec = empty_records(1, self.n_rigs, T)
        for g, s in enumerate(self.tracks):
            if s.tracking:
                put_record(rec, 0, g, predicted(s, T(t), self.o, T), dict(status=OK, flags=0, full=True, m2=T(0), wt=T(1)))
        return rec


def run_batch(batch, T=np.float64):
    """the whole batch in one call on a fresh filter"""
    return Filter(batch["n_rigs"], filter_opts(batch), T).run(batch, batch.get("times"))


def frames_slice(batch, a, b):
    """frames a .. b-1 of a batch as a call of their own (the records' frame fields count within the call)"""
    c = dict(batch, n_frames=b - a)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov", "rec_rig"):
        c[k] = batch[k][a:b]
    c["rec_frame"] = batch["rec_frame"][a:b] - a
    return c


def deviation(got, want):
    """track_statement.deviation's figures; a gated frame's weight is exactly 0 in both (relative deviation has no meaning there)"""
    gw, ww = np.array(got["weight"], copy=True), np.array(want["weight"], copy=True)
    assert ((gw == 0) == (ww == 0)).all()
    gw[gw == 0] = 1
    ww[ww == 0] = 1
    d = ts.deviation(dict(got, weight=gw), dict(want, weight=ww))
    d.pop("cost", None)
    return d
