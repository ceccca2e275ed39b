"""The track noise fit of include/ctag_pose.h (track noise fit, rules 1-9) stated independently in numpy, in float64 and in longdouble,
from the header's rules.  Nothing here comes from csrc, oracle or testkit.  `predicted` and `observation` are track_filter_statement.py's,
the measurement, bad input and SO(3) functions track_statement.py's.  The routes differ from the kernel's on purpose: F, H, K and the
Joseph form are dense 12x12 / 6x12 matrices; log det S is numpy.linalg.slogdet of the dense S (in longdouble, where numpy has no
slogdet, the sum of the logarithms of the pivots of a plain elimination of S itself) -- the kernel adds the logarithms of S's diagonal
and of the pivots of the unit-diagonal matrix.

score(batch, theta) is rule 2's L_g for every rig, fit(batch) rules 3-8's grid search.  A batch is track_statement.py's dict; its opts
give the start values q_rot, q_trans and the other ctag_track_noise_opts fields over DEFAULTS.

The bar.  MEASURED_F64_DEVIATION is the worst |L_f64 - L_longdouble| / max(1, n_terms), and the same for sum_m2, over every batch of
track_noise_shapes.BATCHES at the start values and at track_noise_shapes.CANDIDATES, measured on the CPU by
tests/test_track_noise_statement_cpu.py (python -m pytest -s tests/test_track_noise_statement_cpu.py -k deviation prints it; the figures
below are that test's output).  BAR = 16 x the figure, the project's allowance for the same float64 arithmetic in another order."""
import numpy as np

import track_filter_statement as fs
import track_statement as ts

NOISE_OK, NOISE_BAD_INPUT, NOISE_TOO_FEW, NOISE_SINGULAR = 0, 1, 2, 3
FREE_Q_ROT, FREE_Q_TRANS, FREE_COV_SCALE = 1, 2, 4
PER_RIG, POOLED = 0, 1
LN2 = 0.6931471805599453
NAMES = ("q_rot", "q_trans", "cov_scale")

DEFAULTS = dict(mode=PER_RIG, free_mask=7, rounds=10, max_gap=5, min_terms=8, dt=1.0 / 30.0, q_rot=0.1, q_trans=3000.0, cov_scale=1.0,
                vel0_sigma_rot=10.0, vel0_sigma_trans=1000.0, span=16.0)

# python -m pytest -s tests/test_track_noise_statement_cpu.py -k deviation
MEASURED_F64_DEVIATION = {"L": 6.06e-07, "sum_m2": 6.06e-07}
BAR = {k: 16.0 * v for k, v in MEASURED_F64_DEVIATION.items()}


def noise_opts(batch, **over):
    """the batch's options over the defaults: its q are the start values"""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in batch.get("opts", {}).items() if k in DEFAULTS})
    o.update(over)
    return o


def call_times(batch, o, T):
    if batch.get("times") is None:
        return np.array([T(f) * T(o["dt"]) for f in range(batch["n_frames"])], T)
    return np.asarray(batch["times"], T)


def logdet(S):
    """log det of a symmetric positive definite S"""
    if S.dtype == np.float64:
        return np.linalg.slogdet(S)[1]
    A = np.array(S, copy=True)
    s = A.dtype.type(0)
    for j in range(A.shape[0]):
        s += np.log(A[j, j])
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:]) / A[j, j]
    return s


def measurements(batch, g, T=np.float64):
    """rule 1 for every frame of rig g: None (bad input), or a list of None / (Rm, tm, cov_f from its upper triangle, in float64 as the
    record holds it); measured is decided on cov_f itself.  It does not depend on theta: a caller that scores many candidates computes it once."""
    if ts.bad_input(batch, g):
        return None
    out = []
    for f in range(batch["n_frames"]):
        m = ts.measurement(batch, f, g, T)
        out.append(None if m is None else (m[0], m[1], fs.sym_upper(np.asarray(batch["cov"][f, g], np.float64))))
    return out


def score_rig(batch, g, theta, o, T=np.float64, meas=False):
    """rule 2 for rig g at theta = (q_rot, q_trans, s) -> dict(L, sum_m2, n_terms, n_singular, status); meas: measurements(batch, g, T)"""
    zero = T(0)
    if meas is False:
        meas = measurements(batch, g, T)
    if meas is None:
        return dict(L=zero, sum_m2=zero, n_terms=0, n_singular=0, status=NOISE_BAD_INPUT)
    fo = dict(q_rot=T(theta[0]), q_trans=T(theta[1]))
    s = np.float64(theta[2])
    t = call_times(batch, o, T)
    vr2, vt2 = T(o["vel0_sigma_rot"]) * T(o["vel0_sigma_rot"]), T(o["vel0_sigma_trans"]) * T(o["vel0_sigma_trans"])
    I12 = np.eye(12, dtype=T)
    L, m2sum, n_terms, n_sing = zero, zero, 0, 0
    x = fs.Track()
    for f in range(batch["n_frames"]):
        m = meas[f]
        with np.errstate(over="ignore"):   # s * cov_f is a float64 product in either precision: it may overflow, and then rule 4 refuses it
            cov = None if m is None else (s * m[2]).astype(T)
        if not x.tracking:
            if m is None:
                continue
            x = fs.Track()
            x.tracking, x.misses, x.tprev = True, 0, t[f]
            x.R, x.t, x.w, x.v = m[0], m[1], np.zeros(3, T), np.zeros(3, T)
            x.P = np.zeros((12, 12), T)
            x.P[0:6, 0:6] = cov
            x.P[6:9, 6:9] = np.eye(3, dtype=T) * vr2
            x.P[9:12, 9:12] = np.eye(3, dtype=T) * vt2
            continue
        p = fs.predicted(x, t[f], fo, T)
        if m is None:
            if x.misses + 1 >= o["max_gap"]:
                x = fs.Track()
            else:
                p.misses = x.misses + 1
                x = p
            continue
        e, H = fs.observation(p.R, p.t, m[0], m[1], T)
        S = H @ p.P @ H.T + cov
        Si = fs.sym_inverse(np.array(S, copy=True))
        d2 = e @ Si @ e if Si is not None else None
        if Si is None or not np.isfinite(d2):
            n_sing += 1
            x = fs.Track()
            continue
        L = L + (logdet(fs.sym_upper(S)) + d2)
        m2sum = m2sum + d2
        n_terms += 1
        K = p.P @ H.T @ Si
        delta = -(K @ e)
        A = I12 - K @ H
        p.R, p.t, p.w, p.v = ts.so3_exp(delta[0:3]) @ p.R, p.t + delta[3:6], p.w + delta[6:9], p.v + delta[9:12]
        p.P = fs.sym_upper(A @ p.P @ A.T + K @ cov @ K.T)
        p.misses = 0
        x = p
    return dict(L=L, sum_m2=m2sum, n_terms=n_terms, n_singular=n_sing, status=NOISE_OK)


def score(batch, theta, T=np.float64, **over):
    """rule 2 for every rig of the batch -> list of score_rig's dicts"""
    return score_many(batch, [theta], T, **over)[0]


def score_many(batch, thetas, T=np.float64, **over):
    """score at every theta of a list -> list over thetas of lists over rigs"""
    o = noise_opts(batch, **over)
    meas = [measurements(batch, g, T) for g in range(batch["n_rigs"])]
    return [[score_rig(batch, g, th, o, T, meas[g]) for g in range(batch["n_rigs"])] for th in thetas]


def pooled(parts):
    """the sums over the rigs that are not bad input, in rig order"""
    good = [p for p in parts if p["status"] == NOISE_OK]
    if not good:
        return dict(parts[0])
    out = dict(good[0])
    for p in good[1:]:
        out = dict(L=out["L"] + p["L"], sum_m2=out["sum_m2"] + p["sum_m2"], n_terms=out["n_terms"] + p["n_terms"],
                   n_singular=out["n_singular"] + p["n_singular"], status=NOISE_OK)
    return out


# ---- the grid search (rules 3-8) --------------------------------------------------------------------------------------------------------------
def free_axes(mask):
    return [a for a in range(3) if (mask >> a) & 1]


def step_of(o, r):
    return np.float64(o["span"]) / np.float64(2 ** (r + 1))


def grid_u(uc, h, axes):
    """the round's candidates' u, [5 ** n_free, 3]: candidate c has k_j = (c // 5 ** j) % 5 - 2 on the j-th free axis"""
    n = 5 ** len(axes)
    U = np.tile(np.asarray(uc, np.float64), (n, 1))
    for c in range(n):
        for j, a in enumerate(axes):
            U[c, a] = uc[a] + np.float64((c // 5 ** j) % 5 - 2) * h
    return U


def values_of(start, U):
    return np.asarray(start, np.float64) * np.exp(U * LN2)


def winner_of(Ls, sing):
    """the smallest L among the candidates with no singular frame, ties to the lowest index; -1 when there is none"""
    best = -1
    for c in range(len(Ls)):
        if sing[c] == 0 and (best < 0 or Ls[c] < Ls[best]):
            best = c
    return best


def curvature_sigma(Ls, sing, win, h, axes):
    """log2_sigma and the EDGE flags from the last round's grid"""
    sig, flags = np.zeros(3), 0
    for j, a in enumerate(axes):
        k = (win // 5 ** j) % 5
        if k == 0 or k == 4:
            flags |= 1 << a
            continue
        lo, hi = win - 5 ** j, win + 5 ** j
        if sing[lo] or sing[hi]:
            continue
        c = ((Ls[hi] - 2.0 * Ls[win]) + Ls[lo]) / (h * h)
        if c > 0:
            sig[a] = np.sqrt(2.0 / c)
    return sig, flags


def search(batch, rigs, o, T=np.float64, label=-1, scorer=None):
    """one search over the rigs listed -> (record dict, trace rows, the last round's (Ls, sing))"""
    start = np.array([o[k] for k in NAMES], np.float64)
    axes = free_axes(o["free_mask"])
    rec = dict(status=NOISE_OK, rig=label, n_terms=0, n_free=len(axes), rounds=0, flags=0, q_rot=start[0], q_trans=start[1], cov_scale=start[2],
               log2_sigma=np.zeros(3), score=0.0, score_start=0.0, mean_m2=0.0)
    meas = {g: measurements(batch, g, T) for g in rigs}
    good = [g for g in rigs if meas[g] is not None]
    if not good:
        rec["status"] = NOISE_BAD_INPUT
        return rec, [], None
    memo = {}

    def at(v):
        key = tuple(float(x) for x in v)
        if key not in memo:
            memo[key] = scorer(v) if scorer else pooled([score_rig(batch, g, v, o, T, meas[g]) for g in good])
        return memo[key]

    uc, trace, last = np.zeros(3), [], None
    for r in range(o["rounds"]):
        h = step_of(o, r)
        U = grid_u(uc, h, axes)
        V = values_of(start, U)
        res = [at(v) for v in V]
        Ls, sing = [x["L"] for x in res], [x["n_singular"] for x in res]
        rec["rounds"] = r + 1
        if r == 0:
            c0 = res[(len(res) - 1) // 2]
            rec["score_start"] = c0["L"]
            if c0["n_terms"] < o["min_terms"]:
                rec.update(status=NOISE_TOO_FEW, n_terms=c0["n_terms"], score=c0["L"], mean_m2=c0["sum_m2"] / c0["n_terms"] if c0["n_terms"] else 0.0)
                return rec, trace, None
        win = winner_of(Ls, sing)
        if win < 0:
            v = values_of(start, uc[None, :])[0]
            rec.update(status=NOISE_SINGULAR, q_rot=v[0], q_trans=v[1], cov_scale=v[2])
            return rec, trace, None
        trace.append(dict(u=U[win].copy(), value=V[win].copy(), L=Ls[win], winner=win))
        uc, last = U[win].copy(), (Ls, sing, win, h, res[win], V[win])
    Ls, sing, win, h, w, v = last
    sig, flags = curvature_sigma(Ls, sing, win, h, axes)
    rec.update(q_rot=v[0], q_trans=v[1], cov_scale=v[2], n_terms=w["n_terms"], score=w["L"], flags=flags, log2_sigma=sig,
               mean_m2=w["sum_m2"] / w["n_terms"])
    return rec, trace, (Ls, sing)


def fit(batch, T=np.float64, **over):
    """rules 3-8 -> [(record, trace, last grid)]: one entry per rig (PER_RIG) or one with rig -1 (POOLED)"""
    o = noise_opts(batch, **over)
    if o["mode"] == POOLED:
        return [search(batch, list(range(batch["n_rigs"])), o, T, -1)]
    return [search(batch, [g], o, T, g) for g in range(batch["n_rigs"])]
