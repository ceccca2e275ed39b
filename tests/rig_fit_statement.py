"""An independent statement of the rig assembly (include/ctag_pose.h, rig assembly, rules 1-7), in numpy / scipy only.  Nothing here
comes from oracle/, cylindertag_amd/csrc or testkit; the correspondences, the undistortion and the float32 observations are
pose_statement's, the rig membership is rig_statement's, the residual of many records at once and the dense helpers are
model_fit_statement's.  What is stated:

  counted_markers    rule 1: which marker of a frame counts for which model
  marker_poses       every counted marker's pose under the input model: Gauss-Newton from a given start (EPnP and the Ceres loop are
                     NOT restated: check what they must reach)
  initial_assembly   rule 2: co-visibility counts, anchor, tree, edge transforms
  layout             rule 3: the transforms applied to the input corners
  rig_observations   rule 4: the (frame, rig) items that take part, each as (flat corner ids, observations)
  reduced_system     S = sum (Q Jm)^T (Q Jm), g = sum (Q Jm)^T r with Q = I - Jp (Jp^T Jp)^-1 Jp^T from central differences of the
                     statement's own residual, in any floating-point type
  step               (S + lambda diag S) delta = -g with the anchor's rows dropped
  fit                the Levenberg-Marquardt loop of rule 5 in double
  joint_minimum      scipy.optimize.least_squares over the member transforms AND the rig poses together

The bars the device is held to are the constants at the end; tests/test_rig_fit_statement_cpu.py measures them again on every run,
DESIGN.md section 16 says where each came from."""
import numpy as np
from scipy import sparse
from scipy.optimize import least_squares

import model_fit_statement as ms
import pose_statement as ps
import rig_statement as rs

OK, NOT_SEEN = 0, 5
MAX_MODELS = 16   # CTAG_RIG_FIT_MAX_MODELS


def rot(rv, dtype=np.float64):
    return ms._rot(np.asarray(rv, dtype).reshape(1, 3))[0]


def rvec_of(R):
    return ms._rvec_of(np.asarray(R, np.float64)[None])[0]


# ---------------------------------------------------------------------------------------------------------------------
# rule 1
# ---------------------------------------------------------------------------------------------------------------------
def counted_markers(recs, model, ok_of=None):
    """Per frame {model index: marker index} of the markers whose pose counts: the frame is CTAG_OK, the marker is the first of the
    frame with its model index and its pose record is CTAG_POSE_OK (ok_of(frame, marker); None: whenever the builder gives at least
    4 points)."""
    out = []
    for f, rec in enumerate(recs):
        d, claimed = {}, set()
        for k in range(ps.marker_count(rec)):
            st, mi = ps.expected_record(rec, k, model)[:2]
            if mi < 0 or mi in claimed:
                continue
            claimed.add(mi)
            if st == ps.OK and (ok_of is None or ok_of(f, k)):
                d[mi] = k
        out.append(d)
    return out


def marker_poses(recs, model, camera, counted, start_of):
    """{(frame, model index): pose [6]} of every counted marker under `model`, solved from start_of(frame, marker, model index);
    plus {(frame, model index): cost}."""
    obs = [o if o is not None and counted[o["frame"]].get(o["model"]) == o["marker"] else None for o in ms.observations(recs, model, camera)]
    poses, costs = {}, {}
    for m in range(len(model["ids"])):
        B = ms.Batch(obs, m, camera)
        if not B.recs:
            continue
        X = np.asarray(model["corners"][m], np.float64)
        p = ms.solve_poses(B, X, np.array([start_of(o["frame"], o["marker"], m) for o in B.recs]))
        c = B.costs(X, p)
        for o, pi, ci in zip(B.recs, p, c):
            poses[(o["frame"], m)], costs[(o["frame"], m)] = pi, float(ci)
    return poses, costs


# ---------------------------------------------------------------------------------------------------------------------
# rule 2
# ---------------------------------------------------------------------------------------------------------------------
def covisibility(poses, n_frames, members):
    seen = np.array([[(f, m) in poses for m in members] for f in range(n_frames)], np.int64).reshape(n_frames, len(members))
    cnt = seen.T @ seen
    np.fill_diagonal(cnt, 0)
    return cnt


def initial_assembly(poses, n_frames, members, min_frames=2, wrong=None):
    """Rule 2 for one rig (members: its model indices, ascending).  Returns dict(anchor (-1: none), placed [model indices, ascending],
    parent {model: model}, n_with_parent {model: frames}, T {model: (R, t)}).  wrong="edge direction": a planted error for the
    statement's own tests, the edge transform averaged the other way round."""
    members = list(members)
    cnt = covisibility(poses, n_frames, members)
    out = {"anchor": -1, "placed": [], "parent": {}, "n_with_parent": {}, "T": {}, "counts": cnt}
    ok = [a for a in range(len(members)) if len(members) > 1 and cnt[a].max() >= min_frames]
    if not ok:
        return out
    a0 = ok[0]
    out["anchor"] = members[a0]
    placed = [a0]
    out["T"][members[a0]] = (np.eye(3), np.zeros(3))
    while True:
        best = None
        for b in range(len(members)):
            if b in placed:
                continue
            for a in sorted(placed):
                if cnt[a, b] >= min_frames and (best is None or cnt[a, b] > best[0]):
                    best = (cnt[a, b], a, b)
        if best is None:
            break
        n, a, b = best
        ma, mb = members[a], members[b]
        sR, st = np.zeros((3, 3)), np.zeros(3)
        for f in range(n_frames):
            if (f, ma) in poses and (f, mb) in poses:
                pa, pb = poses[(f, ma)], poses[(f, mb)]
                Ra, Rb = rot(pa[:3]), rot(pb[:3])
                if wrong == "edge direction":
                    sR += Rb.T @ Ra
                    st += Rb.T @ (pa[3:] - pb[3:])
                else:
                    sR += Ra.T @ Rb
                    st += Ra.T @ (pb[3:] - pa[3:])
        U, _, Vt = np.linalg.svd(sR)
        E = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
        Ta = out["T"][ma]
        out["T"][mb] = (Ta[0] @ E, Ta[0] @ (st / n) + Ta[1])
        out["parent"][mb], out["n_with_parent"][mb] = ma, int(n)
        placed.append(b)
    out["placed"] = sorted(members[a] for a in placed)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rule 3
# ---------------------------------------------------------------------------------------------------------------------
def layout(corners_in, T, round_float=True):
    """[n_models, P, 3] float64: the transforms {model: (R, t)} applied to the float32 input corners in double (rounded to float32
    when round_float); a model without a transform, and one whose transform is exactly the identity, keeps its corners."""
    X = np.asarray(corners_in, np.float32).astype(np.float64)
    out = X.copy()
    for m, (R, t) in T.items():
        if (np.asarray(R) == np.eye(3)).all() and not np.asarray(t).any():
            continue
        Y = X[m] @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
        out[m] = Y.astype(np.float32).astype(np.float64) if round_float else Y
    return out


def compose(d, T):
    """Exp(d) o T: R <- Exp(w) R, t <- Exp(w) t + v."""
    E = rot(d[:3])
    return E @ T[0], E @ T[1] + np.asarray(d[3:], np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# rule 4
# ---------------------------------------------------------------------------------------------------------------------
def rig_observations(recs, model, rig_placed, n_rigs, camera, ok_of=None):
    """One entry per (frame, rig) item in item order: dict(w = item, frame, rig, model = rig (for ms.Batch), ids = model index * P +
    corner id per point, obs [n, 2], markers [the member markers]) for the items that take part (two or more members, four or more
    points, ok_of(item) if given: the device's rig pose record is CTAG_POSE_OK), None for the others.  rig_placed: rig_of_model with
    the unplaced models at -1."""
    K, dist = camera
    n, P = len(model["ids"]), int(model["size"]) * 8
    idx = np.zeros((n, P, 3), np.float32)
    idx[:, :, 0] = np.arange(P, dtype=np.float32)
    idx[:, :, 1] = np.arange(n, dtype=np.float32)[:, None]
    im = {"ids": model["ids"], "size": model["size"], "corners": idx}
    out = []
    for f, rec in enumerate(recs):
        for g in range(n_rigs):
            w = f * n_rigs + g
            members, _, obj, img = rs.membership(rec, im, rig_placed, g)
            entry = None
            if len(members) >= 2 and len(obj) >= 4 and (ok_of is None or ok_of(w)):
                mi, c = obj[:, 1].astype(np.int64), obj[:, 0].astype(np.int64)
                entry = {"w": w, "frame": f, "rig": g, "model": g, "ids": mi * P + c, "obs": ps.observations(K, dist, img), "markers": members,
                         "models": sorted(set(mi.tolist()))}
            out.append(entry)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the reduced system: the unknowns of slot s are 6s .. 6s+5 (w, v) of model slots[s]: Y <- Exp(w) Y + v
# ---------------------------------------------------------------------------------------------------------------------
DENSE_RECORDS = 400        # joint_minimum: more records than this take scipy's sparse trust-region solver
TRANSLATION_STEP = 100.0   # central-difference step of a translation, in units of the rotation's (mm against radians at ~600 mm)


def moved(X, delta, slots, P, wrong=None):
    """The flat corner list [n_models * P, 3] with Exp(w_s) Y + v_s applied to the corners of model slots[s], in X's type."""
    out = X.copy()
    for s, m in enumerate(slots):
        d = np.asarray(delta[6 * s:6 * s + 6], X.dtype)
        if not d.any():
            continue
        w = -d[:3] if wrong == "cross sign" else d[:3]
        out[m * P:(m + 1) * P] = X[m * P:(m + 1) * P] @ ms._rot(w.reshape(1, 3))[0].T + d[3:]
    return out


def jac_members(batch, X, delta, poses, slots, P, h, wrong=None):
    """[R, n, 2, 6 M]: d residual / d delta at delta, by central differences of step h (rotations) and TRANSLATION_STEP h."""
    T = batch.dtype
    X = np.asarray(X, T)
    poses = np.asarray(poses, T)
    delta = np.asarray(delta, T)
    J = np.zeros(batch.mask.shape + (2, 6 * len(slots)), T)
    for a in range(6 * len(slots)):
        if wrong == "member dropped" and a // 6 == len(slots) - 1:
            continue
        step = h * (T(TRANSLATION_STEP) if a % 6 >= 3 else T(1))
        d = np.zeros(len(delta), T)
        d[a] = step
        J[..., a] = (batch.residual(moved(X, delta + d, slots, P, wrong), poses) - batch.residual(moved(X, delta - d, slots, P, wrong), poses)) / (2 * step)
    return J


def reduced_system(batch, X, poses, slots, P, reverse=False, wrong=None):
    """S [6M, 6M], g [6M] of one rig at (X flat [n_models * P, 3], poses [R, 6]) over ALL its slots (the anchor's included): the sum
    over its records, in record order (reversed: the other way round), of (Q Jm)^T (Q Jm) and (Q Jm)^T r."""
    T = batch.dtype
    h = ms.step_of(T)
    N = 6 * len(slots)
    Jp = batch.jac_pose(X, poses, h)
    Jm = jac_members(batch, X, np.zeros(N, T), poses, slots, P, h, wrong)
    res = batch.residual(X, poses)
    S, g = np.zeros((N, N), T), np.zeros(N, T)
    order = range(len(batch.recs) - 1, -1, -1) if reverse else range(len(batch.recs))
    for r in order:
        n = int(batch.mask[r].sum())
        A = Jp[r, :n].reshape(2 * n, 6)
        B = Jm[r, :n].reshape(2 * n, N)
        M = B - A @ (ms._inv(A.T @ A) @ (A.T @ B))
        S += M.T @ M
        g += M.T @ res[r, :n].reshape(2 * n)
    return S, g


def step(S, g, dropped, lam):
    """(S + lambda diag S) delta = -g without the rows of the dropped slots (0 there).  dropped: [M] bool.  Returns (delta, positive definite?)."""
    return ms.step(S, g, np.repeat(np.asarray(dropped, bool), 2), lam)


# ---------------------------------------------------------------------------------------------------------------------
# the loop of rule 5 and the joint minimum
# ---------------------------------------------------------------------------------------------------------------------
def fit(batch, corners_in, T0, slots, anchor, poses0, max_rounds=30, lambda0=1e-3, lambda_max=1e6, rel_tol=1e-6, round_float=True, wrong=None):
    """Rule 5 for one rig from the state T0 {model: (R, t)}: returns dict(T, X [n_models, P, 3], poses, cost_init, cost, rounds, lam).
    wrong: "cross sign", "keep anchor", "member dropped" -- planted errors for the statement's own tests."""
    P = np.asarray(corners_in).shape[1]
    T = dict(T0)
    dropped = np.array([m == anchor and wrong != "keep anchor" for m in slots])
    X = layout(corners_in, T, round_float)
    poses = ms.solve_poses(batch, X.reshape(-1, 3), poses0)
    cost = cost_init = float(batch.costs(X.reshape(-1, 3), poses).sum())
    lam, rounds = lambda0, 0
    while rounds < max_rounds:
        rounds += 1
        S, g = reduced_system(batch, X.reshape(-1, 3), poses, slots, P, wrong=wrong)
        d, pd = step(S, g, dropped, lam)
        good = False
        if pd:
            Tt = dict(T)
            for s, m in enumerate(slots):
                if d[6 * s:6 * s + 6].any():
                    Tt[m] = compose(d[6 * s:6 * s + 6], T[m])
            Xt = layout(corners_in, Tt, round_float)
            tp = ms.best_poses(batch, Xt.reshape(-1, 3), poses, poses0)
            c = float(batch.costs(Xt.reshape(-1, 3), tp).sum())
            good = c < cost
        if good:
            drop, cost, T, X, poses = cost - c, c, Tt, Xt, tp
            lam = max(lam / 3, 1e-9)
            if drop < rel_tol * cost:
                break
        else:
            lam *= 4
            if lam > lambda_max:
                break
    return {"T": T, "X": X, "poses": poses, "cost_init": cost_init, "cost": cost, "rounds": rounds, "lam": lam}


def joint_minimum(batch, corners_in, T0, slots, anchor, poses0):
    """The minimum over the member transforms AND the rig poses together by scipy.optimize.least_squares from (T0, poses0); the
    anchor's transform stays.  Unknowns: d_m with T_m = Exp(d_m) o T0_m, and the poses.  Returns dict(T, X (double, not rounded), poses, cost)."""
    P = np.asarray(corners_in).shape[1]
    free = [m for m in slots if m != anchor]
    Y0 = layout(corners_in, T0, round_float=False).reshape(-1, 3)
    R, nd = len(batch.recs), 6 * len(free)
    h = ms.step_of(np.float64)
    rr, nn = np.nonzero(batch.mask)
    big = R > DENSE_RECORDS   # the dense Jacobian of batch (f) would take 20 GB

    def fun(v):
        return batch.residual(moved(Y0, v[:nd], free, P), v[nd:].reshape(R, 6))[batch.mask].ravel()

    def jac(v):
        poses = v[nd:].reshape(R, 6)
        X = moved(Y0, v[:nd], free, P)
        Jp = batch.jac_pose(X, poses, h)[rr, nn]
        Jm = jac_members(batch, Y0, v[:nd], poses, free, P, h)[rr, nn]
        rows = 2 * np.arange(len(rr))[:, None, None] + np.arange(2)[None, :, None]
        cols = nd + 6 * rr[:, None, None] + np.arange(6)[None, None, :]
        Jpose = sparse.coo_matrix((Jp.ravel(), (np.broadcast_to(rows, Jp.shape).ravel(), np.broadcast_to(cols, Jp.shape).ravel())),
                                  shape=(2 * len(rr), nd + 6 * R))
        J = sparse.hstack([sparse.csr_matrix(Jm.reshape(2 * len(rr), nd)), Jpose.tocsr()[:, nd:]]).tocsr()
        return J if big else J.toarray()

    poses0 = ms.solve_poses(batch, Y0, poses0)
    v0 = np.concatenate([np.zeros(nd), np.asarray(poses0, np.float64).ravel()])
    sol = least_squares(fun, v0, jac=jac, method="trf", tr_solver="lsmr" if big else "exact", xtol=1e-12, ftol=1e-13, gtol=1e-12, x_scale=1.0,
                        max_nfev=40)
    T = dict(T0)
    for s, m in enumerate(free):
        T[m] = compose(sol.x[6 * s:6 * s + 6], T0[m])
    X = moved(Y0, sol.x[:nd], free, P)
    poses = sol.x[nd:].reshape(R, 6)
    return {"T": T, "X": X.reshape(np.asarray(corners_in).shape), "poses": poses, "cost": float(batch.costs(X, poses).sum())}


def rig_cost(batch, X, poses0):
    """(cost, poses) of a model state X [n_models, P, 3]: every record's pose solved from poses0."""
    p = ms.solve_poses(batch, np.asarray(X, np.float64).reshape(-1, 3), poses0)
    return float(batch.costs(np.asarray(X, np.float64).reshape(-1, 3), p).sum()), p


def system_deviation(S, g, d, S_ref, g_ref, d_ref, cost):
    """ms.system_deviation: S entries over sqrt(S_ii S_jj), g entries over sqrt(S_ii) |r|, delta over its largest entry."""
    return ms.system_deviation(S, g, d, S_ref, g_ref, d_ref, None, cost)


# The float64 statement against the same computation in numpy.longdouble, worst over the shapes batches, AS MEASURED (three digits);
# tests/test_rig_fit_statement_cpu.py::test_measured_bars measures them again on every run and fails when a figure here is off by
# more than 2 %.  The device is allowed 16 x these.
SYSTEM_ERR = {"S": 1.41e-9, "g": 4.44e-10, "delta": 1.31e-8}
SYSTEM_BAR = {k: 16 * v for k, v in SYSTEM_ERR.items()}
F32_SPACING_MM = 600.0 * 2.0 ** -23   # float32 spacing of a coordinate near 600 mm (the shapes' rigs stand there): 7.2e-5 mm
MINIMA_DISTANCE_MM = 2.78e-9            # the distance between two statement minima from different starts, as measured
CORNER_ERR_MM = max(F32_SPACING_MM, MINIMA_DISTANCE_MM)
CORNER_BAR_MM = 16 * CORNER_ERR_MM
REL_TOL_F32 = 6.198e-6                # relative cost change float32 rounding of the model alone causes (0.1 px batches), as measured
