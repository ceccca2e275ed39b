"""An independent statement of the robust refit (k_pose_robust.hip; include/ctag_pose.h, robust refit, rules 1-7), in numpy only.

Nothing here comes from oracle/, cylindertag_amd/csrc or testkit.  The points of a source record (rule 2), the residuals and their
Jacobian (rule 3) are cov_statement.py's, which holds them against pose_statement.py and mv_statement.py; the scale, the two losses
and the loop are stated here.

  rows             residuals and Jacobian rows of every point, in point order
  scale_of         rule 4: the lower median of the residual norms, sigma_hat, a
  loss             rule 5: rho and rho' of every s_i
  evaluate         one evaluation of the loop: J^T W J and J^T W r of the scaled rows, the cost 0.5 sum rho
  refit            rules 3-7 for one problem: a dict of the record's fields in `ft`, and the loop's trace
  expected_*       the ctag_robust_pose_rec of one source record of each kind
  pose_distance    how far two poses are apart, in pose sigmas per pixel of noise
  check_robust_records   what the records of the device must satisfy

Every step from the observations on runs in the float type `ft`: np.float64, or np.longdouble for the figures the comparison bars come
from.

The comparison bars.  Three figures are MEASURED by tests/test_robust_statement_cpu.py over every record of tests/robust_shapes.py and
written here; the test measures them again and holds them against these constants.
  EVAL   the worst relative deviation of float64 from longdouble in sigma_hat, scale_px, cost0, cost_ls0, cost, cost_ls and
         max_residual_px, with max_iterations = 0
  LOOP   the worst distance of the float64 loop's final pose from the longdouble loop's: max_k |dx_k| / sqrt((H^-1)_kk), H = J^T W J at
         the longdouble end
  STOP   the same distance between the float64 loop's end and scipy's minimum of rule 5's objective polished from that end: how far
         the stop rules themselves leave the loop from the minimum
A device that sums in another order moves rounding by a small multiple: evaluated fields are held to 16 x EVAL, final poses to
16 x max(LOOP, STOP)."""
import numpy as np

import cov_statement as cs

ROBUST_OK, ROBUST_NO_POSE, ROBUST_BAD_RECORD, ROBUST_DEGENERATE = 0, 1, 2, 3
HUBER, CAUCHY = 0, 1
RAYLEIGH_MEDIAN = "1.1774100225154747"  # sqrt(2 ln 2), as the header writes it
MAX_ITERATIONS = 50
MASK_WORDS = 25
ROBUST_POSE_DT = np.dtype([("status", "<i4"), ("n_points", "<i4"), ("n_inliers", "<i4"), ("iterations", "<i4"), ("loss", "<i4"), ("worst_point", "<i4"),
                           ("inlier_mask", "<u4", (MASK_WORDS,)), ("reserved", "<i4"), ("scale_px", "<f8"), ("sigma_hat", "<f8"), ("cost_ls0", "<f8"),
                           ("cost_ls", "<f8"), ("cost0", "<f8"), ("cost", "<f8"), ("max_residual_px", "<f8"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert ROBUST_POSE_DT.itemsize == 232
EVAL_FIELDS = ("sigma_hat", "scale_px", "cost0", "cost_ls0", "cost", "cost_ls", "max_residual_px")
INT_FIELDS = ("n_points", "n_inliers", "loss", "worst_point", "reserved")  # and iterations, where max_iterations ends the loop

EVAL = 5e-9    # measured 4.16e-09, on a noise-free record: residuals of 3e-5 px are differences of pixel coordinates near 1000
LOOP = 4e-7    # measured 3.58e-07, on the two-camera record of 16 points
STOP = 1.2e-7  # measured 1.12e-07, on an eight-camera record
EVAL_BAR = 16 * EVAL
POSE_BAR = 16 * max(LOOP, STOP)
THRESHOLD_MARGIN = 1e-6  # no s_i of any shape lies within this fraction of a^2 of the inlier threshold


def default_opts(loss=CAUCHY, max_iterations=MAX_ITERATIONS, scale_px=0.0, auto_k=2.5, min_scale_px=0.05):
    return {"loss": loss, "max_iterations": max_iterations, "scale_px": scale_px, "auto_k": auto_k, "min_scale_px": min_scale_px}


def opts_ok(o):
    """Rule 9."""
    if o["loss"] not in (HUBER, CAUCHY) or not 0 <= o["max_iterations"] <= MAX_ITERATIONS:
        return False
    if not all(np.isfinite(o[k]) for k in ("scale_px", "auto_k", "min_scale_px")):
        return False
    return o["scale_px"] > 0 or (o["auto_k"] > 0 and o["min_scale_px"] > 0)


# ---- rules 3-5 -------------------------------------------------------------------------------------------------------------------

def rows(pparts, x, ft=np.float64):
    """(ru [n], rv [n], Ju [n,6], Jv [n,6]) in point order at the pose x = (rvec, tvec); the unknowns are the record's own coordinates."""
    r, J, _ = cs.residual_jacobian(pparts, x[:3], x[3:], cs.RVEC, ft)
    ru, rv, Ju, Jv, at = [], [], [], [], 0
    for _, X, _ in pparts:
        m = len(X)
        ru.append(r[at:at + m])
        rv.append(r[at + m:at + 2 * m])
        Ju.append(J[at:at + m])
        Jv.append(J[at + m:at + 2 * m])
        at += 2 * m
    return np.concatenate(ru), np.concatenate(rv), np.concatenate(Ju), np.concatenate(Jv)


PLANTS = ("scaled cost", "upper median", "scale in the loop", "strict inlier", "huber without offset", "unweighted jacobian")


def scale_of(norms, opts, ft=np.float64, plant=()):
    """Rule 4: (sigma_hat, a).  The lower median is one value of the array: rank (n - 1) // 2 in ascending order."""
    m = np.sort(norms)[len(norms) // 2 if "upper median" in plant else (len(norms) - 1) // 2]
    sigma_hat = m / ft(RAYLEIGH_MEDIAN)
    if opts["scale_px"] > 0:
        return sigma_hat, ft(opts["scale_px"])
    a = ft(opts["auto_k"]) * sigma_hat
    floor = ft(opts["min_scale_px"])
    return sigma_hat, a if a > floor else floor


def loss(s, a, kind, ft=np.float64, plant=()):
    """Rule 5: (rho(s), rho'(s)), Ceres 2.0's HuberLoss and CauchyLoss on the squared norm s of a block."""
    a2 = a * a
    if kind == HUBER:
        out = s > a2
        q = np.sqrt(np.where(out, s, ft(1)))
        return np.where(out, 2 * a * q - (0 if "huber without offset" in plant else a2), s), np.where(out, a / q, ft(1))
    q = ft(1) + s / a2
    return a2 * np.log(q), ft(1) / q


def evaluate(pparts, x, a, kind, scale, ft=np.float64, plant=()):
    """One evaluation: (H, g, cost, s).  Both losses have rho'' <= 0, so Ceres' corrector scales a point's two residuals and two
    Jacobian rows by sqrt(rho'(s_i)); the columns are scaled by `scale` on top.  cost = 0.5 sum rho(s_i)."""
    ru, rv, Ju, Jv = rows(pparts, x, ft)
    s = ru * ru + rv * rv
    rho, w = loss(s, a, kind, ft, plant)
    sw = np.sqrt(w)
    jw = np.ones_like(sw) if "unweighted jacobian" in plant else sw
    Ju, Jv = Ju * jw[:, None] * scale[None, :], Jv * jw[:, None] * scale[None, :]
    H = Ju.T @ Ju + Jv.T @ Jv
    g = Ju.T @ (ru * sw) + Jv.T @ (rv * sw)
    return H, g, ft(0.5) * ((w * s).sum() if "scaled cost" in plant else rho.sum()), s


def _chol_solve(A, b, ft):
    """x of A x = b by Cholesky, or None when a pivot is not positive."""
    n = len(b)
    Lm = np.zeros((n, n), ft)
    for j in range(n):
        d = A[j, j] - Lm[j, :j] @ Lm[j, :j]
        if not d > 0:
            return None
        Lm[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            Lm[i, j] = (A[i, j] - Lm[i, :j] @ Lm[j, :j]) / Lm[j, j]
    y = np.zeros(n, ft)
    for i in range(n):
        y[i] = (b[i] - Lm[i, :i] @ y[:i]) / Lm[i, i]
    x = np.zeros(n, ft)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - Lm[i + 1:, i] @ x[i + 1:]) / Lm[i, i]
    return x


# ---- rules 6 and 7 ---------------------------------------------------------------------------------------------------------------

def refit(pparts, rvec, tvec, opts, ft=np.float64, plant=()):
    """Rules 3-7 for one problem from the pose (rvec, tvec): a dict of the record's fields in `ft` ("status" alone unless it is
    ROBUST_OK), with "trace" = {"accepted", "rejected", "stop"}, "s" (the s_i at the final pose) and "threshold_gap" (the smallest
    |s_i / a^2 - 1|) on top.  plant: names of PLANTS, the errors the checker's own test plants."""
    with np.errstate(all="ignore"):
        x = np.concatenate([np.asarray(rvec, ft), np.asarray(tvec, ft)])
        kind = opts["loss"]
        one = np.ones(6, ft)
        ru, rv, _, _ = rows(pparts, x, ft)
        s = ru * ru + rv * rv
        n = len(s)
        sigma_hat, a = scale_of(np.sqrt(s), opts, ft, plant)
        cost_ls0 = ft(0.5) * s.sum()
        H, g, cost, _ = evaluate(pparts, x, a, kind, one, ft, plant)
        cost0 = cost
        if not np.isfinite(cost0):
            return {"status": ROBUST_DEGENERATE}
        # PoseBA's loop (Ceres' TrustRegionMinimizer with the Levenberg-Marquardt strategy), as ctag_pose_dev.h's pose_ba states it
        scale = ft(1) / (ft(1) + np.sqrt(np.diag(H)))
        H, g = H * np.outer(scale, scale), g * scale
        trace = {"accepted": 0, "rejected": 0, "stop": "gradient", "least_change": np.inf, "step_ratio": np.inf}
        live = np.abs(g / scale).max() > 1e-15
        radius, decrease, it = ft(1e4), ft(2), 0
        if live:
            trace["stop"] = "cap"
        while live and it < opts["max_iterations"]:
            it += 1
            if radius < 1e-32:
                trace["stop"] = "radius"
                break
            A = H + np.diag(np.clip(np.diag(H), ft(1e-6), ft(1e32)) / radius)
            delta = _chol_solve(A, -g, ft)
            change = -(delta @ g + ft(0.5) * (delta @ (H @ delta))) if delta is not None else ft(0)
            if delta is None or not np.all(np.isfinite(delta)) or not change > 0:
                radius, decrease = radius / decrease, decrease * 2
                trace["rejected"] += 1
                continue
            du = delta * scale
            xc = x + du
            if "scale in the loop" in plant:
                rcu, rcv, _, _ = rows(pparts, xc, ft)
                a = scale_of(np.sqrt(rcu * rcu + rcv * rcv), opts, ft)[1]
            Hc, gc, cost_c, _ = evaluate(pparts, xc, a, kind, scale, ft, plant)
            finite = bool(np.isfinite(cost_c))
            step_ratio = float(np.sqrt(du @ du) / (ft(1e-10) * (np.sqrt(x @ x) + ft(1e-10))))
            if step_ratio <= 1:
                trace["stop"], trace["step_ratio"] = "step", step_ratio
                break
            cost_change = cost - cost_c
            trace["least_change"] = min(trace["least_change"], float(abs(cost_change) / cost), abs(np.log(step_ratio)))
            if finite and abs(cost_change) <= ft(1e-15) * cost:
                trace["stop"] = "cost"
                break
            rho = cost_change / change
            if finite and rho > 1e-3:
                x, H, g, cost = xc, Hc, gc, cost_c
                trace["accepted"] += 1
                t = 2 * rho - 1
                radius = min(radius / max(1 - t * t * t, ft(1) / 3), ft(1e16))
                decrease = ft(2)
                if np.abs(g / scale).max() <= 1e-15:
                    trace["stop"] = "gradient"
                    break
            else:
                radius, decrease = radius / decrease, decrease * 2
                trace["rejected"] += 1
        if trace["accepted"]:
            ru, rv, _, _ = rows(pparts, x, ft)
            s = ru * ru + rv * rv
        norms = np.sqrt(s)
        worst = int(np.argmax(norms))  # the first of equal maxima
        inlier = s < a * a if "strict inlier" in plant else s <= a * a
        mask = np.zeros(MASK_WORDS, np.uint32)
        for i in np.nonzero(inlier)[0]:
            mask[i >> 5] |= np.uint32(1 << (int(i) & 31))
        return {"status": ROBUST_OK, "n_points": n, "n_inliers": int(inlier.sum()), "iterations": it, "loss": kind, "worst_point": worst,
                "inlier_mask": mask, "reserved": 0, "scale_px": a, "sigma_hat": sigma_hat, "cost_ls0": cost_ls0, "cost_ls": ft(0.5) * s.sum(),
                "cost0": cost0, "cost": cost, "max_residual_px": norms[worst], "rvec": x[:3], "tvec": x[3:], "trace": trace, "s": s,
                "threshold_gap": float(np.abs(s / (a * a) - 1).min())}


def hessian_at(pparts, x, a, kind, ft=np.longdouble):
    """J^T W J at the pose x in the record's own coordinates, unscaled: the matrix pose distances are measured in."""
    return evaluate(pparts, np.asarray(x, ft), a, kind, np.ones(6, ft), ft)[0]


def pose_distance(xa, xb, H):
    """max_k |xa_k - xb_k| / sqrt((H^-1)_kk): pose sigmas per pixel of noise."""
    Hi = np.linalg.inv(np.asarray(H, np.float64))
    d = np.asarray(xa, np.longdouble) - np.asarray(xb, np.longdouble)
    return float((np.abs(d) / np.sqrt(np.diag(Hi))).max())


def pose_of(e):
    return np.concatenate([np.asarray(e["rvec"], np.longdouble), np.asarray(e["tvec"], np.longdouble)])


# ---- rules 1 and 2 ---------------------------------------------------------------------------------------------------------------

def expected(P, parts, cameras, camera_poses, opts, ft=np.float64, plant=()):
    """The fields of the robust record of source record P whose rebuilt points are `parts` (None: rule 2 failed)."""
    if int(P["status"]) != 0:
        return {"status": ROBUST_NO_POSE}
    if parts is None:
        return {"status": ROBUST_BAD_RECORD}
    return refit(cs.problem_parts(parts, cameras, camera_poses, ft), P["rvec"], P["tvec"], opts, ft, plant)


def parts_of(case, P):
    """Rule 2 through cov_statement's walk for a case of tests/cov_shapes.py's form."""
    if int(P["status"]) != 0:
        return None
    if case["kind"] == "marker":
        return cs.parts_of_marker(P, case["recs"], case["model"])
    if case["kind"] == "rig":
        return cs.parts_of_rig(P, case["recs"], case["model"])
    return cs.parts_of_mv(P, case["recs"], case["model"])


def expected_of(case, opts, ft=np.float64, plant=()):
    """The statement's dicts for every source record of a case."""
    return [expected(P, parts_of(case, P), case["cameras"], case["camera_poses"], opts, ft, plant) for P in case["sources"]]


def to_record(e):
    """The dict of expected() as a ROBUST_POSE_DT record (rule 1: zero but for the status unless it is ROBUST_OK)."""
    R = np.zeros((), ROBUST_POSE_DT)
    for k in ROBUST_POSE_DT.names:
        if k in e:
            R[k] = np.asarray(e[k], np.float64) if ROBUST_POSE_DT[k].base.kind == "f" else e[k]
    return R


# ---- comparison ------------------------------------------------------------------------------------------------------------------

def eval_deviation(a, b, fields=EVAL_FIELDS):
    """The largest relative difference of the evaluated fields of two ROBUST_OK records / dicts; b is the reference."""
    worst = 0.0
    for k in fields:
        va, vb = np.longdouble(a[k]), np.longdouble(b[k])
        if vb != 0 or va != 0:
            worst = max(worst, float(abs(va - vb) / abs(vb)))
    return worst


def check_robust_records(got, want, sources, pparts_of=None, eval_bar=None, pose_bar=None, what=""):
    """Asserts that the device's records `got` are the statement's `want` (dicts of expected(), float64) for the source records
    `sources`: status equal; every status but ROBUST_OK: all other bytes zero; ROBUST_OK: n_points, n_inliers, loss, worst_point, reserved
    and the mask equal, n_inliers the mask's count, sigma_hat, scale_px, cost0 and cost_ls0 within eval_bar; iterations equal where
    max_iterations ended the statement's loop (trace stop "cap"), and within 1 .. MAX_ITERATIONS where its own rules did (the
    acceptance of such a loop's last steps is decided by the rounding of the cost: tests/test_robust_statement_cpu.py).  A record whose loop accepted no step: rvec, tvec are the
    source's bytes, and cost, cost_ls, max_residual_px lie within eval_bar too.  One that moved: its pose lies within pose_bar of the
    statement's (pose_distance under J^T W J of pparts_of(w) at the statement's end), and its cost, cost_ls and max_residual_px within
    eval_bar of the statement's evaluation AT THE RECORD'S OWN POSE (they are evaluated fields of that pose).
    Returns (worst evaluated deviation, worst pose distance)."""
    eval_bar = EVAL_BAR if eval_bar is None else eval_bar
    pose_bar = POSE_BAR if pose_bar is None else pose_bar
    assert len(got) == len(want) == len(sources), (what, len(got), len(want), len(sources))
    worst_e = worst_p = 0.0
    for w, (G, E, P) in enumerate(zip(got, want, sources)):
        at = "%s record %d" % (what, w)
        assert int(G["status"]) == E["status"], (at, "status", int(G["status"]), E["status"])
        if E["status"] != ROBUST_OK:
            assert G.tobytes()[4:] == bytes(ROBUST_POSE_DT.itemsize - 4), (at, "fields set on status %d" % E["status"])
            continue
        for k in INT_FIELDS:
            assert int(G[k]) == int(E[k]), (at, k, int(G[k]), int(E[k]))
        assert np.array_equal(G["inlier_mask"], E["inlier_mask"]), (at, "inlier_mask")
        if E["trace"]["stop"] == "cap":
            assert int(G["iterations"]) == E["iterations"], (at, "iterations", int(G["iterations"]), E["iterations"])
        else:
            assert 1 <= int(G["iterations"]) <= MAX_ITERATIONS, (at, "iterations", int(G["iterations"]))
        assert int(G["n_inliers"]) == sum(bin(int(v)).count("1") for v in G["inlier_mask"]), (at, "n_inliers is not the mask's count")
        d = eval_deviation(G, E, ("sigma_hat", "scale_px", "cost0", "cost_ls0"))
        assert d <= eval_bar, (at, "evaluated fields", d, eval_bar)
        worst_e = max(worst_e, d)
        if E["trace"]["accepted"] == 0:
            assert G["rvec"].tobytes() == np.asarray(P["rvec"], np.float64).tobytes() and G["tvec"].tobytes() == np.asarray(P["tvec"], np.float64).tobytes(), (at, "pose moved")
            there = E
        else:
            pp = pparts_of(w)
            H = hessian_at(pp, pose_of(E), np.longdouble(E["scale_px"]), E["loss"])
            dp = pose_distance(np.concatenate([G["rvec"], G["tvec"]]), pose_of(E), H)
            assert dp <= pose_bar, (at, "pose", dp, pose_bar)
            worst_p = max(worst_p, dp)
            e0 = refit(pp, G["rvec"], G["tvec"], default_opts(loss=E["loss"], max_iterations=0, scale_px=float(E["scale_px"])))
            assert e0["status"] == ROBUST_OK, at
            there = {"cost": e0["cost0"], "cost_ls": e0["cost_ls0"], "max_residual_px": e0["max_residual_px"]}
        d = eval_deviation(G, there, ("cost", "cost_ls", "max_residual_px"))
        assert d <= eval_bar, (at, "fields of the final pose", d, eval_bar)
        worst_e = max(worst_e, d)
    return worst_e, worst_p
