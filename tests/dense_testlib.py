"""Numpy statement of a dense edge-based pose refinement for the reference's useDensePoseRefine (CylinderTag.cpp:198-209,
PoseEstimator::DenseSolver, an empty stub in pose_estimation.cpp:145-148), and the accuracy study that measured it against
planted poses before any kernel was written (tools/dense_study.py; the numbers and the decision are in docs/history.md,
"Dense pose refinement").

Everything is written out here from the definition: the camera model, the undistortion, the Rodrigues derivative, the edge
search and the IRLS + Levenberg-Marquardt loop.  The corner term's correspondences come from the pose oracle
(tests/pose_testlib.py), which restates pose_estimation.cpp:72-95 on the CPU.  Nothing here is imported by the product package."""
import os

import numpy as np

import testkit as tk
from ctag_testlib import GOLDEN, Oracle, read_marker_file
from pose_testlib import PoseOracle, make_camera, make_model_view, rodrigues

DENSE_OK, DENSE_SKIPPED, DENSE_FEW_SAMPLES, DENSE_REJECTED, DENSE_NOT_FINITE = 0, 1, 2, 3, 4

DEFAULTS = {"samples_per_edge": 8, "search_px": 3.0, "min_contrast": 8.0, "huber_px": 1.0, "dense_weight": 1.0,
            "max_outer": 3, "max_inner": 10, "min_samples": 16}

SIDES = ((0, 3, 1, 2), (1, 2, 0, 3), (5, 6, 4, 7), (4, 7, 5, 6))  # (a, b) of a long side, then the opposite side of its quad


class Cam:
    """K and the 14 distortion terms (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4), float32 values widened to double."""

    def __init__(self, K, dist):
        K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
        self.fx, self.fy, self.cx, self.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        d = np.zeros(14)
        dd = np.asarray(dist, np.float32).astype(np.float64).ravel()
        d[:dd.size] = dd
        self.k = d


def project_full(cam, R, t, X):
    """cv::projectPoints (no tilt) in double; X [n,3] -> [n,2], z <= 0 gives nan."""
    P = X @ R.T + t
    z = P[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = P[:, 0] / z, P[:, 1] / z
    k = cam.k
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    cd = (1 + k[0] * r2 + k[1] * r4 + k[4] * r6) / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6)
    xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r4
    yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r4
    out = np.stack([cam.fx * xd + cam.cx, cam.fy * yd + cam.cy], 1)
    out[~(z > 0)] = np.nan
    return out


def undistort_px(cam, uv):
    """OpenCV's 5 fixed-point iterations (cvUndistortPointsInternal), then through K again: pinhole pixels."""
    k = cam.k
    x0 = (uv[:, 0] - cam.cx) / cam.fx
    y0 = (uv[:, 1] - cam.cy) / cam.fy
    x, y = x0.copy(), y0.copy()
    live = np.ones(x.shape, bool)
    for _ in range(5):
        r2 = x * x + y * y
        ic = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        live &= ic >= 0
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = np.where(live, (x0 - dx) * ic, x0)
        y = np.where(live, (y0 - dy) * ic, y0)
    return np.stack([cam.fx * x + cam.cx, cam.fy * y + cam.cy], 1)


def rot_and_derivs(r):
    """R(r) and dR/dr_k (Gallego & Yezzi 2015, eq. 9); the small-angle limit dR/dr_k = [e_k]x."""
    r = np.asarray(r, np.float64)
    R = rodrigues(r)
    th2 = r @ r

    def hat(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    dR = np.zeros((3, 3, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1
        if th2 < 1e-24:
            dR[k] = hat(e)
        else:
            dR[k] = (r[k] * hat(r) + hat(np.cross(r, (np.eye(3) - R) @ e))) @ R / th2
    return R, dR


def pinhole_and_jac(cam, R, dR, t, X):
    """pi_0 (pinhole, pixels) of X [n,3] and its Jacobian [n,2,6] w.r.t. (rvec, tvec)."""
    P = X @ R.T + t
    iz = 1.0 / P[:, 2]
    u = np.stack([cam.fx * P[:, 0] * iz + cam.cx, cam.fy * P[:, 1] * iz + cam.cy], 1)
    dP = np.zeros((X.shape[0], 3, 6))
    for k in range(3):
        dP[:, :, k] = X @ dR[k].T
    dP[:, :, 3:] = np.eye(3)
    J = np.zeros((X.shape[0], 2, 6))
    J[:, 0] = cam.fx * (dP[:, 0] * iz[:, None] - (P[:, 0] * iz * iz)[:, None] * dP[:, 2])
    J[:, 1] = cam.fy * (dP[:, 1] * iz[:, None] - (P[:, 1] * iz * iz)[:, None] * dP[:, 2])
    return u, J


def record_segments(res, rec, model_corners, model_size):
    """3-D long sides of the record's features: arrays a, b, (opposite a, opposite b) [m,3] in feature / side order."""
    M = res["markers"][rec["marker"]]
    nf = min(int(M["n_features"]), int(M["n_pos"]))
    segs = []
    for j in range(max(nf, 0)):
        pos = int(res["features"][int(M["first_feature"]) + j]["pos"])
        if pos < 0 or pos >= model_size:
            continue
        C = model_corners[pos * 8:pos * 8 + 8].astype(np.float64)
        for a, b, oa, ob in SIDES:
            segs.append((C[a], C[b], C[oa], C[ob]))
    if not segs:
        z = np.zeros((0, 3))
        return z, z, z, z
    s = np.array(segs)
    return s[:, 0], s[:, 1], s[:, 2], s[:, 3]


def bilinear(img, x, y):
    """Bilinear read of u8 img at (x, y), pixel centres at integers; nan outside [0, cols-1] x [0, rows-1]."""
    rows, cols = img.shape
    ok = (x >= 0) & (y >= 0) & (x <= cols - 1) & (y <= rows - 1)
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    x0 = np.minimum(np.floor(xs).astype(np.int64), cols - 2 if cols > 1 else 0)
    y0 = np.minimum(np.floor(ys).astype(np.int64), rows - 2 if rows > 1 else 0)
    fx, fy = xs - x0, ys - y0
    x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
    I = img.astype(np.float64)
    top = (1 - fx) * I[y0, x0] + fx * I[y0, x1]
    bot = (1 - fx) * I[y1, x0] + fx * I[y1, x1]
    return np.where(ok, (1 - fy) * top + fy * bot, np.nan)


def search_edges(img, cam, rvec, tvec, a, b, oa, ob, p):
    """Edge search at pose (rvec, tvec).  Per sample (segment-major): projected point [n,2], unit normal (dark -> bright) [n,2],
    found offset along it [n] (nan when dropped), keep flag [n], the found point undistorted to pinhole pixels [n,2], segment
    index [n]."""
    S = int(p["samples_per_edge"])
    r = float(p["search_px"])
    nt = int(round(4 * r)) + 1
    R = rodrigues(rvec)
    t = np.asarray(tvec, np.float64)
    m = a.shape[0]
    s = (np.arange(S) + 0.5) / S
    seg = np.repeat(np.arange(m), S)
    ss = np.tile(s, m)
    d = b[seg] - a[seg]
    h = 1.0 / 64
    Xs = a[seg] + ss[:, None] * d
    P = project_full(cam, R, t, Xs)
    T = project_full(cam, R, t, Xs + h * d) - project_full(cam, R, t, Xs - h * d)
    Q = project_full(cam, R, t, oa[seg] + ss[:, None] * (ob[seg] - oa[seg]))
    tl = np.hypot(T[:, 0], T[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.stack([-T[:, 1] / tl, T[:, 0] / tl], 1)
    flip = ((P - Q) * n).sum(1) < 0
    n[flip] = -n[flip]
    offs = -r + 0.5 * np.arange(nt)
    xs = P[:, 0:1] + offs[None, :] * n[:, 0:1]
    ys = P[:, 1:2] + offs[None, :] * n[:, 1:2]
    finite = np.isfinite(xs) & np.isfinite(ys)
    prof = bilinear(img, np.where(finite, xs, -1.0), np.where(finite, ys, -1.0))
    inside = np.isfinite(prof).all(1)
    prof = np.where(np.isfinite(prof), prof, 0.0)
    D = 0.5 * (prof[:, 2:] - prof[:, :-2])  # D[:, i] is the difference at tap i+1
    k = np.argmax(D, 1)  # first maximum
    dk = D[np.arange(D.shape[0]), k]
    interior = (k > 0) & (k < D.shape[1] - 1)
    keep = inside & interior & (dk >= float(p["min_contrast"]))
    km, kp = np.maximum(k - 1, 0), np.minimum(k + 1, D.shape[1] - 1)
    dm, dp = D[np.arange(D.shape[0]), km], D[np.arange(D.shape[0]), kp]
    den = dm - 2 * dk + dp
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(den < 0, 0.5 * (dm - dp) / den, 0.0)
    off = -r + 0.5 * (k + 1) + 0.5 * delta
    off = np.where(keep, off, np.nan)
    found = P + np.where(keep, off, 0.0)[:, None] * n
    und = undistort_px(cam, found)
    keep &= np.isfinite(und).all(1)
    return {"point": P, "normal": n, "offset": off, "keep": keep, "found": und, "segment": seg}


def huber_cost(e, delta):
    a = np.abs(e)
    return np.where(a <= delta, e * e, 2 * delta * a - delta * delta)


def _terms(cam, rvec, tvec, Xc, obs, a, b, y, with_j, p):
    """Corner residuals [2n], edge residuals [m] and, with_j, their Jacobians."""
    R, dR = rot_and_derivs(rvec)
    t = np.asarray(tvec, np.float64)
    uc, Jc = pinhole_and_jac(cam, R, dR, t, Xc)
    rc = (uc - obs).ravel()
    ua, Ja = pinhole_and_jac(cam, R, dR, t, a)
    ub, Jb = pinhole_and_jac(cam, R, dR, t, b)
    d = ub - ua
    v = y - ua
    L = np.hypot(d[:, 0], d[:, 1])
    c = d[:, 0] * v[:, 1] - d[:, 1] * v[:, 0]
    e = c / L
    if not with_j:
        return rc, e, None, None
    dd = Jb - Ja
    dv = -Ja
    dc = dd[:, 0] * v[:, 1:2] + d[:, 0:1] * dv[:, 1] - dd[:, 1] * v[:, 0:1] - d[:, 1:2] * dv[:, 0]
    dL = (d[:, 0:1] * dd[:, 0] + d[:, 1:2] * dd[:, 1]) / L[:, None]
    Je = dc / L[:, None] - (c / (L * L))[:, None] * dL
    return rc, e, Jc.reshape(-1, 6), Je


def energy(cam, rvec, tvec, Xc, obs, a, b, y, p):
    rc, e, _, _ = _terms(cam, rvec, tvec, Xc, obs, a, b, y, False, p)
    return (rc * rc).sum() + float(p["dense_weight"]) * huber_cost(e, float(p["huber_px"])).sum(), rc, e


def refine_record(img, cam, res, rec, model_corners, model_size, Xc, obs, params=None):
    """Dense refinement of one pose record.  Xc [n,3] / obs [n,2]: the record's correspondences and PoseBA's observations
    (undistorted, through K, rounded to float).  Returns (rvec, tvec, info dict)."""
    p = dict(DEFAULTS)
    p.update(params or {})
    r0, t0 = np.array(rec["rvec"], np.float64), np.array(rec["tvec"], np.float64)
    info = {"status": DENSE_SKIPPED, "n_samples": 0, "n_kept": 0, "iterations": 0, "corner_rms0": 0.0, "corner_rms": 0.0,
            "edge_rms0": 0.0, "edge_rms": 0.0}
    if rec["status"] != 0:
        return r0, t0, info
    Xc = np.asarray(Xc, np.float32).astype(np.float64)
    obs = np.asarray(obs, np.float32).astype(np.float64)
    a, b, oa, ob = record_segments(res, rec, model_corners, model_size)
    info["n_samples"] = a.shape[0] * int(p["samples_per_edge"])
    delta, w = float(p["huber_px"]), float(p["dense_weight"])
    r, t = r0.copy(), t0.copy()
    iters = 0
    status = DENSE_OK
    sel = None
    for outer in range(int(p["max_outer"])):
        srch = search_edges(img, cam, r, t, a, b, oa, ob, p)
        sel = srch["keep"]
        info["n_kept"] = int(sel.sum())
        if sel.sum() < int(p["min_samples"]):
            status = DENSE_FEW_SAMPLES
            break
        sa, sb, y = a[srch["segment"][sel]], b[srch["segment"][sel]], srch["found"][sel]
        E, _, _ = energy(cam, r, t, Xc, obs, sa, sb, y, p)
        lam = 1e-3
        rs, ts = r.copy(), t.copy()
        for inner in range(int(p["max_inner"])):
            rc, e, Jc, Je = _terms(cam, r, t, Xc, obs, sa, sb, y, True, p)
            ae = np.abs(e)
            wi = w * np.where(ae <= delta, 1.0, delta / np.maximum(ae, delta))
            H = Jc.T @ Jc + (Je * wi[:, None]).T @ Je
            g = Jc.T @ rc + (Je * wi[:, None]).T @ e
            iters += 1
            A = H + lam * np.diag(np.diag(H))
            try:
                step = -np.linalg.solve(A, g)
            except np.linalg.LinAlgError:
                lam *= 10
                continue
            rn, tn = r + step[:3], t + step[3:]
            En, _, _ = energy(cam, rn, tn, Xc, obs, sa, sb, y, p)
            if np.isfinite(En) and En < E:
                r, t, E = rn, tn, En
                lam = max(lam / 10, 1e-12)
                if np.abs(step[:3]).max() < 1e-10 and np.abs(step[3:]).max() < 1e-8 * np.abs(t).max():
                    break
            else:
                lam *= 10
        moved_r, moved_t = np.abs(r - rs).max(), np.abs(t - ts).max()
        if moved_r < 1e-10 and moved_t < 1e-8 * np.abs(t).max():
            break
    info["iterations"] = iters
    if status == DENSE_OK:
        E0, rc0, e0 = energy(cam, r0, t0, Xc, obs, sa, sb, y, p)
        E1, rc1, e1 = energy(cam, r, t, Xc, obs, sa, sb, y, p)
        n = Xc.shape[0]
        info["corner_rms0"] = float(np.sqrt((rc0 * rc0).sum() / n))
        info["corner_rms"] = float(np.sqrt((rc1 * rc1).sum() / n))
        info["edge_rms0"] = float(np.sqrt((e0 * e0).mean()))
        info["edge_rms"] = float(np.sqrt((e1 * e1).mean()))
        if not (np.isfinite(r).all() and np.isfinite(t).all() and np.isfinite(E1)):
            status = DENSE_NOT_FINITE
        elif not (E1 < E0 and info["corner_rms"] <= max(2 * info["corner_rms0"], 1.0)):
            status = DENSE_REJECTED
    info["status"] = status
    if status != DENSE_OK:
        return r0, t0, info
    return r, t, info


def degrade(img, seed, blur_sigma=1.0, noise_sigma=6.0):
    """Gaussian blur (separable, radius 4 sigma, edges replicated) then additive Gaussian noise, rounded and clipped to u8."""
    rad = int(np.ceil(4 * blur_sigma))
    x = np.arange(-rad, rad + 1)
    k = np.exp(-0.5 * (x / blur_sigma) ** 2)
    k /= k.sum()
    f = img.astype(np.float64)
    pad = np.pad(f, ((0, 0), (rad, rad)), mode="edge")
    f = sum(k[i] * pad[:, i:i + f.shape[1]] for i in range(k.size))
    pad = np.pad(f, ((rad, rad), (0, 0)), mode="edge")
    f = sum(k[i] * pad[i:i + f.shape[0], :] for i in range(k.size))
    f += np.random.default_rng(seed).normal(0, noise_sigma, f.shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


# ---- the accuracy study (tools/dense_study.py, docs/history.md): planted poses on ray-cast cylinders
ROWS, COLS = 1080, 1920
K_PLANTED = np.array([[2600.0, 0, 960.0], [0, 2600.0, 540.0], [0, 0, 1]])


def synth_scene():
    state, fs = read_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    _, corners = tk.synth3d_model(state)
    ids = np.arange(state.shape[0], dtype=np.int32)
    model = {"ids": ids, "size": state.shape[1], "base": np.zeros((len(ids), 3), np.float32),
             "axis": np.zeros((len(ids), 3), np.float32), "corners": corners}
    K = K_PLANTED.copy()
    K[0, 2] -= 0.5
    K[1, 2] -= 0.5
    return state, fs, model, K


def pose_errors(r, t, truth, k):
    R, Rt = rodrigues(r), truth["R"][k].reshape(3, 3)
    ang = np.degrees(np.arccos(np.clip((np.trace(R.T @ Rt) - 1) / 2, -1, 1)))
    return ang, np.linalg.norm(np.asarray(t) - truth["t"][k]) / np.linalg.norm(truth["t"][k])


def run(frames, first=0, degraded=False, params=None, seed=1000):
    """[(rot_ba, rel_t_ba, rot_dense, rel_t_dense)] per decoded marker with a PoseBA pose, and the dense statuses."""
    state, fs, model, K = synth_scene()
    orc, po = Oracle(), PoseOracle()
    mv = make_model_view(model)
    cam, dcam = make_camera(K, np.zeros(5)), Cam(K, np.zeros(5))
    errs, statuses = [], []
    for f in range(first, first + frames):
        img, truth = tk.synth3d_frame_host(state, f, K_PLANTED, rows=ROWS, cols=COLS)
        if degraded:
            img = degrade(img, seed + f)
        res = orc.detect_fast(img, state, fs)
        if res["status"] != 0:
            continue
        for p in po.pose_frame(res, mv, cam):
            if p["status"] != 0:
                continue
            ks = [i for i in range(truth["n_markers"]) if truth["dict_row"][i] == model["ids"][p["model_index"]]]
            if not ks:
                continue
            _, obj, im = po.correspondences(res, int(p["marker"]), mv, int(p["model_index"]))
            obs = po.undistort(cam, im, True).astype(np.float32)
            r, t, info = refine_record(img, dcam, res, p, model["corners"][p["model_index"]], model["size"], obj, obs, params)
            errs.append(pose_errors(p["rvec"], p["tvec"], truth, ks[0]) + pose_errors(r, t, truth, ks[0]))
            statuses.append(info["status"])
    return np.array(errs).reshape(-1, 4), np.array(statuses, np.int64)
