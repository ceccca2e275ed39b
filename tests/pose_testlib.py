"""ctypes binding of the pose oracle (test infrastructure) + independent Python readers / camera model used to
check it.  Nothing here is imported by the product package."""
import ctypes as C
import os
import re

import numpy as np

from ctag_testlib import GOLDEN, RESULT_DT, ROOT, build_oracle
from pose_statement import check_pose_records, project12

POSE_DT = np.dtype([("status", "<i4"), ("model_index", "<i4"), ("frame", "<i4"), ("marker", "<i4"),
                    ("n_points", "<i4"), ("iterations", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)),
                    ("rvec0", "<f8", (3,)), ("tvec0", "<f8", (3,)), ("cost0", "<f8"), ("cost", "<f8")])
assert POSE_DT.itemsize == 136
MAX_POINTS = 160


class Camera(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("dist", C.c_float * 14), ("n_dist", C.c_int32)]


class ModelView(C.Structure):
    _fields_ = [("n_models", C.c_int32), ("model_size", C.c_int32), ("marker_id", C.POINTER(C.c_int32)),
                ("base", C.POINTER(C.c_float)), ("axis", C.POINTER(C.c_float)), ("corners", C.POINTER(C.c_float))]


def read_model_file(path):
    """Independent reader of the .model text format (CylinderTag.cpp:161-190): ids, base, axis, corners[n][size*8][3]."""
    t = open(path).read().split()
    n, size = int(t[0]), int(t[1])
    p = 2
    ids = np.zeros(n, np.int32)
    base = np.zeros((n, 3), np.float32)
    axis = np.zeros((n, 3), np.float32)
    corners = np.zeros((n, size * 8, 3), np.float32)
    for i in range(n):
        ids[i] = int(t[p]); p += 1
        base[i] = [np.float32(x) for x in t[p:p + 3]]; p += 3
        axis[i] = [np.float32(x) for x in t[p:p + 3]]; p += 3
        for _ in range(size * 8):
            cid = int(t[p])
            corners[i, cid] = [np.float32(x) for x in t[p + 1:p + 4]]
            p += 4
    return {"ids": ids, "size": size, "base": base, "axis": axis, "corners": corners}


def read_camera_yml(path):
    """Independent reader of the two !!opencv-matrix nodes of cameraParams.yml."""
    txt = open(path).read()
    out = {}
    for name in ("cameraMatrix", "distCoeffs"):
        m = re.search(name + r":\s*!!opencv-matrix\s*rows:\s*(\d+)\s*cols:\s*(\d+)\s*dt:\s*(\w)\s*data:\s*\[([^\]]*)\]", txt)
        vals = [float(x) for x in m.group(4).replace("\n", " ").split(",")]
        out[name] = np.array(vals, np.float32).reshape(int(m.group(1)), int(m.group(2)))
    return out["cameraMatrix"], out["distCoeffs"].ravel()


def make_camera(K, dist):
    c = Camera()
    for i, v in enumerate(np.asarray(K, np.float32).ravel()):
        c.K[i] = float(v)
    d = np.asarray(dist, np.float32).ravel()
    for i in range(14):
        c.dist[i] = float(d[i]) if i < d.size else 0.0
    c.n_dist = int(d.size)
    return c


class _Held:
    pass


def make_model_view(model):
    h = _Held()
    h.ids = np.ascontiguousarray(model["ids"], np.int32)
    h.base = np.ascontiguousarray(model["base"], np.float32)
    h.axis = np.ascontiguousarray(model["axis"], np.float32)
    h.corners = np.ascontiguousarray(model["corners"], np.float32)
    v = ModelView()
    v.n_models = h.ids.size
    v.model_size = int(model["size"])
    v.marker_id = h.ids.ctypes.data_as(C.POINTER(C.c_int32))
    v.base = h.base.ctypes.data_as(C.POINTER(C.c_float))
    v.axis = h.axis.ctypes.data_as(C.POINTER(C.c_float))
    v.corners = h.corners.ctypes.data_as(C.POINTER(C.c_float))
    h.view = v
    return h


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    w = r / th
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * Wx + (1 - np.cos(th)) * np.outer(w, w)


def project(K, dist, rvec, tvec, X, distort=True):
    """cv::projectPoints model (k1 k2 p1 p2 k3), float64."""
    K = np.asarray(K, np.float64)
    d = np.zeros(5)
    dd = np.asarray(dist, np.float64).ravel()
    d[:min(5, dd.size)] = dd[:5]
    P = X @ rodrigues(rvec).T + np.asarray(tvec, np.float64)
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    if distort:
        r2 = x * x + y * y
        rad = 1 + d[0] * r2 + d[1] * r2 ** 2 + d[4] * r2 ** 3
        xd = x * rad + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
        yd = y * rad + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
        x, y = xd, yd
    return np.stack([K[0, 0] * x + K[0, 2], K[1, 1] * y + K[1, 2]], 1)


class PoseOracle:
    def __init__(self, path=None):
        path = path or os.path.join(ROOT, "oracle", "_build", "libctag_pose_oracle.so")
        if not os.path.exists(path):
            build_oracle()
        L = self.L = C.CDLL(path)
        pf, pd = C.POINTER(C.c_float), C.POINTER(C.c_double)
        L.ctago_undistort_points.argtypes = [C.POINTER(Camera), C.c_int, pf, C.c_int, pd]
        L.ctago_undistort_points.restype = None
        L.ctago_solve_pnp_epnp.argtypes = [C.POINTER(Camera), C.c_int, pf, pf, pd, pd]
        L.ctago_pose_ba.argtypes = [C.POINTER(Camera), C.c_int, pf, pf, pd, pd, pd, pd]
        L.ctago_build_correspondences.argtypes = [C.c_void_p, C.c_int, C.POINTER(ModelView), C.c_int, pf, pf,
                                                  C.POINTER(C.c_int)]
        L.ctago_linalg_probe.argtypes = [C.c_int, pd, pd]
        L.ctago_linalg_probe.restype = None
        L.ctago_pose_frame.argtypes = [C.c_void_p, C.POINTER(ModelView), C.POINTER(Camera), C.c_int, C.c_void_p]

    def linalg(self, op, data, n_out):
        data = np.ascontiguousarray(data, np.float64).ravel()
        out = np.zeros(n_out, np.float64)
        self.L.ctago_linalg_probe(op, data.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def undistort(self, cam, uv, with_P):
        uv = np.ascontiguousarray(uv, np.float32)
        out = np.zeros(uv.shape, np.float64)
        self.L.ctago_undistort_points(C.byref(cam), uv.shape[0], uv.ctypes.data_as(C.POINTER(C.c_float)), int(with_P),
                                      out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def epnp(self, cam, obj, img):
        obj = np.ascontiguousarray(obj, np.float32)
        img = np.ascontiguousarray(img, np.float32)
        r, t = np.zeros(3), np.zeros(3)
        st = self.L.ctago_solve_pnp_epnp(C.byref(cam), obj.shape[0], obj.ctypes.data_as(C.POINTER(C.c_float)),
                                         img.ctypes.data_as(C.POINTER(C.c_float)), r.ctypes.data_as(C.POINTER(C.c_double)),
                                         t.ctypes.data_as(C.POINTER(C.c_double)))
        return st, r, t

    def ba(self, cam, obj, img, rvec, tvec):
        obj = np.ascontiguousarray(obj, np.float32)
        img = np.ascontiguousarray(img, np.float32)
        r, t = np.array(rvec, np.float64), np.array(tvec, np.float64)
        c0, c1 = C.c_double(), C.c_double()
        it = self.L.ctago_pose_ba(C.byref(cam), obj.shape[0], obj.ctypes.data_as(C.POINTER(C.c_float)),
                                  img.ctypes.data_as(C.POINTER(C.c_float)), r.ctypes.data_as(C.POINTER(C.c_double)),
                                  t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(c0), C.byref(c1))
        return it, r, t, c0.value, c1.value

    def correspondences(self, res, marker, mv, model_index):
        res = np.ascontiguousarray(res)
        obj = np.zeros((MAX_POINTS, 3), np.float32)
        img = np.zeros((MAX_POINTS, 2), np.float32)
        n = C.c_int()
        st = self.L.ctago_build_correspondences(res.ctypes.data, marker, C.byref(mv.view), model_index,
                                                obj.ctypes.data_as(C.POINTER(C.c_float)),
                                                img.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n))
        return st, obj[:n.value], img[:n.value]

    def pose_frame(self, res, mv, cam, frame_index=0):
        res = np.ascontiguousarray(res)
        out = np.zeros(100, POSE_DT)
        n = self.L.ctago_pose_frame(res.ctypes.data, C.byref(mv.view), C.byref(cam), frame_index, out.ctypes.data)
        return out[:n]


FRAME = (1920, 1200)  # cols, rows of the golden camera's images


def in_frame(pts, frame, margin=2.0):
    return bool((pts[:, 0] >= margin).all() and (pts[:, 0] <= frame[0] - 1 - margin).all() and (pts[:, 1] >= margin).all() and
                (pts[:, 1] <= frame[1] - 1 - margin).all())


def synth_pose_results(model, K, dist, n_frames, seed, noise_px=0.2, max_markers=5, n_features=None, id_pattern=None, inside=None):
    """Detection records (RESULT_DT) whose corners are projections of the model under random poses (+ pixel noise), with
    feature id patterns that exercise every branch of the correspondence builder.  Returns (records, truth) where
    truth[f] is a list of (model_index, rvec, tvec).

    The model may have any size <= 20.  n_features fixes the feature count of every marker (default: 1..7 at random),
    id_pattern = (id_left, id_right) fixes every feature's ids, or one pair per feature of a marker (default: one of eight
    patterns at random).  inside = (cols, rows) draws a marker's pose again until the corners of its features lie inside that
    frame, where the five undistortion iterations have converged and the pose problem has one minimum.  More than five
    distortion coefficients go through pose_statement.project12.  max_markers may be as large as the record's 100 features
    allow.  With the default arguments the records are those of every earlier version (tests/test_pose_statement_cpu.py holds
    their hashes)."""
    rng = np.random.default_rng(seed)
    res = np.zeros(n_frames, RESULT_DT)
    truth = []
    size = model["size"]
    id_patterns = [(3, 3), (3, 4), (2, 4), (1, 4), (5, -1), (0, 0), (6, 7), (7, 4)]
    proj = project if np.asarray(dist).size <= 5 else project12
    for f in range(n_frames):
        nm = int(rng.integers(0, max_markers + 1))
        tf = []
        nfeat = 0
        r = res[f]
        r["status"] = 0
        for m in range(nm):
            nf = int(rng.integers(1, 8)) if n_features is None else int(n_features)
            if nfeat + nf > 100:
                break
            known = rng.random() < 0.85
            mi = int(rng.integers(0, model["ids"].size))
            marker_id = int(model["ids"][mi]) if known else 40  # 40: not in CTag_2f12c.model
            X = model["corners"][mi].astype(np.float64)
            c = X.mean(0)
            while True:
                rv = rng.normal(0, 0.25, 3)
                dt = rng.normal(0, 1, 3) * np.array([40., 30., 60.])
                R = rodrigues(rv)
                tv = c - R @ c + dt
                p0 = int(rng.integers(0, size - nf + 1))
                pts = proj(K, dist, rv, tv, X)
                if inside is None or in_frame(pts[p0 * 8:(p0 + nf) * 8], inside):
                    break
            pts = pts + rng.normal(0, noise_px, (X.shape[0], 2))
            r["markers"][m] = (marker_id, nfeat, nf, nf)
            for j in range(nf):
                F = r["features"][nfeat + j]
                F["pos"] = p0 + j
                if id_pattern is None:
                    il, ir = id_patterns[int(rng.integers(0, len(id_patterns)))]
                else:
                    il, ir = id_pattern if np.ndim(id_pattern) == 1 else id_pattern[j]
                F["id_left"], F["id_right"] = il, ir
                F["id"] = 8 * il + ir if ir >= 0 else -2
                F["corners"] = pts[(p0 + j) * 8:(p0 + j) * 8 + 8].astype(np.float32).ravel()
            nfeat += nf
            tf.append((mi if known else -1, rv, tv))
        r["n_markers"] = len(tf)
        r["n_features"] = nfeat
        truth.append(tf)
    return res, truth


# ---------------------------------------------------------------------------------------------------------------------
# Models, cameras and record batches of tests/test_pose_statement_cpu.py (oracle) and tests/test_pose_forms_gpu.py (device):
# both build the same batches here, so what the statement accepts from the oracle is what it is asked about the kernel.
# ---------------------------------------------------------------------------------------------------------------------
FULL, HALF_MID, HALF_ALONE = (3, 3), (7, 4), (5, -1)  # id pairs: 8 points; 4 points (skipped at a marker's ends); 4 points


def make_cylinder_model(n_models, size):
    """n_models markers of `size` columns (12..20) on a cylinder of radius 40 mm along y, about half a metre in front of the
    camera: float32 corner lists [n_models, size*8, 3], ids 0 .. n_models-1.  A column is 6.4 mm wide and 50 mm tall, about the
    golden model's, so that two columns (16 points) already fix a pose as well as they do there."""
    assert 12 <= size <= 20
    corners = np.zeros((n_models, size * 8, 3), np.float32)
    for m in range(n_models):
        for p in range(size):
            for k in range(8):
                th = (p - (size - 1) / 2.0) * 0.16 + 0.05 * (k % 2) + 0.03 * (k // 2) + 0.01 * m  # no feature's corners in one plane
                y = -24.0 + 16.0 * (k // 2) + 2.0 * (k % 2) + 3.0 * m
                corners[m, p * 8 + k] = (40.0 * np.sin(th), y, 500.0 - 40.0 * np.cos(th))
    return {"ids": np.arange(n_models, dtype=np.int32), "size": size, "base": np.zeros((n_models, 3), np.float32),
            "axis": np.tile(np.float32([0, 1, 0]), (n_models, 1)), "corners": corners}


def _flattened(model, axes, which=None):
    out = dict(model)
    out["corners"] = model["corners"].copy()
    for mi in (range(len(model["ids"])) if which is None else which):
        out["corners"][mi][:, axes] = 0.0
    return out


def planar_model(model, which=None):
    """The same corner lists with z = 0 (all models, or the model indices in `which`)."""
    return _flattened(model, [2], which)


def collinear_model(model, which=None):
    """The same corner lists with y = z = 0."""
    return _flattened(model, [1, 2], which)


def golden_camera_and_model():
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    return K, dist, read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model"))


def test_cameras():
    """name -> distortion coefficients: the six n_dist the pose stage accepts, built up from the golden camera's five, and one
    whose k1 drives icdist negative inside a 1920x1200 frame."""
    base = golden_camera_and_model()[1].astype(np.float32)
    d8 = np.concatenate([base, np.float32([0.8, -3.0, 5.0])])
    d12 = np.concatenate([d8, np.float32([2e-3, -4e-3, 1e-3, 3e-3])])
    return {"n_dist0": np.zeros(0, np.float32), "n_dist4": base[:4].copy(), "n_dist5": base, "n_dist8": d8, "n_dist12": d12,
            "n_dist14": np.concatenate([d12, np.zeros(2, np.float32)]), "icdist": np.float32([-60, 0, 0, 0, 0])}


test_cameras.__test__ = False  # a generator, not a test


def form_model(form):
    """The model list that sends ctag_pose_batch_device down k_pose<96,2> ("small": 12 columns) or k_pose<160,1> ("large")."""
    return golden_camera_and_model()[2] if form == "small" else make_cylinder_model(6, 16)


def place_marker(r, marker_id, pts, size, positions, patterns):
    """Appends one marker whose feature j sits at positions[j] with the id pair patterns[j]; corners from the projected model
    points pts (a position outside the model borrows the corners of position % size)."""
    m, f0 = int(r["n_markers"]), int(r["n_features"])
    assert m < 100 and f0 + len(positions) <= 100
    r["markers"][m] = (marker_id, f0, len(positions), len(positions))
    for j, (pos, (il, ir)) in enumerate(zip(positions, patterns)):
        F = r["features"][f0 + j]
        F["pos"] = pos
        F["id_left"], F["id_right"] = il, ir
        F["id"] = 8 * il + ir if ir >= 0 else -2
        q = pos % size
        F["corners"] = pts[q * 8:q * 8 + 8].astype(np.float32).ravel()
    r["n_markers"] = m + 1
    r["n_features"] = f0 + len(positions)


def random_view(rng, X, K, dist, noise_px, inside=FRAME, used=slice(None)):
    """(rvec, tvec, pixel corners) of model points X under a random pose as synth_pose_results draws them, drawn again until the
    points X[used] project inside the frame `inside` (None: anywhere)."""
    X = X.astype(np.float64)
    c = X.mean(0)
    while True:
        rv = rng.normal(0, 0.25, 3)
        tv = c - rodrigues(rv) @ c + rng.normal(0, 1, 3) * np.array([40., 30., 60.])
        pts = project12(K, dist, rv, tv, X)
        if inside is None or in_frame(pts[used], inside):
            break
    return rv, tv, pts + rng.normal(0, noise_px, pts.shape) if noise_px else pts


def marker_of_points(points, size):
    """(positions, patterns) of a marker with exactly `points` correspondences on a model of `size` columns; points is a
    multiple of 4, at most size*8 + 4 (which repeats a position: one more feature than the model has columns)."""
    full, half = divmod(points, 8)
    half //= 4
    if full == 0:
        return [0], [HALF_ALONE]
    if full > size:
        full, half = size, 1
    positions, patterns = list(range(full)), [FULL] * full
    if half:  # the 4-point feature goes second, where the end-feature rule cannot skip it
        positions.insert(1, full if full < size else 2)
        patterns.insert(1, HALF_MID)
    return positions, patterns


def escape_consistent_view(rng, X, K, dist):
    """random_view for a camera whose undistortion escapes (icdist < 0) over part of the frame, where its forward model has no
    inverse: every point gets the pixel that undistorts back to its own normalised position -- the pinhole pixel where that
    pixel takes the escape (undistortPoints then returns the pinhole coordinates), the forward model's pixel elsewhere.  Poses
    with a point that neither pixel brings back to within 0.05 px (the zone between the two regimes) are drawn again, and so are
    poses where the 0.2 px noise moves a point by more than 2 px after undistortion (it crossed the regime boundary).
    Returns (rvec, tvec, pixels, number of escaping points)."""
    from pose_statement import undistort12
    fx = float(K[0, 0])
    for _ in range(200):
        rv, tv, forward = random_view(rng, X, K, dist, 0, inside=None)
        P = X.astype(np.float64) @ rodrigues(rv).T + tv
        xn = P[:, :2] / P[:, 2:]
        pinhole = project12(K, np.zeros(5), rv, tv, X)
        esc = undistort12(K, dist, pinhole, return_escaped=True)[1]
        pix = np.where(esc[:, None], pinhole, forward)
        if not in_frame(pix, FRAME):
            continue
        noisy = pix + rng.normal(0, 0.2, pix.shape)
        back, esc_noisy = undistort12(K, dist, noisy.astype(np.float32), return_escaped=True)
        if (np.abs(undistort12(K, dist, pix.astype(np.float32)) - xn).max() * fx < 0.05 and np.abs(back - xn).max() * fx < 2.0
                and np.array_equal(esc, esc_noisy)):
            return rv, tv, noisy, int(esc.sum())
    raise AssertionError("no consistent view found")


def camera_batch(name, form):
    """64 frames of up to 12 markers under one of test_cameras(), pixels through that camera's own forward model.  The icdist
    camera's forward model folds the image, so its pixels come from escape_consistent_view: whole markers in the escape region,
    whole markers near the principal point, and markers across both."""
    K, _, _ = golden_camera_and_model()
    dist = test_cameras()[name]
    model = form_model(form)
    seed = 40 + sorted(test_cameras()).index(name) + (100 if form == "large" else 0)
    if name != "icdist":
        recs, _ = synth_pose_results(model, K, dist, 64, seed, max_markers=12, inside=FRAME)
        return {"recs": recs, "model": model, "K": K, "dist": dist, "min_cap": 150}
    rng = np.random.default_rng(seed)
    patterns = [(3, 3), (3, 4), (2, 4), (1, 4), (5, -1), (0, 0), (6, 7), (7, 4)]
    recs = np.zeros(64, RESULT_DT)
    escaping = 0
    for f in range(64):
        for _ in range(int(rng.integers(4, 13))):
            nf = int(rng.integers(1, 8))
            mi = int(rng.integers(0, len(model["ids"])))
            p0 = int(rng.integers(0, model["size"] - nf + 1))
            rv, tv, pts, n_esc = escape_consistent_view(rng, model["corners"][mi][p0 * 8:(p0 + nf) * 8], K, dist)
            escaping += n_esc
            full = np.zeros((model["size"] * 8, 2))
            full[p0 * 8:(p0 + nf) * 8] = pts
            place_marker(recs[f], int(model["ids"][mi]) if rng.random() < 0.85 else 40, full, model["size"], list(range(p0, p0 + nf)),
                         [patterns[int(rng.integers(0, 8))] for _ in range(nf)])
    return {"recs": recs, "model": model, "K": K, "dist": dist, "min_cap": 150, "escaping_points": escaping}


def capacity_batch(size):
    """Noise-free, distortion-free frames whose markers have exactly the point counts at the edges of the two kernel forms:
    size 12 -> 4, 8, 92, 96; larger sizes -> 100, 104, 152, 160 as far as the model has columns, and a marker with a repeated
    position that would have size*8 + 4 points.  Poses are planted."""
    K, _, golden = golden_camera_and_model()
    model = golden if size == 12 else make_cylinder_model(4, size)
    counts = [4, 8, 92, 96] if size == 12 else [c for c in (100, 104, 152, 160) if c <= size * 8] + [size * 8 + 4]
    rng = np.random.default_rng(900 + size)
    n_frames = 6
    recs = np.zeros(n_frames, RESULT_DT)
    planted = []
    for f in range(n_frames):
        tf = []
        for i in range(len(counts)):
            c = counts[(i + f) % len(counts)]
            mi = int(rng.integers(0, len(model["ids"])))
            rv, tv, pts = random_view(rng, model["corners"][mi], K, np.zeros(5), 0, inside=None)
            positions, patterns = marker_of_points(c, size)
            if int(recs[f]["n_features"]) + len(positions) > 100:
                continue
            place_marker(recs[f], int(model["ids"][mi]), pts, size, positions, patterns)
            tf.append((mi, rv, tv))
        planted.append(tf)
    return {"recs": recs, "model": model, "K": K, "dist": np.zeros(5, np.float32), "planted": planted, "counts": counts}


GRID_BLOCKS = 4096          # ctag_pose_batch_device launches min(capacity, 4096) blocks
GRID_KINDS = ("56 points", "4 points", "NO_MODEL", "BAD_POS", "TOO_FEW", "planar DEGENERATE")
GRID_PLANAR = 5             # the model of the list that is made planar


def grid_stride_batch(form):
    """At least 2 * 4096 + 33 work items for one call, so that every block takes a second item and some a third.  Work item w is
    of kind GRID_KINDS[w % 6]; 4096 % 6 = 4, so the items w, w + 4096, w + 8192 of one block are of three different kinds.  The
    first 64 frames are repeated as the last 64 (the frame before them is padded until they start at a multiple of 6)."""
    K, dist, _ = golden_camera_and_model()
    base = form_model(form)
    size = base["size"]
    model = planar_model(base, [GRID_PLANAR])
    rng = np.random.default_rng(77 if form == "small" else 78)
    others = [i for i in range(len(base["ids"])) if i != GRID_PLANAR]
    frames, w = [], 0

    def add_frame(nm):
        nonlocal w
        r = np.zeros((), RESULT_DT)
        for _ in range(nm):
            kind = w % 6
            mi = GRID_PLANAR if kind == 5 else others[int(rng.integers(0, len(others)))]
            nf = (7, 1, 2, 2, 0, 3)[kind]
            p0 = int(rng.integers(0, size - nf + 1))
            _, _, pts = random_view(rng, base["corners"][mi], K, dist, 0.2, used=slice(p0 * 8, (p0 + nf) * 8))
            positions = [size if kind == 3 else p0 + j for j in range(nf)]
            place_marker(r, 40 if kind == 2 else int(base["ids"][mi]), pts, size, positions, [HALF_ALONE if kind == 1 else FULL] * nf)
            w += 1
        frames.append(r)

    while w < 2 * GRID_BLOCKS + 33 - 300:
        add_frame(int(rng.integers(8, 13)))
    add_frame(8 + (-(w + 8)) % 6)
    assert w % 6 == 0
    recs = np.array(frames + frames[:64], RESULT_DT)
    return {"recs": recs, "model": model, "K": K, "dist": dist, "min_cap": 150, "degenerate": lambda f, m, mi: mi == GRID_PLANAR}


def status_batches():
    """name -> batch: a planar and a collinear model list (every posed marker DEGENERATE), and the golden model with NaN corners,
    Inf corners and a marker without features planted in frames 3, 4 and 5."""
    K, dist, model = golden_camera_and_model()
    out = {}
    for name, flat in (("planar", planar_model(model)), ("collinear", collinear_model(model))):
        recs, _ = synth_pose_results(model, K, dist, 20, 61, inside=FRAME)
        out[name] = {"recs": recs, "model": flat, "K": K, "dist": dist, "degenerate": lambda f, m, mi: True}
    recs, _ = synth_pose_results(model, K, dist, 12, 62, max_markers=4, inside=FRAME)
    rng = np.random.default_rng(63)
    hit = {}
    for f, value in ((3, np.nan), (4, np.inf), (5, None)):
        r = recs[f]
        r["n_markers"], r["n_features"] = 0, 0
        for mi in (1, 2, 3):
            _, _, pts = random_view(rng, model["corners"][mi], K, dist, 0.2, used=slice(16, 56))
            place_marker(r, int(model["ids"][mi]), pts, 12, [2, 3, 4, 5, 6], [FULL] * 5)
        if value is None:
            r["markers"][1]["n_features"] = 0
        else:
            r["features"][5 + 2]["corners"][0] = value  # marker 1, its middle feature, x of corner 0: always a correspondence
            hit[(f, 1)] = True
    out["non-finite corners"] = {"recs": recs, "model": model, "K": K, "dist": dist, "degenerate": lambda f, m, mi: (f, m) in hit,
                                 "too_few": (5, 1)}
    return out


def guard_batch():
    """16 frames with four corrupted records in the middle (frames 5 .. 8, never the first or the last frame of the batch, so
    that a guard gone missing would still read inside the allocation): a marker whose features end past the record, one that
    starts before it, a negative marker count and one far above the record's 100."""
    K, dist, model = golden_camera_and_model()
    recs = np.zeros(16, RESULT_DT)
    rng = np.random.default_rng(64)
    for f in range(16):
        for _ in range(3):
            mi = int(rng.integers(0, 6))
            _, _, pts = random_view(rng, model["corners"][mi], K, dist, 0.2, used=slice(32, 56))
            place_marker(recs[f], int(model["ids"][mi]), pts, 12, [4, 5, 6], [FULL] * 3)
    recs[5]["markers"][1]["first_feature"], recs[5]["markers"][1]["n_features"] = 98, 5
    recs[6]["markers"][1]["first_feature"] = -1
    recs[7]["n_markers"] = -3
    recs[8]["n_markers"] = 1000
    return {"recs": recs, "model": model, "K": K, "dist": dist}


OFFSET_FRAME_COUNTS = (1, 2, 255, 256, 257, 513)  # around the 256 threads of k_pose_offsets: below, at, one past, two rounds + 1


def offsets_batch(n_frames):
    """n_frames frames of up to two markers; every fifth frame (from frame 2) is not CTAG_OK, every seventh is empty."""
    K, dist, model = golden_camera_and_model()
    recs, _ = synth_pose_results(model, K, dist, n_frames, 300 + n_frames, max_markers=2, n_features=2, id_pattern=FULL, inside=FRAME)
    recs["status"][2::5] = 1
    recs["n_markers"][6::7] = 0
    return {"recs": recs, "model": model, "K": K, "dist": dist}


def oracle_records(po, batch):
    """The pose oracle's records of a batch, frame by frame, in batch order."""
    mv, cam = make_model_view(batch["model"]), make_camera(batch["K"], batch["dist"])
    per = [po.pose_frame(batch["recs"][f], mv, cam, f) for f in range(len(batch["recs"]))]
    return np.concatenate(per) if per else np.zeros(0, POSE_DT)


def check_batch(records, batch):
    """pose_statement.check_pose_records on the records of one of the batches above; a capped batch must fill its cap.  Returns
    the number of records held against scipy's minimum."""
    n = check_pose_records(records, batch["recs"], batch["model"], (batch["K"], batch["dist"]), planted=batch.get("planted"),
                           degenerate=batch.get("degenerate"), max_minimum_checks=batch.get("min_cap"))
    if "min_cap" in batch:
        assert n == batch["min_cap"], "only %d records with >= 16 points" % n
    return n
