"""The cases of tests/test_intr_fit_statement_cpu.py (statement alone), tests/test_intr_fit_forms_gpu.py (the kernels through the
probes) and tests/test_intr_fit_gpu.py (the public calls): hand-built detection records -- rigs of rig_fit_shapes.rig_truth carried
through the frame of the golden camera under planted poses, their pixels the statement's forward projection under a planted camera,
rounded to float32.  Nothing is rendered.  Each shape comes noise-free and at 0.1 px.

A case: name, shape, state (the dictionary of its handle), recs (RESULT_DT), model, rig_of_model, n_rigs, K, dist (the planted camera),
n_dist, seed (K, dist: the free parameters 5 % off in focal length, 25 px off in the principal point and without distortion, the fixed
ones as planted), mask, tie, min_points, noise, planted {item: (rvec, tvec)}."""
import functools

import numpy as np

import intr_fit_statement as it
import pose_statement as ps
from ctag_testlib import RESULT_DT
from pose_testlib import FRAME, FULL, HALF_ALONE, golden_camera_and_model, in_frame, marker_of_points, place_marker, test_cameras
from rig_fit_shapes import rig_truth

RECORD_GRID = 256       # k_ifit_record's grid (testkit.intrinsics_fit_limits() is held against it on the device)
PASS_RECORDS = 512      # observation records one pass of its workspace holds
MASK_HOLES = (1 << 0) | (1 << 1) | (1 << 4) | (1 << 8)   # fx fy . . k1 . . . k3: cx cy k2 fixed, and p1 p2 (below)
# p1 and p2 are free in shape (b) alone.  They are planted at 0, where float32 has no spacing to speak of, and the float32 lattice of the
# OTHER parameters moves their conditional optimum by 1e-10 .. 1e-9: the statement's own float32 loop missed their bar on the 0.1 px
# cases of (b holes), (c) and (d) with them free, so those masks were tightened (the probe's masks still cover their columns).
MASK_NO_TANGENTIAL = 0x3F                                # fx fy cx cy k1 k2


def _recentre(truth):
    """rig_truth puts the tube 600 mm down the z axis; the views here place the rig themselves, so its centre goes to the origin."""
    c = truth["corners"].reshape(-1, 3).astype(np.float64).mean(0)
    out = dict(truth)
    out["corners"] = (truth["corners"].astype(np.float64) - c).astype(np.float32)
    out["base"] = (truth["base"].astype(np.float64) - c).astype(np.float32)
    return out


class _Views:
    def __init__(self, seed, truth, rig_of_model, K, dist, noise, depth=(650.0, 1000.0), tilt=0.35):
        self.rng = np.random.default_rng(seed)
        self.truth, self.rig, self.K, self.dist, self.noise = truth, np.asarray(rig_of_model, np.int32), K, dist, noise
        self.size, self.depth, self.tilt = truth["size"], depth, tilt
        self.n_rigs = int(self.rig.max()) + 1
        self.frames, self.planted = [], {}

    def frame(self, shown, status=0, extra=()):
        """shown = [(model index, positions, patterns)]: every rig among them gets one planted pose that keeps its shown columns in the
        frame; extra = [(model index, positions, patterns)]: markers placed with their rig's pose that are no use (no features)."""
        r = np.zeros((), RESULT_DT)
        f = len(self.frames)
        X = self.truth["corners"].astype(np.float64)
        fx, fy, cx, cy = ps._intrinsics(self.K)
        poses = {}
        for g in sorted({int(self.rig[it_[0]]) for it_ in list(shown) + list(extra)}):
            mine = [s for s in shown if int(self.rig[s[0]]) == g]
            used = np.concatenate([X[m][[8 * (q % self.size) + k for q in (pos or [0]) for k in range(8)]] for m, pos, _ in mine]) if mine else X[0][:8]
            for _ in range(4000):
                rv = self.rng.normal(0, self.tilt, 3)
                z = self.rng.uniform(*self.depth)
                u, v = self.rng.uniform(60, FRAME[0] - 60), self.rng.uniform(60, FRAME[1] - 60)
                tv = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) - ps.rodrigues(rv) @ used.mean(0)
                if in_frame(ps.project12(self.K, self.dist, rv, tv, used), FRAME, margin=4.0):
                    break
            else:
                raise AssertionError("the shown markers do not fit the frame")
            poses[g] = (rv, tv)
            self.planted[f * self.n_rigs + g] = (rv, tv)
        for m, positions, patterns in list(shown) + list(extra):
            rv, tv = poses[int(self.rig[m])]
            pts = ps.project12(self.K, self.dist, rv, tv, X[m])
            if self.noise:
                pts = pts + self.rng.normal(0, self.noise, pts.shape)
            place_marker(r, int(self.truth["ids"][m]), pts, self.size, positions, patterns)
        r["status"] = status
        self.frames.append(r)

    def columns(self, m, n):
        p0 = int(self.rng.integers(0, self.size - n + 1))
        return (m, list(range(p0, p0 + n)), [FULL] * n)


def _seed_of(K, dist, mask, tie):
    """The free parameters off (5 % in focal length, 25 px in the principal point, no distortion), the fixed ones as planted.  A tied
    seed has fy = fx: the ratio 1 survives rule 3's rounding to float32 exactly, any other ratio only to half a spacing of fy, which
    frees fy by that much and moves the weakest coefficients past their bar (measured: 18 x on k1)."""
    K0 = np.array(K, np.float32)
    K0[0, 0] *= np.float32(1.05)
    K0[1, 1] = K0[0, 0] if tie else K0[1, 1] * np.float32(1.05)
    if mask & 4:
        K0[0, 2] += np.float32(25.0)
    if mask & 8:
        K0[1, 2] -= np.float32(25.0)
    d0 = np.array(dist, np.float32)
    for i in range(len(d0)):
        if (mask >> (4 + i)) & 1:
            d0[i] = 0.0
    return K0, d0


def _finish(shape, noise, b, dist, mask=0, tie=False, min_points=8):
    n_dist = len(dist)
    mask = mask or it.default_mask(n_dist)
    name = "%s %s" % (shape, "0.1 px" if noise else "noise-free")
    return {"name": name, "shape": shape, "state": np.random.default_rng(len(shape)).integers(0, 64, (len(b.truth["ids"]), b.size)).astype(np.int32),
            "recs": np.array(b.frames, RESULT_DT), "model": b.truth, "rig_of_model": b.rig.copy(), "n_rigs": b.n_rigs, "K": b.K, "dist": dist, "n_dist": n_dist,
            "seed": _seed_of(b.K, dist, mask, tie), "mask": mask, "tie": tie, "min_points": min_points, "noise": noise, "planted": b.planted}


SHAPES = ("a", "b", "b tied", "b holes", "c", "c12", "d", "e")
END_TO_END = ("a", "b", "b tied", "b holes", "c", "d", "e")   # c12 is the system probe's: sixteen free parameters on 16 records
JOINT = END_TO_END   # the cases held to the statement's joint minimum: every end-to-end shape
NAMES = ["%s %s" % (s, n) for s in SHAPES for n in ("noise-free", "0.1 px")]


@functools.lru_cache(maxsize=None)
def all_cases():
    K = golden_camera_and_model()[0]
    cams = test_cameras()
    out = []
    for noise in (0.0, 0.1):
        # (a) one singleton rig, pinhole, free fx fy cx cy; 6 records at the edges of a 64-point tile
        b = _Views(31, _recentre(rig_truth(1, 20)), [0], K, cams["n_dist0"], noise)
        for n in (8, 60, 64, 68, 128, 132):
            b.frame([(0,) + tuple(marker_of_points(n, 20))])
        out.append(_finish("a", noise, b, cams["n_dist0"]))
        # (b) three-marker rigs, five coefficients, 12 records; the same tied, and with cx cy k2 fixed
        b = _Views(32, _recentre(rig_truth(3, 12)), [0, 0, 0], K, cams["n_dist5"], noise)
        for _ in range(12):
            b.frame([b.columns(m, int(b.rng.integers(4, 7))) for m in range(3)])
        out.append(_finish("b", noise, b, cams["n_dist5"]))
        # tied: fx cx cy k1 k2, with p1 p2 k3 as planted (the float32 rounding of the tied fy alone moves the weakest coefficients past their bar)
        out.append(_finish("b tied", noise, b, cams["n_dist5"], mask=0x3F, tie=True))
        out.append(_finish("b holes", noise, b, cams["n_dist5"], mask=MASK_HOLES))
        # (c) two rigs, eight (and twelve) coefficients, 16 frames: a failed frame, a TOO_FEW record, a record below min_points, an
        #     instant where one rig is not seen
        for shape, dname in (("c", "n_dist8"), ("c12", "n_dist12")):
            b = _Views(33, _recentre(rig_truth(4, 12)), [0, 0, 1, 1], K, cams[dname], noise)
            for f in range(16):
                both = [b.columns(m, int(b.rng.integers(4, 7))) for m in range(4)]
                if f == 3:
                    b.frame(both, status=1)
                elif f == 5:
                    b.frame(both[:2], extra=[(2, [], [])])                 # rig 1: one member without a point
                elif f == 8:
                    b.frame(both[:2] + [(2, [4], [HALF_ALONE])])           # rig 1: 4 points, below min_points
                elif f == 11:
                    b.frame(both[2:])                                      # rig 0 not seen
                else:
                    b.frame(both)
            # eight coefficients: fx fy cx cy k1 k2 free, p1 p2 k3 and the denominator's k4 k5 k6 as planted (free together with the
            # numerator's they trade off along a valley no 16 views of this camera's field of view close)
            out.append(_finish(shape, noise, b, cams[dname], mask=MASK_NO_TANGENTIAL if shape == "c" else 0))
        # (d) 4 records of 796 and 800 points: five members of 160, four coefficients
        b = _Views(34, _recentre(rig_truth(5, 20, gap=2.0, pitch=1.0)), [0] * 5, K, cams["n_dist4"], noise, depth=(520.0, 750.0), tilt=0.5)
        whole = (list(range(20)), [FULL] * 20)
        for f in range(4):
            b.frame([(m,) + whole for m in range(4)] + [(4,) + (whole if f % 2 else tuple(marker_of_points(156, 20)))])
        out.append(_finish("d", noise, b, cams["n_dist4"], mask=MASK_NO_TANGENTIAL))
        # (e) 572 records of 8 + 8 points: past the grid and past a pass; pinhole, tied focal length
        b = _Views(35, _recentre(rig_truth(2, 4, gap=30.0)), [0, 0], K, cams["n_dist0"], noise, depth=(450.0, 700.0), tilt=0.5)
        for _ in range(PASS_RECORDS + 60):
            b.frame([b.columns(0, 1), b.columns(1, 1)])
        out.append(_finish("e", noise, b, cams["n_dist0"], tie=True))
    return out


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def tie_of(c, p_seed=None):
    """Rule 5's ratio: seed fy / seed fx (None without tie_focal)."""
    if not c["tie"]:
        return None
    p = it.camera_vector(*c["seed"]) if p_seed is None else p_seed
    return float(p[1] / p[0])


@functools.lru_cache(maxsize=None)
def views(name):
    c = case(name)
    return it.Views(c["recs"], c["model"], c["rig_of_model"], c["n_rigs"], c["min_points"])


def planted_poses(c, V):
    return np.array([np.concatenate(c["planted"][i]) for i in V.items])


def planted_camera(c):
    return it.camera_vector(c["K"], c["dist"])


def start_camera(c):
    """The planted camera with the fixed parameters at the seed's values: the basin of the call's minimum."""
    p, s = planted_camera(c), it.camera_vector(*c["seed"])
    rows = it.free_rows(c["mask"])
    fixed = [i for i in range(it.N) if i not in rows]
    p[fixed] = s[fixed]
    return p


@functools.lru_cache(maxsize=None)
def second_reference(name):
    """A second joint minimum, from where the statement's own loop ended: MINIMA_DISTANCE is measured between the two."""
    c, V = case(name), views(name)
    F = fit_reference(name)
    return it.joint_minimum(V, F["p"], c["mask"], tie_of(c), F["poses"])


@functools.lru_cache(maxsize=None)
def unrounded_reference(name):
    """The joint minimum of a noise-free case whose pixels are not rounded to float32: F32_PIXEL_MOVE is its distance to joint_reference."""
    c, V = case(name), views(name)
    assert not c["noise"]
    poses = planted_poses(c, V)
    V0 = V.with_pixels(np.zeros_like(V.uv))
    V64 = V.with_pixels(it.residual(V0, planted_camera(c), poses)[0])
    p = start_camera(c)
    tie = tie_of(c)
    if tie is not None:
        p[1] = p[0] * tie
    return it.joint_minimum(V64, p, c["mask"], tie, poses)


@functools.lru_cache(maxsize=None)
def probed_state(name):
    """The state the system probe is asked at: the planted camera (its float32 values) with every record's pose at its minimum."""
    c, V = case(name), views(name)
    p = planted_camera(c)
    return p, it.solve_poses(V, p, planted_poses(c, V))


@functools.lru_cache(maxsize=None)
def joint_reference(name):
    """The statement's joint minimum from the PLANTED state (fixed parameters: the seed's), the planted ratio fy / fx replaced by the
    seed's under tie_focal."""
    c, V = case(name), views(name)
    p = start_camera(c)
    tie = tie_of(c)
    if tie is not None:
        p[1] = p[0] * tie
    return it.joint_minimum(V, p, c["mask"], tie, planted_poses(c, V))


@functools.lru_cache(maxsize=None)
def fit_reference(name, max_rounds=30):
    """The statement's own loop of rule 5 from the seed with rule 3's float32 camera, the view poses started at the planted ones."""
    c, V = case(name), views(name)
    return it.fit(V, it.camera_vector(*c["seed"]), c["n_dist"], c["mask"], tie_of(c), planted_poses(c, V), max_rounds=max_rounds, rel_tol=1e-12)


def check_claims(c):
    """Asserts what a case says it covers, from the statement."""
    V = views(c["name"])
    pts = sorted(set(V.n_points))
    if c["shape"] == "a":
        assert V.n_points == [8, 60, 64, 68, 128, 132], V.n_points
    if c["shape"].startswith("b"):
        assert V.R == 12
    if c["shape"] in ("c", "c12"):
        n_items = len(c["recs"]) * 2
        seen = set(V.items)
        assert len(c["recs"]) == 16 and int((c["recs"]["status"] != 0).sum()) == 1
        assert 6 not in seen and 7 not in seen            # the failed frame
        assert 10 in seen and 11 not in seen              # TOO_FEW: a member without a point
        assert 16 in seen and 17 not in seen              # 4 points: below min_points
        assert 22 not in seen and 23 in seen              # rig 0 not seen
        assert V.R == n_items - 2 - 3
    if c["shape"] == "d":
        assert V.n_points == [796, 800, 796, 800]
    if c["shape"] == "e":
        assert V.R == PASS_RECORDS + 60 > PASS_RECORDS > RECORD_GRID and pts == [16]
    return True
