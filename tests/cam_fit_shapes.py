"""The cases of tests/test_cam_fit_statement_cpu.py (statement alone), tests/test_cam_fit_forms_gpu.py (the kernels through the probe)
and tests/test_cam_fit_gpu.py (the public calls): hand-built detection records -- a rig model in one frame, carried through planted
poses in front of cameras on a ring about a metre away, the rig within |x/z| < 0.15 of every optical axis (where
the five undistortion steps converge below float32's pixel rounding).  Nothing is rendered.  Every case comes noise-free and at 0.1 px;
markers carry at least 2 features each, so that no start record is a lone 4-corner pose.  Every coverage claim of a case ("claims") is
asserted from the statement by check_claims(), not assumed.

A case: name, state (the dictionary of its handle), recs [camera][instant] (RESULT_DT), model, rig_of_model, n_rigs, cameras [(K, dist)],
camera_poses (planted, in the ring's reference frame), planted {(instant, rig): (rvec, tvec)} in that frame, noise, min_items, claims."""
import functools

import numpy as np

import cam_fit_statement as cf
import mv_statement as mv
import pose_statement as ps
from ctag_testlib import RESULT_DT
from pose_testlib import FULL, HALF_ALONE, golden_camera_and_model, marker_of_points, place_marker, test_cameras
from rig_fit_shapes import rig_truth

RECORD_GRID = 256       # k_cfit_record's grid (testkit.camera_fit_limits() is held against it on the device)
PASS_RECORDS = 512      # observation records one pass of its workspace holds
DISTANCE = cf.CAMERA_DISTANCE_MM
CENTRE = np.array([0.0, 0.0, DISTANCE])
TWO_HALVES = ([2, 8], [HALF_ALONE, HALF_ALONE])   # 8 points from two 4-point features six columns apart


def ring_cameras(n, seed):
    """n cameras with their own intrinsics and coefficient counts (0, 5, 8, 12) on a ring round CENTRE, each shifted a little."""
    rng = np.random.default_rng(seed)
    K0 = golden_camera_and_model()[0]
    tc = test_cameras()
    cameras = []
    for c in range(n):
        K = K0.copy()
        s = 0.9 + 0.03 * c
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K[0, 0] * s, K[1, 1] * (s + 0.01), K[0, 2] + 11 * c, K[1, 2] - 7 * c
        cameras.append((K, tc[("n_dist0", "n_dist5", "n_dist8", "n_dist12")[c % 4]]))
    step = 50.0 if n == 2 else min(40.0, 300.0 / n)
    angles = [(c - (n - 1) / 2.0) * step + rng.uniform(-4, 4) + 3.0 for c in range(n)]
    return cameras, mv.ring_poses(CENTRE, angles, shifts=rng.normal(0, 1, (n, 3)) * np.array([15.0, 10.0, 30.0]))


class _Builder:
    def __init__(self, seed, model, rig_of_model, n_cameras, noise):
        self.rng = np.random.default_rng(seed)
        self.model, self.rig, self.noise, self.size = model, np.asarray(rig_of_model, np.int32), noise, model["size"]
        self.cameras, self.poses = ring_cameras(n_cameras, seed)
        self.inst, self.planted = [], {}
        self.limit = 0.15   # |x/z| of every point

    def instant(self, shown, status=None, empty=()):
        """One instant.  shown = {camera: [(model, positions, patterns) or (model, n features)]}; every rig among them gets one planted
        pose.  status = {camera: record status}; empty = [(camera, model)]: a marker without features."""
        f = len(self.inst)
        recs = np.zeros(len(self.cameras), RESULT_DT)
        X = self.model["corners"].astype(np.float64)
        rigs = sorted({int(self.rig[it[0]]) for items in shown.values() for it in items})
        pose = {}
        for g in rigs:
            mine = np.nonzero(self.rig == g)[0]
            rv = self.rng.normal(0, 0.2, 3)
            tv = CENTRE + self.rng.normal(0, 1, 3) * np.array([30.0, 30.0, 40.0]) - ps.rodrigues(rv) @ X[mine].reshape(-1, 3).mean(0)
            pose[g] = self.planted[(f, g)] = (rv, tv)
        for c, items in shown.items():
            for it in items:
                mi = it[0]
                if len(it) == 2:
                    p0 = int(self.rng.integers(0, self.size - it[1] + 1))
                    it = (mi, list(range(p0, p0 + it[1])), [FULL] * it[1])
                rv, tv = pose[int(self.rig[mi])]
                pts = mv.project_camera(self.cameras[c], self.poses[c], rv, tv, X[mi])
                assert np.abs((pts - self.cameras[c][0][:2, 2]) / np.diag(self.cameras[c][0])[:2]).max() < self.limit, "a point leaves |x/z| < %g" % self.limit
                if self.noise:
                    pts = pts + self.rng.normal(0, self.noise, pts.shape)
                place_marker(recs[c], int(self.model["ids"][mi]), pts, self.size, it[1], it[2])
        for c, mi in empty:
            place_marker(recs[c], int(self.model["ids"][mi]), np.zeros((self.size * 8, 2)), self.size, [], [])
        for c, st in (status or {}).items():
            recs[c]["status"] = st
        self.inst.append(recs)
        return f

    def finish(self, name, n_rigs, claims, min_items=2):
        recs = np.array(self.inst, RESULT_DT).T.copy()   # [camera][instant]
        state = np.random.default_rng(len(name)).integers(0, 64, (len(self.model["ids"]), self.size)).astype(np.int32)
        return {"name": name, "state": state, "recs": recs, "model": self.model, "rig_of_model": self.rig.copy(), "n_rigs": n_rigs, "cameras": self.cameras,
                "camera_poses": self.poses, "planted": self.planted, "noise": self.noise, "min_items": min_items, "claims": claims}


def _points(mi, n, size):
    return (mi,) + (TWO_HALVES if n == 8 else tuple(marker_of_points(n, size)))


def _case_a(noise):
    b = _Builder(31, rig_truth(2, 12), [0, 0], 2, noise)
    for n0, n1 in ((8, 8), (60, 64), (64, 68), (68, 60)):
        b.instant({0: [_points(0, n0, 12)], 1: [_points(1, n1, 12)]})
    for _ in range(8):
        b.instant({c: [(0, int(b.rng.integers(2, 5))), (1, int(b.rng.integers(2, 5)))] for c in range(2)})
    return b.finish("a: 2 cameras, runs of 8 60 64 68", 1, {"anchor": 0, "placed": [0, 1], "parents": {1: 0}, "runs": (8, 60, 64, 68)})


def _case_b(noise):
    b = _Builder(32, rig_truth(2, 12), [0, 0], 4, noise)
    for pair, n in (((0, 1), 4), ((1, 2), 2), ((2, 3), 4)):
        for _ in range(n):
            b.instant({c: [(0, int(b.rng.integers(2, 5))), (1, int(b.rng.integers(2, 5)))] for c in pair})
    return b.finish("b: chain of 4 cameras", 1, {"anchor": 0, "placed": [0, 1, 2, 3], "parents": {1: 0, 2: 1, 3: 2}, "chain": True, "exactly_min_items": (1, 2)})


def _case_c(noise):
    b = _Builder(33, rig_truth(4, 12), [0, 0, 1, 1], 5, noise)
    both = lambda g: [(2 * g, int(b.rng.integers(2, 4))), (2 * g + 1, int(b.rng.integers(2, 4)))]  # noqa: E731
    for _ in range(4):
        b.instant({1: both(0), 2: both(0)})
    for _ in range(3):
        b.instant({1: both(1), 3: both(1), 2: both(0)})          # two rigs at one instant: cameras 1 and 3 share rig 1, camera 2 sees rig 0 alone
    # cameras 2 and 3 share rig 0 three times
    for _ in range(3):
        b.instant({2: both(0), 3: both(0)})
    for _ in range(3):
        b.instant({3: both(0), 4: both(0)})
    for _ in range(2):
        b.instant({0: both(0)})                                   # seen by one camera only: no observation
    b.instant({0: both(0), 1: both(0)})                           # camera 0 shares one item: below min_items, unplaced
    b.instant({1: both(0), 2: both(0)}, status={2: 1})            # a failed frame
    b.instant({1: both(0)}, empty=[(2, 0)])                       # camera 2's rig record is TOO_FEW
    b.instant({3: both(0), 4: [(0, [3], [HALF_ALONE])]})          # camera 4's record has 4 points: below min_points
    return b.finish("c: anchor 1, camera 0 unplaced, two rigs", 2,
                    {"anchor": 1, "placed": [1, 2, 3, 4], "parents": {2: 1, 3: 1, 4: 3}, "unplaced": [0], "tie": (3, 1, 2), "failed_frames": 1, "too_few": 1,
                     "below_min_points": 1, "single_camera_items": 3})


def _case_d(noise):
    b = _Builder(34, rig_truth(8, 20, gap=2.0, pitch=1.0), [0] * 8, 8, noise)
    for last in (100, 100, 96):
        b.instant({c: [_points(c, last if c == 7 else 100, 20)] for c in range(8)})
    for _ in range(5):
        b.instant({c: [(c, 2), ((c + 1) % 8, 2)] for c in range(8)})
    return b.finish("d: 8 cameras, instants of 796 and 800 points", 1, {"anchor": 0, "placed": list(range(8)), "totals": (796, 800), "cap": True})


def _case_e(noise):
    b = _Builder(35, rig_truth(2, 12), [0, 0], 2, noise)
    for _ in range(PASS_RECORDS + 60):
        b.instant({0: [_points(0, 8, 12)], 1: [_points(1, 8, 12)]})
    return b.finish("e: 572 records of 8 + 8 points", 1, {"anchor": 0, "placed": [0, 1], "parents": {1: 0}, "past_limits": True})


BASE = {"a": _case_a, "b": _case_b, "c": _case_c, "d": _case_d, "e": _case_e}
NAMES = ["%s %s" % (k, n) for k in BASE for n in ("noise-free", "0.1 px")]


@functools.lru_cache(maxsize=None)
def case(name):
    k, n = name.split(" ", 1)
    b = BASE[k](0.0 if n == "noise-free" else 0.1)
    b["name"] = name
    return b


def planted_start(b):
    """start_of(camera, instant, rig) for cf.rig_records: the planted rig pose seen from the planted camera."""
    def start_of(c, f, g):
        rv, tv = b["planted"][(f, g)]
        Rc, tc = ps.rodrigues(b["camera_poses"][c][0]), np.asarray(b["camera_poses"][c][1])
        return mv.rotvec(Rc @ ps.rodrigues(rv)), Rc @ np.asarray(tv) + tc
    return start_of


def planted_set(b, placed, anchor):
    """(R [k, 3, 3], t [k, 3]) of the placed cameras' planted poses carried into the anchor's frame: T_c o T_anchor^-1."""
    Ra, ta = ps.rodrigues(b["camera_poses"][anchor][0]), np.asarray(b["camera_poses"][anchor][1])
    R, t = [], []
    for c in placed:
        Rc, tc = ps.rodrigues(b["camera_poses"][c][0]), np.asarray(b["camera_poses"][c][1])
        Rn = Rc @ Ra.T
        R.append(np.eye(3) if c == anchor else Rn)
        t.append(np.zeros(3) if c == anchor else tc - Rn @ ta)
    return np.array(R), np.array(t)


def planted_rig_poses(b, O, anchor):
    """[R, 6]: the planted rig poses of the observation records in the anchor camera's frame."""
    Ra, ta = ps.rodrigues(b["camera_poses"][anchor][0]), np.asarray(b["camera_poses"][anchor][1])
    out = []
    for w in O.items:
        rv, tv = b["planted"][(w // b["n_rigs"], w % b["n_rigs"])]
        out.append(np.concatenate([mv.rotvec(Ra @ ps.rodrigues(rv)), Ra @ np.asarray(tv) + ta]))
    return np.array(out).reshape(-1, 6)


@functools.lru_cache(maxsize=None)
def assembled(name):
    """The statement's rules 1-3 of a case, computed once and shared: dict(rr (rig_records), init (initial_assembly), R0 t0 (the initial
    set over the placed cameras), slot (the anchor's slot), obs (Observations over the placed cameras))."""
    b = case(name)
    n_items = b["recs"].shape[1] * b["n_rigs"]
    rr = cf.rig_records(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], planted_start(b))
    init = cf.initial_assembly(rr, len(b["cameras"]), n_items, b["min_items"])
    placed = init["placed"]
    out = {"rr": rr, "init": init}
    if placed:
        out["R0"] = np.array([init["T"][c][0] for c in placed])
        out["t0"] = np.array([init["T"][c][1] for c in placed])
        out["slot"] = placed.index(init["anchor"])
        out["obs"] = cf.Observations(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], placed)
    return out


@functools.lru_cache(maxsize=None)
def joint_reference(name):
    """The statement's joint minimum over camera poses and rig poses, started from the PLANTED set carried into the anchor's frame."""
    b, A = case(name), assembled(name)
    O, init = A["obs"], A["init"]
    R, t = planted_set(b, init["placed"], init["anchor"])
    return cf.joint_minimum(O, R, t, A["slot"], planted_rig_poses(b, O, init["anchor"]))


@functools.lru_cache(maxsize=None)
def fit_reference(name, max_rounds=15):
    """The statement's own loop of rule 4 from the rule-2 start."""
    b, A = case(name), assembled(name)
    return cf.fit(A["obs"], A["R0"], A["t0"], A["slot"], planted_rig_poses(b, A["obs"], A["init"]["anchor"]), max_rounds=max_rounds)


def set_distance(Ra, ta, Rb, tb):
    return cf.pose_distance(Ra, ta, Rb, tb, DISTANCE)


def within_bar(d):
    return d[0] <= cf.POSE_BAR[0] and d[1] <= cf.POSE_BAR[1]


def check_claims(b):
    """Asserts what a case says it covers, from the statement."""
    A = assembled(b["name"])
    c, init, rr, O = b["claims"], A["init"], A["rr"], A["obs"]
    n_cam, n_inst, n_rigs = len(b["cameras"]), b["recs"].shape[1], b["n_rigs"]
    assert init["anchor"] == c["anchor"] and init["placed"] == c["placed"], (init["anchor"], init["placed"])
    if "parents" in c:
        assert init["parent"] == c["parents"], init["parent"]
    cnt = init["counts"]
    for (cc, i), r in rr.items():   # no start record is a lone 4-corner pose, bar the one the case plants
        assert r["n_points"] >= 8 or c.get("below_min_points"), (cc, i)
    if "runs" in c:
        runs = {p for pts in O.points_of_camera for p in pts}
        assert set(c["runs"]) <= runs, runs
    if c.get("chain"):
        assert all(cnt[a, bb] == 0 for a in range(n_cam) for bb in range(n_cam) if abs(a - bb) > 1)
        assert cnt[c["exactly_min_items"]] == b["min_items"]
    if "unplaced" in c:
        assert [k for k in range(n_cam) if k not in init["placed"]] == c["unplaced"] and c["anchor"] != 0
        assert n_rigs == 2 and len({w % n_rigs for w in O.items}) == 2
        bb, a1, a2 = c["tie"]
        assert cnt[a1, bb] == cnt[a2, bb] >= b["min_items"]
        assert int((b["recs"]["status"] != 0).sum()) == c["failed_frames"]
        assert sum(1 for r in rr.values() if not r["counted"]) == c["below_min_points"]
        empty = sum(1 for k in range(n_cam) for f in range(n_inst) for m in range(ps.marker_count(b["recs"][k][f])) if b["recs"][k][f]["markers"][m]["n_features"] == 0)
        assert empty == c["too_few"]
        single = 0
        for f in range(n_inst):
            for g in range(n_rigs):
                per, _ = mv.membership([b["recs"][k][f] for k in init["placed"]], b["model"], b["rig_of_model"], g)
                single += sum(1 for m, _, _ in per if m) == 1
        assert single >= c["single_camera_items"] and all(sum(1 for p in pts if p) >= 1 for pts in O.points_of_camera)
    if "totals" in c:
        assert set(c["totals"]) <= set(O.n_points) and max(O.n_points) == 800 and len(init["placed"]) == mv.MAX_CAMERAS
    if c.get("past_limits"):
        assert O.R > PASS_RECORDS > RECORD_GRID and set(O.n_points) == {16}
    return True
