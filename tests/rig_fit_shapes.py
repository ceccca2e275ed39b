"""The batches of tests/test_rig_fit_statement_cpu.py (statement alone), tests/test_rig_fit_forms_gpu.py (the kernels through the
probe) and tests/test_rig_fit_gpu.py (the public calls): hand-built detection records -- a true rig model, every member in one
frame, projected through planted rig poses -- with an input model in which every member but the anchor has been moved by a random
rigid transform of about 0.5 rad and 50 mm.  Nothing is rendered.  Every coverage claim of a batch ("claims") is asserted from the
statement by check_claims(), not assumed.

A batch: name, state (the dictionary of its handle: model_size columns), recs (RESULT_DT), truth / model (model dicts: the rig in one
frame / what the call is given), rig_of_model, n_rigs, K, dist, min_frames, noise, planted {(frame, rig): (rvec, tvec)}, moves
{model: (R, t)} with X_in = R X_truth + t, claims."""
import functools

import numpy as np

import model_fit_statement as ms
import pose_statement as ps
import rig_fit_statement as rf
from ctag_testlib import RESULT_DT
from pose_testlib import FRAME, FULL, HALF_ALONE, golden_camera_and_model, in_frame, marker_of_points, place_marker, test_cameras

RECORD_GRID = 256       # k_rfit_record's grid (testkit.rig_fit_limits() is held against it on the device)
PASS_RECORDS = 512      # observation records one pass of its workspace holds
DEPTH = 600.0           # mm in front of the camera
PITCH = 3.0             # mm between two columns of a marker


def rig_truth(n, size, gap=8.0, pitch=PITCH):
    """n markers of `size` columns wrapped round one tube of radius 25 mm along y, one above the other: all in ONE frame."""
    corners = np.zeros((n, size * 8, 3), np.float32)
    spacing = size * pitch + gap
    for m in range(n):
        y0 = (m - (n - 1) / 2.0) * spacing
        for p in range(size):
            for k in range(8):
                th = (k % 4 - 1.5) * 0.5 + 0.08 * (k // 4) + 0.3 * np.sin(1.7 * m)
                y = y0 + p * pitch + (k // 4) * 0.4 * pitch + (0.17 * pitch if k % 2 else 0.0)
                corners[m, p * 8 + k] = (25.0 * np.sin(th), y, DEPTH - 25.0 * np.cos(th))
    centre = corners.reshape(n, -1, 3).astype(np.float64).mean(1)
    return {"ids": np.arange(n, dtype=np.int32), "size": size, "base": centre.astype(np.float32), "axis": np.tile(np.float32([0, 1, 0]), (n, 1)),
            "corners": corners}


def moved_model(truth, rng, keep=()):
    """The input model: every model of the truth but those in `keep` moved by a rigid transform of about 0.5 rad about its own centre
    and 50 mm.  Returns (model, moves {model: (R, t)} with X_in = R X_truth + t)."""
    m_in = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in truth.items()}
    moves = {}
    for m in range(len(truth["ids"])):
        if m in keep:
            moves[m] = (np.eye(3), np.zeros(3))
            continue
        w = rng.normal(0, 1, 3)
        R = ps.rodrigues(0.5 * w / np.linalg.norm(w))
        s = rng.normal(0, 1, 3)
        c = truth["corners"][m].astype(np.float64).mean(0)
        t = c - R @ c + 50.0 * s / np.linalg.norm(s)
        moves[m] = (R, t)
        m_in["corners"][m] = (truth["corners"][m].astype(np.float64) @ R.T + t).astype(np.float32)
        m_in["base"][m] = (R @ truth["base"][m].astype(np.float64) + t).astype(np.float32)
        m_in["axis"][m] = (R @ truth["axis"][m].astype(np.float64)).astype(np.float32)
    return m_in, moves


class _Builder:
    def __init__(self, seed, truth, rig_of_model, K, dist, noise):
        self.rng = np.random.default_rng(seed)
        self.truth, self.rig, self.K, self.dist, self.noise = truth, np.asarray(rig_of_model, np.int32), K, dist, noise
        self.size = truth["size"]
        self.frames, self.planted = [], {}

    def frame(self, shown, status=0, shuffle=False, extra=(), pose_seed=None):
        """One frame: shown = [(model index, positions, patterns) or (model index, n columns)]; every rig among them gets one planted
        pose.  extra = [(marker id, model index whose points it borrows, positions, patterns)]: markers that are no members."""
        r = np.zeros((), RESULT_DT)
        f = len(self.frames)
        items = []
        for it in shown:
            mi = it[0]
            if len(it) == 2:
                nf = it[1]
                p0 = int(self.rng.integers(0, self.size - nf + 1))
                it = (mi, list(range(p0, p0 + nf)), [FULL] * nf)
            items.append((int(self.truth["ids"][mi]),) + tuple(it))
        items += [tuple(e) for e in extra]
        X = self.truth["corners"].astype(np.float64)
        rng = self.rng if pose_seed is None else np.random.default_rng(pose_seed)
        poses = {}
        for g in sorted({int(self.rig[it[1]]) for it in items}):
            mine = [it for it in items if int(self.rig[it[1]]) == g]
            used = np.concatenate([X[it[1]][[8 * (p % self.size) + k for p in (it[2] or [0]) for k in range(8)]] for it in mine])
            for _ in range(1000):  # the shown columns in front of the camera, about DEPTH away
                rv = rng.normal(0, 0.2, 3)
                tv = np.array([0.0, 0.0, DEPTH]) + rng.normal(0, 1, 3) * np.array([20.0, 20.0, 40.0]) - ps.rodrigues(rv) @ used.mean(0)
                if in_frame(ps.project12(self.K, self.dist, rv, tv, used), FRAME):
                    break
            else:
                raise AssertionError("the shown markers do not fit the frame")
            poses[g] = (rv, tv)
            if g >= 0:
                self.planted[(f, g)] = (rv, tv)
        if shuffle:
            items = [items[i] for i in self.rng.permutation(len(items))]
        for marker_id, mi, positions, patterns in items:
            rv, tv = poses[int(self.rig[mi])]
            pts = ps.project12(self.K, self.dist, rv, tv, X[mi])
            if self.noise:
                pts = pts + self.rng.normal(0, self.noise, pts.shape)
            place_marker(r, marker_id, pts, self.size, positions, patterns)
        r["status"] = status
        self.frames.append(r)
        return f

    def records(self):
        return np.array(self.frames, RESULT_DT)


def _state(rng, n_models, size):
    return rng.integers(0, 64, (n_models, size)).astype(np.int32)


def _finish(name, b, model, moves, n_rigs, min_frames, claims):
    return {"name": name, "state": _state(np.random.default_rng(len(name)), len(b.truth["ids"]), b.size), "recs": b.records(), "truth": b.truth, "model": model,
            "rig_of_model": b.rig.copy(), "n_rigs": n_rigs, "K": b.K, "dist": b.dist, "min_frames": min_frames, "noise": b.noise, "planted": b.planted,
            "moves": moves, "claims": claims}


def _points(n, size):
    return (0,) + tuple(marker_of_points(n, size))


@functools.lru_cache(maxsize=None)
def all_batches():
    K = golden_camera_and_model()[0]
    cams = test_cameras()
    none = np.zeros(0, np.float32)
    out = []

    # (a) 2 models, 24 frames, noise-free, pinhole: the 6 x 6 system; records of 8 points (4 + 4) and of 60 / 64 / 68 points
    truth = rig_truth(2, 12)
    b = _Builder(21, truth, [0, 0], K, none, 0.0)
    model, moves = moved_model(truth, b.rng, keep=(0,))
    # a pose under which EPnP leaves neither 4-point marker in its mirrored minimum (nine draws in ten do): check_no_mirror holds it
    b.frame([(0, [3], [HALF_ALONE]), (1, [5], [HALF_ALONE])], pose_seed=1001)
    for n1 in (28, 32, 36):
        b.frame([(0,) + tuple(marker_of_points(32, 12)), (1,) + tuple(marker_of_points(n1, 12))])
    while len(b.frames) < 24:
        b.frame([(0, int(b.rng.integers(4, 7))), (1, int(b.rng.integers(4, 7)))])
    out.append(_finish("a: 2 models noise-free pinhole", b, model, moves, 1, 2, {"n_placed": {0: 2}, "anchor": {0: 0}, "points": (8, 60, 64, 68), "recover": True}))

    # (b) 4 models in a chain, m and m + 2 never share a frame, 40 frames, 0.1 px, five coefficients; the pair (0, 3) is seen exactly once
    truth = rig_truth(4, 12)
    b = _Builder(22, truth, [0, 0, 0, 0], K, cams["n_dist5"], 0.1)
    model, moves = moved_model(truth, b.rng, keep=(0,))
    b.frame([(0, 5), (3, 5)])
    while len(b.frames) < 40:
        m = (len(b.frames) - 1) % 3
        b.frame([(m, int(b.rng.integers(4, 7))), (m + 1, int(b.rng.integers(4, 7)))])
    out.append(_finish("b: chain of 4 0.1 px n_dist5", b, model, moves, 1, 2,
                       {"n_placed": {0: 4}, "anchor": {0: 0}, "never_together": [(0, 2), (1, 3)], "seen_once": (0, 3), "parents": {1: 0, 2: 1, 3: 2}}))

    # (c) rig 0: models 0-5 and model 9, which is never seen with it; rig 1: models 6-8, its lowest index never co-visible; model 10 loose;
    #     frames that are not CTAG_OK, TOO_FEW / BAD_POS / model-less markers, one model twice in a frame, markers interleaved; eight coefficients
    truth = rig_truth(11, 12)
    rig = [0, 0, 0, 0, 0, 0, 1, 1, 1, 0, -1]
    b = _Builder(23, truth, rig, K, cams["n_dist8"], 0.0)
    model, moves = moved_model(truth, b.rng, keep=(0, 7))
    for i in range(30):
        k = int(b.rng.integers(2, 4))
        first = int(b.rng.integers(0, 7 - k))
        shown = [(m, int(b.rng.integers(4, 7))) for m in range(first, first + k)]
        if i % 2 == 0:
            shown += [(7, 5), (8, 5)]
        if i % 5 == 0:
            shown.append((10, 5))
        b.frame(shown, shuffle=True)
    for _ in range(3):
        b.frame([(6, 5)])
        b.frame([(9, 5), (10, 4)])
    b.frame([(1, 5), (2, 5), (1, 5)])                                                   # model 1 twice: only the first counts
    b.frame([(2, 5), (3, 5)], extra=[(3, 3, [], []), (4, 4, [12, 3, 4], [FULL] * 3), (40, 5, [2, 3, 4, 5], [FULL] * 4)])  # TOO_FEW (a second marker of model 3), BAD_POS, no model
    b.frame([(0, 5), (1, 5)], status=1)
    b.frame([], status=2)
    out.append(_finish("c: two rigs, loose and unplaced models n_dist8", b, model, moves, 2, 2,
                       {"n_placed": {0: 6, 1: 2}, "anchor": {0: 0, 1: 7}, "unplaced": [6, 9, 10], "bad_frames": 2, "too_few": 1, "bad_pos": 1, "no_model": 1,
                        "twice": True, "recover": True}))

    # (d) size 20: 5 members at 160 points, records at 796 / 800 points, 24 frames, 0.1 px, twelve coefficients
    truth = rig_truth(5, 20, gap=2.0, pitch=1.0)
    b = _Builder(24, truth, [0] * 5, K, cams["n_dist12"], 0.1)
    model, moves = moved_model(truth, b.rng, keep=(0,))
    whole = (list(range(20)), [FULL] * 20)
    for i in range(4):
        b.frame([(m,) + whole for m in range(5)])
    b.frame([(m,) + whole for m in range(4)] + [(4,) + tuple(marker_of_points(156, 20))])
    while len(b.frames) < 24:
        k = int(b.rng.integers(2, 4))
        first = int(b.rng.integers(0, 6 - k))
        b.frame([(m, int(b.rng.integers(4, 7))) for m in range(first, first + k)])
    out.append(_finish("d: 5 members of 160 points 0.1 px n_dist12", b, model, moves, 1, 2, {"n_placed": {0: 5}, "anchor": {0: 0}, "points": (796, 800)}))

    # (e) 16 models (the cap, a 90 x 90 system), each frame showing 2-3 neighbours, noise-free, pinhole
    truth = rig_truth(16, 4, gap=6.0)
    b = _Builder(25, truth, [0] * 16, K, none, 0.0)
    model, moves = moved_model(truth, b.rng, keep=(0,))
    for rep in range(3):
        for m in range(15):
            k = 2 if (m + rep) % 2 or m == 14 else 3
            b.frame([(j, 4 if rep else 3) for j in range(m, m + k)])
    out.append(_finish("e: 16 models noise-free pinhole", b, model, moves, 1, 2, {"n_placed": {0: 16}, "anchor": {0: 0}, "cap": True, "recover": True}))

    # (f) size 4, 2 models, more observation records than k_rfit_record's grid and than one workspace pass
    truth = rig_truth(2, 4)
    b = _Builder(26, truth, [0, 0], K, none, 0.0)
    model, moves = moved_model(truth, b.rng, keep=(0,))
    for _ in range(PASS_RECORDS + 60):
        b.frame([(0, int(b.rng.integers(3, 5))), (1, int(b.rng.integers(3, 5)))])
    out.append(_finish("f: 2 models past the grid and the pass", b, model, moves, 1, 2, {"n_placed": {0: 2}, "anchor": {0: 0}, "past_limits": True, "recover": True}))
    return out


NAMES = ["a: 2 models noise-free pinhole", "b: chain of 4 0.1 px n_dist5", "c: two rigs, loose and unplaced models n_dist8",
         "d: 5 members of 160 points 0.1 px n_dist12", "e: 16 models noise-free pinhole", "f: 2 models past the grid and the pass"]


def batch(name):
    return next(b for b in all_batches() if b["name"] == name)


def camera_of(b):
    return b["K"], b["dist"]


def members_of(b, g):
    return [m for m in range(len(b["rig_of_model"])) if b["rig_of_model"][m] == g]


def over_the_cap():
    """Batch (e)'s layout with 17 models in the rig: (model dict, rig_of_model, state)."""
    truth = rig_truth(17, 4, gap=6.0)
    return truth, np.zeros(17, np.int32), _state(np.random.default_rng(17), 17, 4)


def planted_marker_start(b):
    """start_of(frame, marker, model) for rf.marker_poses: the planted rig pose composed with the input model's move -- the exact pose
    of a noise-free record, the basin of the right minimum otherwise.  X_cam = Rp X_truth + tp and X_truth = R^T (X_in - t)."""
    def start_of(f, k, m):
        g = int(b["rig_of_model"][m])
        rv, tv = b["planted"][(f, g)] if (f, g) in b["planted"] else (np.zeros(3), np.array([0.0, 0.0, 1.0]))
        R, t = b["moves"][m]
        Rn = ps.rodrigues(rv) @ R.T
        return np.concatenate([rf.rvec_of(Rn), np.asarray(tv) - Rn @ t])
    return start_of


@functools.lru_cache(maxsize=None)
def assembled(name):
    """The statement's rules 1-4 of a batch, computed once and shared: dict(counted, poses, costs, rigs {g: initial_assembly}, T
    {model: (R, t)} of the placed models, rig_placed, X0 (the initial assembly, float32 values), obs (rig_observations on it))."""
    b = batch(name)
    cam = camera_of(b)
    counted = rf.counted_markers(b["recs"], b["model"])
    poses, costs = rf.marker_poses(b["recs"], b["model"], cam, counted, planted_marker_start(b))
    rigs, T = {}, {}
    rig_placed = -np.ones(len(b["rig_of_model"]), np.int32)
    for g in range(b["n_rigs"]):
        rigs[g] = rf.initial_assembly(poses, len(b["recs"]), members_of(b, g), b["min_frames"])
        T.update(rigs[g]["T"])
        rig_placed[rigs[g]["placed"]] = g
    X0 = rf.layout(b["model"]["corners"], T)
    m0 = dict(b["model"], corners=X0.astype(np.float32))
    obs = rf.rig_observations(b["recs"], m0, rig_placed, b["n_rigs"], cam)
    return {"counted": counted, "poses": poses, "costs": costs, "rigs": rigs, "T": T, "rig_placed": rig_placed, "X0": X0, "obs": obs}


def planted_rig_poses(b, B, anchor):
    """[R, 6] poses of the records of a rig's ms.Batch when the rig's frame is its anchor's input frame: planted o move(anchor)^-1."""
    R, t = b["moves"][anchor]
    out = []
    for o in B.recs:
        rv, tv = b["planted"][(o["frame"], o["rig"])]
        Rn = ps.rodrigues(rv) @ R.T
        out.append(np.concatenate([rf.rvec_of(Rn), np.asarray(tv) - Rn @ t]))
    return np.array(out).reshape(-1, 6)


def planted_layout(b, g, anchor, placed):
    """{model: (R, t)} that carries each placed input model into the anchor's input frame: move(anchor) o move(m)^-1."""
    Ra, ta = b["moves"][anchor]
    T = {}
    for m in placed:
        R, t = b["moves"][m]
        Rn = Ra @ R.T
        T[m] = (np.eye(3), np.zeros(3)) if m == anchor else (Rn, ta - Rn @ t)
    return T


@functools.lru_cache(maxsize=None)
def joint_reference(name):
    """Per rig with observations: the statement's joint minimum over transforms and rig poses, started from the PLANTED layout carried
    into the anchor's frame -- the basin of the global minimum by construction.  {g: dict(batch, T, X, poses, cost)}."""
    b, A = batch(name), assembled(name)
    out = {}
    for g, rig in A["rigs"].items():
        B = ms.Batch(A["obs"], g, camera_of(b))
        if rig["anchor"] < 0 or not B.recs:
            continue
        T0 = planted_layout(b, g, rig["anchor"], rig["placed"])
        out[g] = dict(rf.joint_minimum(B, b["model"]["corners"], T0, rig["placed"], rig["anchor"], planted_rig_poses(b, B, rig["anchor"])), batch=B)
    return out


@functools.lru_cache(maxsize=None)
def fit_reference(name, max_rounds=15):
    """The statement's own loop of rule 5 from the rule-2 start (in double, no float32 rounding), per rig."""
    b, A = batch(name), assembled(name)
    out = {}
    for g, rig in A["rigs"].items():
        B = ms.Batch(A["obs"], g, camera_of(b))
        if rig["anchor"] < 0 or not B.recs:
            continue
        if len(B.recs) > rf.DENSE_RECORDS:   # batch (f): batch (a)'s geometry many times over, minutes of numpy
            continue
        out[g] = rf.fit(B, b["model"]["corners"], rig["T"], rig["placed"], rig["anchor"], planted_rig_poses(b, B, rig["anchor"]), max_rounds=max_rounds,
                        round_float=False)
    return out


def corner_distance(X, Y, models):
    return float(max(np.abs(np.asarray(X, np.float64)[m] - np.asarray(Y, np.float64)[m]).max() for m in models))


MIRROR_FACTOR = 4.0   # a per-marker pose counts as mirrored when its cost exceeds this many times the planted pose's (and 1e-6 px^2)


def check_no_mirror(b, counted, costs):
    """No per-marker pose {(frame, model): cost} of the batch sits in a mirrored minimum: its cost is held against the planted pose's."""
    start_of, cam = planted_marker_start(b), camera_of(b)
    for (f, m), cost in costs.items():
        k = counted[f][m]
        _, _, _, obj, img = ps.expected_record(b["recs"][f], k, b["model"])
        p = start_of(f, k, m)
        planted_cost = ps.Problem(cam[0], cam[1], obj, img).cost_at(p[:3], p[3:])
        assert cost <= max(MIRROR_FACTOR * planted_cost, 1e-6), ("mirrored marker pose", f, m, cost, planted_cost)


def check_claims(b):
    """Asserts what a batch says it covers, from the statement."""
    A = assembled(b["name"])
    c, recs = b["claims"], b["recs"]
    for g, rig in A["rigs"].items():
        assert len(rig["placed"]) == c["n_placed"].get(g, 0) and rig["anchor"] == c["anchor"].get(g, -1), (g, rig["placed"], rig["anchor"])
        assert len(members_of(b, g)) <= rf.MAX_MODELS
    counts = A["rigs"][0]["counts"]
    mem = members_of(b, 0)
    for a, bb in c.get("never_together", []):
        assert counts[mem.index(a), mem.index(bb)] == 0
    if "seen_once" in c:
        a, bb = c["seen_once"]
        assert counts[mem.index(a), mem.index(bb)] == 1 and A["rigs"][0]["parent"][bb] != a and A["rigs"][0]["parent"].get(a) != bb
    if "parents" in c:
        assert A["rigs"][0]["parent"] == c["parents"]
    if "unplaced" in c:
        assert sorted(m for m in range(len(b["rig_of_model"])) if A["rig_placed"][m] < 0) == c["unplaced"]
        lowest = members_of(b, 1)[0]
        assert A["rigs"][1]["anchor"] != lowest and A["rig_placed"][lowest] < 0
    st = [ps.expected_record(recs[f], m, b["model"])[0] for f in range(len(recs)) for m in range(ps.marker_count(recs[f]))]
    assert st.count(ps.TOO_FEW) == c.get("too_few", 0) and st.count(ps.BAD_POS) == c.get("bad_pos", 0) and st.count(ps.NO_MODEL) == c.get("no_model", 0)
    assert int((recs["status"] != 0).sum()) == c.get("bad_frames", 0)
    if c.get("twice"):
        assert any(len([k for k in range(ps.marker_count(r)) if r["markers"][k]["marker_id"] == 1]) == 2 for r in recs)
    n_pts = [len(o["ids"]) for o in A["obs"] if o is not None]
    for n in c.get("points", ()):
        assert n in n_pts, (n, sorted(set(n_pts)))
    if c.get("cap"):
        assert len(A["rigs"][0]["placed"]) == rf.MAX_MODELS
    if c.get("past_limits"):
        assert len(n_pts) > PASS_RECORDS > RECORD_GRID
    for o in A["obs"]:
        if o is not None:
            assert len(o["markers"]) >= 2 and all(A["rig_placed"][m] == o["rig"] for m in o["models"])
    # the initialisation's basin: no per-marker pose sits in a mirrored minimum (its cost against the planted pose's) ...
    check_no_mirror(b, A["counted"], A["costs"])
    # ... and the statement's own loop from the rule-2 start reaches the joint minimum
    ref, own = joint_reference(b["name"]), fit_reference(b["name"])
    for g in own:
        d = corner_distance(own[g]["X"], ref[g]["X"], A["rigs"][g]["placed"])
        assert d <= rf.CORNER_BAR_MM, ("the loop stops away from the joint minimum", g, d)
    return True
