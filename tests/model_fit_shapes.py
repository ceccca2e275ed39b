"""The batches of tests/test_model_fit_statement_cpu.py (statement alone), tests/test_model_fit_forms_gpu.py (the kernels through the
probe) and tests/test_model_fit_gpu.py (the public calls): hand-built detection records -- a true model projected through planted
poses -- with a seed that is off.  Nothing is rendered.  Every coverage claim of a batch ("claims") is asserted from the statement
by check_claims(), not assumed.

A batch: name, state (the dictionary of its handle: model_size columns), recs (RESULT_DT), truth / seed (model dicts), K, dist,
min_obs, noise, planted {(frame, marker): (model, rvec, tvec)}, claims."""
import functools

import numpy as np

import model_fit_statement as ms
import pose_statement as ps
from ctag_testlib import RESULT_DT
from cylindertag_amd.models import cylinder_model
from pose_testlib import FRAME, FULL, HALF_ALONE, HALF_MID, golden_camera_and_model, place_marker, random_view, test_cameras

STRIP = 50.0            # strip height, mm
RADIUS = 40.0           # the true tubes
RECORD_GRID = 256       # k_mfit_record's grid (testkit.model_fit_limits() is held against it on the device)
PATTERNS = (FULL, FULL, FULL, (3, 4), (2, 4), HALF_MID, HALF_ALONE)  # 8 points; 4 points; 4 points, skipped at a marker's ends


def _cylinders(state, radius, rng=None, warp_mm=0.0):
    """Ideal cylinders of the dictionary, half a metre in front of the camera, plus a uniform random warp."""
    c = cylinder_model(state, STRIP, radius).astype(np.float64)
    c[..., 2] += 500.0
    if warp_mm:
        c += rng.uniform(-warp_mm, warp_mm, c.shape)
    return c.astype(np.float32)


def _warped(corners, rng, amp_mm):
    """The corner lists bent by a smooth warp of amplitude amp_mm per axis, about one wave over the strip: what a tube that is not
    a cylinder, or a strip that does not lie flat on it, does to a model."""
    c = corners.astype(np.float64)
    out = c.copy()
    for m in range(len(c)):
        for k in range(3):
            f = rng.uniform(0.5, 1.5, 2)
            out[m, :, k] += amp_mm * np.sin(2 * np.pi * (f[0] * c[m, :, 0] / 100.0 + f[1] * c[m, :, 1] / 100.0) + rng.uniform(0, 2 * np.pi))
    return out.astype(np.float32)


def _model(state, corners):
    n = len(state)
    return {"ids": np.arange(n, dtype=np.int32), "size": state.shape[1], "base": np.tile(np.float32([0, -STRIP / 2, 500]), (n, 1)),
            "axis": np.tile(np.float32([0, 1, 0]), (n, 1)), "corners": corners}


class _Builder:
    def __init__(self, seed, state, K, dist, noise):
        self.rng = np.random.default_rng(seed)
        self.state, self.K, self.dist, self.noise = state, K, dist, noise
        self.size = state.shape[1]
        self.frames, self.planted = [], {}

    def frame(self, status=0):
        r = np.zeros((), RESULT_DT)
        r["status"] = status
        self.frames.append(r)
        return len(self.frames) - 1

    def marker(self, truth, mi, positions, patterns, f=None, marker_id=None):
        f = self.frame() if f is None else f
        used = [p % self.size for p in positions] or [0]
        sl = slice(min(used) * 8, (max(used) + 1) * 8)
        rv, tv, pts = random_view(self.rng, truth[mi], self.K, self.dist, self.noise, inside=FRAME, used=sl)
        r = self.frames[f]
        self.planted[(f, int(r["n_markers"]))] = (mi, rv, tv)
        place_marker(r, mi if marker_id is None else marker_id, pts, self.size, positions, patterns)
        return f

    def random_marker(self, truth, mi, nfs, p_min=0, f=None):
        nf = int(self.rng.choice(nfs))
        p0 = int(self.rng.integers(p_min, self.size - nf + 1))
        pats = [PATTERNS[int(self.rng.integers(0, len(PATTERNS)))] for _ in range(nf)]
        return self.marker(truth, mi, list(range(p0, p0 + nf)), pats, f)

    def records(self):
        return np.array(self.frames, RESULT_DT)


def _no_corner_seen_too_seldom(b, truth, seed_model, models, min_obs, keep=(), p_min=0):
    """Adds full-pattern records until no corner of `models` is seen by 1 .. min_obs - 1 records (those in `keep` excepted)."""
    cam = (b.K, b.dist)
    for _ in range(200):
        seen = ms.seen_counts(ms.observations(b.records(), seed_model, cam), len(b.state), b.size * 8)
        todo = [(m, c) for m in models for c in range(b.size * 8) if 0 < seen[m, c] < min_obs and (m, c) not in keep]
        if not todo:
            return
        m, c = todo[0]
        nf = min(4, b.size)
        p0 = min(max(c // 8 - 1, p_min), b.size - nf)
        b.marker(truth, m, list(range(p0, p0 + nf)), [FULL] * nf)
    raise AssertionError("corners stay under-observed")


def _finish(name, b, truth, seed, min_obs, claims, strip_height=0.0):
    """The batch; the seed's corners that are seen but held (fewer than min_obs records) are set to where the truth lies in the
    seed's gauge: a held corner still takes part in the pose of the record that sees it, with the seed's value (rule 2), and only
    a consistent value leaves the fitted corners' minimum where the similarity gauge puts it."""
    recs, cam = b.records(), (b.K, b.dist)
    seed = seed.copy()
    tm, sm = _model(b.state, truth), _model(b.state, seed)
    obs = ms.observations(recs, sm, cam)
    seen = ms.seen_counts(obs, len(b.state), b.size * 8)
    held = seen < min_obs
    for m in range(len(b.state)):
        odd = held[m] & (seen[m] > 0)
        if odd.any() and (~held[m]).sum() >= 3:
            sim = ms.similarity(truth[m][~held[m]].astype(np.float64), seed[m][~held[m]].astype(np.float64))
            seed[m][odd] = ms.apply_similarity(sim, truth[m][odd]).astype(np.float32)
    return {"name": name, "state": b.state, "recs": recs, "truth": tm, "seed": _model(b.state, seed), "K": b.K, "dist": b.dist, "min_obs": min_obs,
            "noise": b.noise, "planted": b.planted, "claims": claims, "strip_height": strip_height}


def _state(rng, n_models, size):
    return rng.integers(0, 64, (n_models, size)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def all_batches():
    K = golden_camera_and_model()[0]
    cams = test_cameras()
    out = []

    # 1. size 12, three models of 30 records, seed radius +20 %, noise-free, pinhole; model 0 has corners seen by exactly 1, 2 and 3 records
    rng = np.random.default_rng(1)
    st = _state(rng, 3, 12)
    truth, seed = _cylinders(st, RADIUS, rng, 0.3), _cylinders(st, RADIUS * 1.2)
    b = _Builder(11, st, K, np.zeros(0, np.float32), 0.0)
    for p0 in (0, 1, 2):
        b.marker(truth, 0, list(range(p0, p0 + 5)), [FULL] * 5)
    for _ in range(27):
        b.random_marker(truth, 0, (4, 5, 6), p_min=3)
    for m in (1, 2):
        for _ in range(30):
            b.random_marker(truth, m, (4, 5, 6))
    keep = {(0, c) for c in range(8)}
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), (0, 1, 2), 2, keep, p_min=3)
    out.append(_finish("size 12 radius +20% noise-free", b, truth, seed, 2,
                       {"seen": {(0, 0): 1, (0, 8): 2, (0, 16): 3}, "held_seen": True, "n_models": 3, "recover": True}))

    # 2. size 12, radius -20 %, 0.1 px, the golden camera's five coefficients: 60 and 24 records, a model no frame shows, frames that
    #    are not CTAG_OK, records that are TOO_FEW / BAD_POS under the seed, one model twice in a frame
    rng = np.random.default_rng(2)
    st = _state(rng, 3, 12)
    truth, seed = _cylinders(st, RADIUS, rng, 0.3), _cylinders(st, RADIUS * 0.8)
    b = _Builder(12, st, K, cams["n_dist5"], 0.1)
    for m, n in ((0, 60), (1, 24)):
        for _ in range(n):
            b.random_marker(truth, m, (4, 5, 6))
    f = b.random_marker(truth, 0, (5,))
    b.random_marker(truth, 0, (5,), f=f)                       # the same model twice in one frame
    f = b.random_marker(truth, 1, (4,))
    b.marker(truth, 1, [], [], f=f)                             # no feature: TOO_FEW
    b.marker(truth, 0, [12, 3, 4], [FULL] * 3, f=f)             # a position outside the model: BAD_POS
    b.marker(truth, 1, [2, 3, 4, 5], [FULL] * 4, f=f, marker_id=40)  # no model
    f = b.frame(status=1)
    b.marker(truth, 0, [2, 3, 4, 5], [FULL] * 4, f=f)          # a frame that is not CTAG_OK
    b.frame(status=2)
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), (0, 1), 2)
    out.append(_finish("size 12 radius -20% 0.1 px n_dist5", b, truth, seed, 2,
                       {"unseen_model": 2, "bad_frames": 2, "too_few": 1, "bad_pos": 1, "no_model": 1, "twice": True, "n_models": 3}))

    # 3. size 20 (160 corners, the cap): two models of 60 records, seed = truth + a smooth warp of 1 mm, noise-free, eight coefficients
    rng = np.random.default_rng(3)
    st = _state(rng, 2, 20)
    truth = _cylinders(st, RADIUS * 1.5, rng, 0.3)
    seed = _warped(truth, rng, 1.0)
    b = _Builder(13, st, K, cams["n_dist8"], 0.0)
    for m in (0, 1):
        for _ in range(60):
            b.random_marker(truth, m, (4, 5, 6))
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), (0, 1), 2)
    out.append(_finish("size 20 warp 1 mm noise-free n_dist8", b, truth, seed, 2, {"n_models": 2, "recover": True, "corners": 160}))

    # 4. size 20, radius +20 % and the warp, 0.1 px, twelve coefficients, min_obs 3
    rng = np.random.default_rng(4)
    st = _state(rng, 2, 20)
    truth = _cylinders(st, RADIUS * 1.5, rng, 0.3)
    seed = _warped(_cylinders(st, RADIUS * 1.5 * 1.2), rng, 1.0)
    b = _Builder(14, st, K, cams["n_dist12"], 0.1)
    for m in (0, 1):
        for _ in range(60):
            b.random_marker(truth, m, (4, 5, 6))
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), (0, 1), 3)
    out.append(_finish("size 20 radius +20% warp 0.1 px n_dist12 min_obs 3", b, truth, seed, 3, {"n_models": 2, "corners": 160}))

    # 5. size 4, six models, more records than k_mfit_record's grid, radius -20 %, noise-free, pinhole
    rng = np.random.default_rng(5)
    st = _state(rng, 6, 4)
    truth, seed = _cylinders(st, RADIUS * 0.5, rng, 0.2), _cylinders(st, RADIUS * 0.5 * 0.8)
    b = _Builder(15, st, K, np.zeros(0, np.float32), 0.0)
    for i in range(RECORD_GRID + 28):
        b.random_marker(truth, i % 6, (3, 4))
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), range(6), 2)
    out.append(_finish("size 4 six models past the grid", b, truth, seed, 2, {"n_models": 6, "past_grid": True, "recover": True}))

    # 6. the metric scale: batch 1's geometry with a seed that is the truth scaled by 1.1 about its centroid
    rng = np.random.default_rng(6)
    st = _state(rng, 2, 12)
    truth = _cylinders(st, RADIUS, rng, 0.0)
    seed = truth.astype(np.float64)
    seed = (seed.mean(1, keepdims=True) + 1.1 * (seed - seed.mean(1, keepdims=True))).astype(np.float32)
    b = _Builder(16, st, K, np.zeros(0, np.float32), 0.0)
    for m in (0, 1):
        for _ in range(24):
            b.random_marker(truth, m, (4, 5, 6))
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), (0, 1), 2)
    out.append(_finish("size 12 seed scaled by 1.1 noise-free", b, truth, seed, 2, {"n_models": 2, "recover": True, "scaled_seed": 1.1}, strip_height=STRIP))
    # 7. the issue's own case: 96 corners, 60 records a model, seed = truth + 1 mm of RANDOM warp (every coordinate of every corner
    #    moved independently by up to 1 mm), 0.1 px
    rng = np.random.default_rng(7)
    st = _state(rng, 2, 12)
    truth = _cylinders(st, RADIUS, rng, 0.3)
    seed = (truth.astype(np.float64) + rng.uniform(-1.0, 1.0, truth.shape)).astype(np.float32)
    b = _Builder(17, st, K, cams["n_dist5"], 0.1)
    for m in (0, 1):
        for _ in range(60):
            b.random_marker(truth, m, (4, 5, 6))
    _no_corner_seen_too_seldom(b, truth, _model(st, seed), (0, 1), 2)
    out.append(_finish("size 12 random warp 1 mm 0.1 px n_dist5", b, truth, seed, 2, {"n_models": 2, "random_warp_mm": 1.0}))
    return out


def batch(name):
    return next(b for b in all_batches() if b["name"] == name)


NAMES = ["size 12 radius +20% noise-free", "size 12 radius -20% 0.1 px n_dist5", "size 20 warp 1 mm noise-free n_dist8",
         "size 20 radius +20% warp 0.1 px n_dist12 min_obs 3", "size 4 six models past the grid", "size 12 seed scaled by 1.1 noise-free", "size 12 random warp 1 mm 0.1 px n_dist5"]


def camera_of(b):
    return b["K"], b["dist"]


@functools.lru_cache(maxsize=None)
def observed(name):
    """(observations, held [n_models, P], seen [n_models, P]) of a batch under its seed, by the statement."""
    b = batch(name)
    P = b["seed"]["size"] * 8
    obs = ms.observations(b["recs"], b["seed"], camera_of(b))
    n = len(b["seed"]["ids"])
    return obs, ms.held_mask(obs, n, P, b["min_obs"]), ms.seen_counts(obs, n, P)


def planted_poses(b, batch_of_model):
    """[R, 6] planted (rvec, tvec) of the records of a ms.Batch."""
    return np.array([np.concatenate(b["planted"][(o["frame"], o["marker"])][1:]) for o in batch_of_model.recs]).reshape(-1, 6)


def check_claims(b):
    """Asserts what a batch says it covers, from the statement."""
    obs, held, seen = observed(b["name"])
    c = b["claims"]
    recs, seed = b["recs"], b["seed"]
    size = seed["size"]
    assert len(seed["ids"]) == c["n_models"] and 2 <= c["n_models"] <= 6
    per_model = np.bincount([o["model"] for o in obs if o is not None], minlength=c["n_models"])
    for m, n in enumerate(per_model):
        if n:
            assert 24 <= n or c.get("past_grid"), (m, n)
    for (m, corner), n in c.get("seen", {}).items():
        assert seen[m, corner] == n and held[m, corner] == (n < b["min_obs"])
    if c.get("held_seen"):
        assert (held & (seen > 0)).any()
    else:
        assert not (held & (seen > 0)).any(), "a held corner is seen: its seed value would bias the minimum"
    if "unseen_model" in c:
        assert per_model[c["unseen_model"]] == 0 and held[c["unseen_model"]].all()
    st = [ps.expected_record(recs[f], m, seed)[0] for f in range(len(recs)) for m in range(ps.marker_count(recs[f]))]
    assert st.count(ps.TOO_FEW) == c.get("too_few", 0) and st.count(ps.BAD_POS) == c.get("bad_pos", 0) and st.count(ps.NO_MODEL) == c.get("no_model", 0)
    assert int((recs["status"] != 0).sum()) == c.get("bad_frames", 0)
    if c.get("twice"):
        frames = [(o["frame"], o["model"]) for o in obs if o is not None]
        assert len(frames) != len(set(frames))
    if c.get("past_grid"):
        assert sum(o is not None for o in obs) > RECORD_GRID
    if "corners" in c:
        assert size * 8 == c["corners"]
    # records see 4-6 consecutive features (3-4 on the size-4 models), and the end-feature rule bites somewhere
    skipped = 0
    for o in obs:
        if o is None:
            continue
        M = recs[o["frame"]]["markers"][o["marker"]]
        nf = int(M["n_features"])
        assert nf in ((3, 4) if size == 4 else (4, 5, 6))
        cols = sorted(set((o["ids"] // 8).tolist()))
        skipped += nf - len(cols)
    assert skipped > 0, "no end feature was ever skipped"
    return True


def _per_model(name, make):
    b = batch(name)
    obs, held, _ = observed(name)
    out = {}
    for m in range(len(b["seed"]["ids"])):
        B = ms.Batch(obs, m, camera_of(b))
        out[m] = None if not B.recs or held[m].all() else make(b, B, m, held[m], b["seed"]["corners"][m].astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def joint_reference(name):
    """Per model of a batch, computed once and shared (None for a model without observations): the statement's joint minimum over
    corners and poses, started from the PLANTED model and poses carried into the seed's gauge -- the basin of the global minimum by
    construction, which neither the statement's loop nor the device's is asked to find it.  dict(batch, X, poses, cost)."""
    def make(b, B, m, held, seed):
        truth = b["truth"]["corners"][m].astype(np.float64)
        sim = ms.similarity(truth[~held], seed[~held])
        X0 = np.where(held[:, None], seed, ms.apply_similarity(sim, truth))
        return dict(ms.joint_minimum(B, X0, seed, held, ms.moved_poses(sim, planted_poses(b, B))), batch=B)
    return _per_model(name, make)


@functools.lru_cache(maxsize=None)
def fit_reference(name):
    """The statement's own loop of rule 4 from the seed (in double, no float32 rounding), per model: dict(X, poses, cost0, cost, rounds, lam)."""
    return _per_model(name, lambda b, B, m, held, seed: ms.fit(B, seed, held, planted_poses(b, B), max_rounds=15, round_float=False))
