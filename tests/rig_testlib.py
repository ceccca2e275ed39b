"""Rig poses on the CPU (test infrastructure): the reference oracle of ctag_rig_pose_batch_device is a composition of the
existing pose oracle -- ctago_build_correspondences per member marker, concatenation, ctago_solve_pnp_epnp, ctago_pose_ba --
following the rules of include/ctag_pose.h.  Also synthetic rigs (stacked copies of one marker model, planted poses) and
the accuracy study of tools/rig_study.py."""
import numpy as np

from ctag_testlib import RESULT_DT
from pose_testlib import project, rodrigues

RIG_POSE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("n_members", "<i4"), ("n_excluded", "<i4"),
                        ("n_points", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"), ("member_mask", "<u4", (4,)),
                        ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("rvec0", "<f8", (3,)), ("tvec0", "<f8", (3,)),
                        ("cost0", "<f8"), ("cost", "<f8")])
assert RIG_POSE_DT.itemsize == 160
POSE_OK, POSE_TOO_FEW, POSE_BAD_POS, POSE_NOT_SEEN = 0, 2, 3, 5
RIG_MAX_POINTS = 800
MAX_MARKERS = 100


def rig_points(po, res, mv, ids, rig_of_model, g):
    """Membership of rig g in one frame record and its concatenated correspondences:
    (member_mask list of marker indices, n_excluded, obj[n,3] float32, img[n,2] float32)."""
    members, excluded, objs, imgs, n, seen_ids = [], 0, [], [], 0, set()
    for k in range(min(int(res["n_markers"]), MAX_MARKERS)):
        mid = int(res["markers"][k]["marker_id"])
        hit = np.nonzero(ids == mid)[0]
        if hit.size == 0 or rig_of_model[int(hit[0])] != g:
            continue
        mi = int(hit[0])
        dup = mid in seen_ids
        seen_ids.add(mid)
        if dup:
            excluded += 1
            continue
        st, obj, img = po.correspondences(res, k, mv, mi)
        if st != POSE_OK or n + len(obj) > RIG_MAX_POINTS:
            excluded += 1
            continue
        members.append(k)
        objs.append(obj)
        imgs.append(img)
        n += len(obj)
    obj = np.concatenate(objs) if objs else np.zeros((0, 3), np.float32)
    img = np.concatenate(imgs) if imgs else np.zeros((0, 2), np.float32)
    return members, excluded, obj, img


def compose_rig_poses(po, res, mv, cam, rig_of_model, n_rigs, frame_index=0):
    """The n_rigs records of one frame as include/ctag_pose.h states them, from the pose oracle's pieces."""
    ids = np.ctypeslib.as_array(mv.view.marker_id, (mv.view.n_models,)).copy() if mv.view.n_models else np.zeros(0, np.int32)
    out = np.zeros(n_rigs, RIG_POSE_DT)
    for g in range(n_rigs):
        R = out[g]
        R["rig"], R["frame"] = g, frame_index
        R["status"] = POSE_NOT_SEEN
        if res["status"] != 0:
            continue
        members, excluded, obj, img = rig_points(po, res, mv, ids, rig_of_model, g)
        R["n_members"], R["n_excluded"], R["n_points"] = len(members), excluded, len(obj)
        for k in members:
            R["member_mask"][k >> 5] |= np.uint32(1 << (k & 31))
        if not members:
            continue
        if len(obj) < 4:
            R["status"] = POSE_TOO_FEW
            continue
        st, r0, t0 = po.epnp(cam, obj, img)
        R["status"] = st
        if st != POSE_OK:
            continue
        it, r, t, c0, c1 = po.ba(cam, obj, img, r0, t0)
        R["rvec0"], R["tvec0"], R["rvec"], R["tvec"] = r0, t0, r, t
        R["iterations"], R["cost0"], R["cost"] = it, c0, c1
    return out


def stacked_rig_model(model, n=3, spacing=70.0, src=0, ids=None):
    """n copies of model `src`'s geometry stacked `spacing` mm apart along its axis (centred on it): one rig, one frame."""
    ax = np.asarray(model["axis"][src], np.float64)
    ax = ax / np.linalg.norm(ax)
    off = [(j - (n - 1) / 2.0) * spacing * ax for j in range(n)]
    return {"ids": np.asarray(ids if ids is not None else np.arange(n), np.int32), "size": model["size"],
            "base": np.array([model["base"][src] + o for o in off], np.float32),
            "axis": np.array([model["axis"][src]] * n, np.float32),
            "corners": np.array([model["corners"][src] + o for o in off], np.float32)}


def cylinder_model(n, size, spacing=40.0, pitch=1.8, radius=25.0, z=1500.0, ids=None):
    """n synthetic markers of `size` features (8 corners each, features `pitch` mm apart) on one cylinder of the given radius along
    y, `spacing` mm apart, about z mm in front of the camera: models in one frame, for model sizes the shipped .model does not have."""
    corners = np.zeros((n, size * 8, 3), np.float32)
    for m in range(n):
        y0 = (m - (n - 1) / 2.0) * spacing
        for p in range(size):
            for k in range(8):
                th = (k % 4 - 1.5) * 0.28 + 0.05 * (k // 4)
                y = y0 + p * pitch + (k // 4) * 0.7 + (0.3 if k % 2 else 0.0)
                corners[m, p * 8 + k] = (radius * np.sin(th), y, z - radius * np.cos(th))
    return {"ids": np.asarray(ids if ids is not None else np.arange(n), np.int32), "size": size,
            "base": np.zeros((n, 3), np.float32), "axis": np.tile(np.float32([0, -1, 0]), (n, 1)), "corners": corners}


def random_pose(rng, centre, rot_sigma=0.2, shift=(20.0, 20.0, 40.0)):
    rv = rng.normal(0, rot_sigma, 3)
    R = rodrigues(rv)
    tv = centre - R @ centre + rng.normal(0, 1, 3) * np.asarray(shift)
    return rv, tv


def add_marker(r, marker_id, model_index, model, pts, p0, nf, patterns, rng):
    """Appends one marker of nf consecutive features from position p0, corners from the projected model points pts."""
    m, f0 = int(r["n_markers"]), int(r["n_features"])
    r["markers"][m] = (marker_id, f0, nf, nf)
    for j in range(nf):
        F = r["features"][f0 + j]
        F["pos"] = p0 + j
        il, ir = patterns[int(rng.integers(0, len(patterns)))]
        F["id_left"], F["id_right"] = il, ir
        F["id"] = 8 * il + ir if ir >= 0 else -2
        F["corners"] = pts[(p0 + j) * 8:(p0 + j) * 8 + 8].astype(np.float32).ravel()
    r["n_markers"] = m + 1
    r["n_features"] = f0 + nf


def synth_rig_frame(rng, model, rigs, K, dist, noise_px, feats=(2, 5), patterns=((3, 4),), show=None):
    """One CTAG_OK frame record: per rig (a list of model indices) one planted pose, and for every shown member nf in feats
    consecutive features with pixel noise.  show(rig_index, members) -> the members to show (default: all).  Markers of all rigs
    are interleaved in a random order.  Returns (record, [(rvec, tvec) per rig])."""
    r = np.zeros((), RESULT_DT)
    truth, items = [], []
    for gi, mem in enumerate(rigs):
        centre = model["corners"][list(mem)].reshape(-1, 3).astype(np.float64).mean(0)
        rv, tv = random_pose(rng, centre)
        truth.append((rv, tv))
        for mi in (show(gi, mem) if show else mem):
            X = model["corners"][mi].astype(np.float64)
            pts = project(K, dist, rv, tv, X) + rng.normal(0, noise_px, (X.shape[0], 2))
            nf = int(rng.integers(feats[0], feats[1] + 1))
            p0 = int(rng.integers(0, model["size"] - nf + 1))
            items.append((int(model["ids"][mi]), mi, pts, p0, nf))
    for i in rng.permutation(len(items)):
        mid, mi, pts, p0, nf = items[i]
        if int(r["n_features"]) + nf > 100:
            continue
        add_marker(r, mid, mi, model, pts, p0, nf, patterns, rng)
    return r, truth


def rot_err_deg(r1, r2):
    R = rodrigues(r1).T @ rodrigues(r2)
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


def rig_study(po, model, K, dist, cam, mv, n_frames=300, noise_px=0.2, seed=7):
    """The issue's study: a rig of 3 stacked copies of `model`'s geometry, planted random poses, 2-5 consecutive features per
    marker with pixel noise; errors of every per-marker pose (pose oracle, model frame = rig frame) and of the rig pose
    (this composition) against the planted pose.  Returns {"marker": (rot_deg[], trans_mm[]), "rig": (...)}."""
    rng = np.random.default_rng(seed)
    rig_model = model
    per_r, per_t, rig_r, rig_t = [], [], [], []
    rig_of_model = np.zeros(len(rig_model["ids"]), np.int32)
    for f in range(n_frames):
        res, truth = synth_rig_frame(rng, rig_model, [list(range(len(rig_model["ids"])))], K, dist, noise_px)
        rv, tv = truth[0]
        for p in po.pose_frame(res, mv, cam):
            if p["status"] == POSE_OK:
                per_r.append(rot_err_deg(p["rvec"], rv))
                per_t.append(float(np.linalg.norm(p["tvec"] - tv)))
        R = compose_rig_poses(po, res, mv, cam, rig_of_model, 1)[0]
        if R["status"] == POSE_OK:
            rig_r.append(rot_err_deg(R["rvec"], rv))
            rig_t.append(float(np.linalg.norm(R["tvec"] - tv)))
    return {"marker": (np.array(per_r), np.array(per_t)), "rig": (np.array(rig_r), np.array(rig_t))}


def compose_batch(po, batch, recs=None):
    """compose_rig_poses over the frames of one of tests/rig_shapes.py's batches (or over `recs` under its model and camera)."""
    from pose_testlib import make_camera, make_model_view
    recs = batch["recs"] if recs is None else recs
    mv, cam = make_model_view(batch["model"]), make_camera(batch["K"], batch["dist"])
    return np.concatenate([compose_rig_poses(po, recs[f], mv, cam, batch["rig_of_model"], batch["n_rigs"], f) for f in range(len(recs))])
