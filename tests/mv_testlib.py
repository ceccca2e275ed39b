"""Multi-view rig poses (test infrastructure): synthetic instants seen by several cameras, the one-camera stage of the statement
taken from the pose oracle, and the accuracy study of tools/mv_study.py."""
import numpy as np

from ctag_testlib import RESULT_DT
from mv_statement import MvProblem, membership, project_camera, ring_poses, rotvec, solve_instant, start_camera, to_reference
from pose_statement import rodrigues
from pose_testlib import make_camera
from rig_testlib import add_marker, compose_rig_poses, random_pose, rot_err_deg


def oracle_stage1(po):
    """stage1 of mv_statement.solve_instant from the pose oracle's EPnP and PoseBA."""
    def stage1(K, dist, obj, img):
        cam = make_camera(K, dist)
        st, r0, t0 = po.epnp(cam, obj, img)
        if st != 0:
            return None
        it, r, t, c0, c1 = po.ba(cam, obj, img, r0, t0)
        return r0, t0, r, t, c0, c1, it
    return stage1


def synth_mv_instant(rng, model, rigs, cameras, camera_poses, noise_px, feats=(2, 5), patterns=((3, 4),), show=None, rot_sigma=0.2):
    """One CTAG_OK record per camera of one instant: per rig (a list of model indices) one planted pose in the reference frame,
    and in every camera, for every member shown there, nf in feats consecutive features with pixel noise.  show(camera, rig_index,
    members) -> the members that camera sees (default: all).  Each camera's markers come in a random order.  Returns (records
    [n_cameras], [(rvec, tvec) per rig])."""
    recs = np.zeros(len(cameras), RESULT_DT)
    truth = []
    items = [[] for _ in cameras]
    for gi, mem in enumerate(rigs):
        centre = model["corners"][list(mem)].reshape(-1, 3).astype(np.float64).mean(0)
        rv, tv = random_pose(rng, centre, rot_sigma=rot_sigma)
        truth.append((rv, tv))
        for c in range(len(cameras)):
            for mi in (show(c, gi, mem) if show else mem):
                X = model["corners"][mi].astype(np.float64)
                pts = project_camera(cameras[c], camera_poses[c], rv, tv, X) + rng.normal(0, noise_px, (X.shape[0], 2))
                nf = int(rng.integers(feats[0], feats[1] + 1))
                p0 = int(rng.integers(0, model["size"] - nf + 1))
                items[c].append((int(model["ids"][mi]), mi, pts, p0, nf))
    for c in range(len(cameras)):
        for i in rng.permutation(len(items[c])):
            mid, mi, pts, p0, nf = items[c][i]
            if int(recs[c]["n_features"]) + nf > 100:
                continue
            add_marker(recs[c], mid, mi, model, pts, p0, nf, patterns, rng)
    return recs, truth


def mv_study(po, model, mv, camera, angles_deg, n_frames=300, noise_px=0.2, seed=7):
    """A rig of all of `model`'s markers under planted poses, seen by len(angles_deg) equal cameras on a ring round it (2-5
    consecutive features per marker and camera, pixel noise).  Errors against the planted pose, in the reference frame, of every
    single camera's rig pose (rig composition of the pose oracle, moved by the camera's pose) and of the statement's multi-view
    minimum.  Returns {"single": [(rot_deg[], trans_mm[]) per camera], "mv": (rot_deg[], trans_mm[])}."""
    rng = np.random.default_rng(seed)
    n_models = len(model["ids"])
    rig_of_model = np.zeros(n_models, np.int32)
    centre = model["corners"].reshape(-1, 3).astype(np.float64).mean(0)
    cameras = [camera] * len(angles_deg)
    poses = ring_poses(centre, angles_deg)
    cam_o = make_camera(*camera)
    single = [([], []) for _ in cameras]
    mv_r, mv_t = [], []
    stage1 = oracle_stage1(po)
    for f in range(n_frames):
        recs, truth = synth_mv_instant(rng, model, [list(range(n_models))], cameras, poses, noise_px)
        rv, tv = truth[0]
        for c in range(len(cameras)):
            R = compose_rig_poses(po, recs[c], mv, cam_o, rig_of_model, 1)[0]
            if R["status"] == 0:
                r, t = to_reference(R["rvec"], R["tvec"], poses[c])
                single[c][0].append(rot_err_deg(r, rv))
                single[c][1].append(float(np.linalg.norm(t - tv)))
        M = solve_instant(recs, model, rig_of_model, 1, cameras, poses, stage1, f)[0]
        if M["status"] == 0:
            mv_r.append(rot_err_deg(M["rvec"], rv))
            mv_t.append(float(np.linalg.norm(M["tvec"] - tv)))
    return {"single": [(np.array(a), np.array(b)) for a, b in single], "mv": (np.array(mv_r), np.array(mv_t))}
