"""What the GPU test files of the camera set fit share: a detector per dictionary, the case's inputs as the calls take them, device
multi-view records under a camera set, and the checks of a returned set against the statement."""
import numpy as np

import cam_fit_shapes as sh
import cam_fit_statement as cf
import cylindertag_amd as ca
import pose_statement as ps
from model_fit_testlib import Detectors, model_of  # noqa: F401  (re-exported)

TIGHT = 1e-9   # rel_tol of the tests that ask for the minimum itself


def input_of(b):
    """(Model, Rigs, [CameraC]) a case's call is given."""
    M = model_of(b["model"])
    return M, ca.Rigs(M, b["rig_of_model"], b["n_rigs"]), [ca.make_camera(K, d) for K, d in b["cameras"]]


def set_of(b, placed, R, t):
    """The CameraSet of the cameras `placed` at the state (R, t)."""
    return ca.CameraSet([ca.make_camera(*b["cameras"][c]) for c in placed], [(cf.mv.rotvec(R[k]) if np.abs(R[k] - np.eye(3)).max() else np.zeros(3), t[k]) for k in range(len(placed))])


def device_mv_poses(det, recs, model, rigs, cs):
    """MV_POSE_DT records [n_frames * n_rigs] of ctag_mv_rig_pose_batch_device for host detection records recs[camera][frame]."""
    import torch
    recs = np.asarray(recs)
    n_frames = recs.shape[1]
    d = [torch.from_numpy(np.ascontiguousarray(recs[c]).view(np.uint8).reshape(-1)).cuda() for c in range(recs.shape[0])]
    n = n_frames * rigs.n_rigs
    out = torch.zeros(n * ca.MV_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    det.mv_rig_pose_batch_device([t.data_ptr() for t in d], n_frames, model, rigs, cs, out.data_ptr())
    det.sync()
    return out.cpu().numpy().view(ca.MV_POSE_DT).copy()


def device_rig_records(det, b, model, rigs, cams, min_points=8):
    """cf.rig_records' dictionary from the device's own per-camera rig poses (ctag_rig_pose_batch_device, camera by camera): rule 1 as
    the call sees it, whichever minimum EPnP + PoseBA ended in."""
    import torch
    out = {}
    n_frames = b["recs"].shape[1]
    for c in range(len(cams)):
        d_recs = torch.from_numpy(np.ascontiguousarray(b["recs"][c]).view(np.uint8).reshape(-1)).cuda()
        d_out = torch.zeros(n_frames * rigs.n_rigs * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
        det.rig_pose_batch_device(d_recs.data_ptr(), n_frames, model, rigs, cams[c], d_out.data_ptr())
        det.sync()
        for i, r in enumerate(d_out.cpu().numpy().view(ca.RIG_POSE_DT)):
            if r["status"] == 0:
                out[(c, i)] = {"pose": np.concatenate([r["rvec"], r["tvec"]]), "n_points": int(r["n_points"]), "counted": int(r["n_points"]) >= min_points}
    return out


def state_of(cam_stats, placed):
    """(R, t) of the placed cameras from CAMERA_FIT_CAM_STAT_DT records."""
    return np.array([ps.rodrigues(cam_stats[c]["rvec"]) for c in placed]), np.array([cam_stats[c]["tvec"] for c in placed])


def observation_cost(mv_poses, items):
    """Rule 3's sum: the cost fields of the observation records, in item order."""
    total = 0.0
    for w in items:
        total += float(mv_poses[w]["cost"])
    return total
