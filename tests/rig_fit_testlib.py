"""What the GPU test files of the rig assembly share: device rig-pose records of a batch under a model, the batch's Rigs, and the
sums the statistics are held to."""
import numpy as np

import cylindertag_amd as ca
import rig_fit_shapes as sh
from model_fit_testlib import Detectors, device_poses, model_of  # noqa: F401  (re-exported)


def device_rig_poses(det, recs, model, rigs, cam):
    """RIG_POSE_DT records [n_frames * n_rigs] of ctag_rig_pose_batch_device for host detection records."""
    import torch
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).cuda()
    n = len(recs) * rigs.n_rigs
    d_out = torch.zeros(n * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    det.rig_pose_batch_device(d_recs.data_ptr(), len(recs), model, rigs, cam, d_out.data_ptr())
    det.sync()
    return d_out.cpu().numpy().view(ca.RIG_POSE_DT).copy()


def input_of(b):
    """(Model, Rigs) a batch's call is given."""
    M = model_of(b["model"])
    return M, ca.Rigs(M, b["rig_of_model"], b["n_rigs"])


def model_at(b, corners):
    """The batch's model list with other corners (float32)."""
    return model_of(dict(b["model"], corners=np.asarray(corners, np.float32)))


def observation_cost(rig_poses, obs, g):
    """Rule 4's sum: the cost fields of rig g's observation records, in (frame, rig) order."""
    total = 0.0
    for o in obs:
        if o is not None and o["rig"] == g:
            total += float(rig_poses[o["w"]]["cost"])
    return total


def marker_costs(b, poses, counted):
    """{(frame, model): cost} of the device's per-marker pose records (POSE_DT, pose record k of a frame is its marker k) for the counted markers."""
    import pose_statement as ps
    off = ps.offsets_of(b["recs"])
    return {(f, m): float(poses[off[f] + k]["cost"]) for f, d in enumerate(counted) for m, k in d.items()}
