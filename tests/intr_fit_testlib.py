"""What the GPU test files of the intrinsics fit share: a detector per dictionary, a case's inputs as the calls take them, the device's
rig pose records under a camera, and records that carry the statement's poses for the probes."""
import numpy as np

import cylindertag_amd as ca
import intr_fit_shapes as sh
import intr_fit_statement as it
from model_fit_testlib import Detectors, model_of  # noqa: F401  (re-exported)

TIGHT = 1e-12   # rel_tol of the tests that ask for the minimum itself
NOT_SEEN = 5


def input_of(c):
    """(Model, Rigs, seed CameraC) a case's call is given."""
    M = model_of(c["model"])
    return M, ca.Rigs(M, c["rig_of_model"], c["n_rigs"]), ca.make_camera(*c["seed"])


def opts_of(c, **kw):
    o = dict(free_mask=c["mask"], tie_focal=int(c["tie"]), min_points=c["min_points"], rel_tol=TIGHT)
    o.update(kw)
    return o


def camera_c(p, c):
    """The CameraC of a parameter vector with the case's n_dist."""
    return ca.make_camera(*it.camera_of(p, c["K"], c["n_dist"]))


def vector_of(cam):
    return it.camera_vector(np.array(cam.K[:], np.float32).reshape(3, 3), np.array(cam.dist[:cam.n_dist], np.float32))


def device_rig_poses(det, recs, model, rigs, cam):
    """RIG_POSE_DT records [n_frames * n_rigs] of ctag_rig_pose_batch_device for host detection records."""
    import torch
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).cuda()
    n = len(recs) * rigs.n_rigs
    d_out = torch.zeros(n * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    det.rig_pose_batch_device(d_recs.data_ptr(), len(recs), model, rigs, cam, d_out.data_ptr())
    det.sync()
    return d_out.cpu().numpy().view(ca.RIG_POSE_DT).copy()


def records_at(template, V, poses):
    """The template's records with the observation records of V carrying `poses` and every other record out of the way (NOT_SEEN): what
    the probes take as a state."""
    out = template.copy()
    keep = np.zeros(len(out), bool)
    for k, item in enumerate(V.items):
        assert out[item]["status"] == 0 and out[item]["n_points"] == V.n_points[k], (item, out[item]["status"], out[item]["n_points"], V.n_points[k])
        out[item]["rvec"], out[item]["tvec"] = poses[k, :3], poses[k, 3:]
        keep[item] = True
    out["status"][~keep] = NOT_SEEN
    return out


def poses_of(recs, V):
    return np.array([np.concatenate([recs[i]["rvec"], recs[i]["tvec"]]) for i in V.items])


def cost_sum(recs, items):
    """The cost fields of the given records summed in record order."""
    total = 0.0
    for i in items:
        total += float(recs[i]["cost"])
    return total
