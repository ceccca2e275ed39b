"""What the two GPU test files of the model reconstruction share: a detector per dictionary, device pose records of a batch under a
model, and the statement's view of them."""
import numpy as np

import cylindertag_amd as ca
import testkit as tk


class Detectors:
    """One tk.Detector per dictionary (a reconstructed model has as many columns as the handle's dictionary)."""

    def __init__(self):
        self.d = {}

    def of(self, b):
        key = b["state"].tobytes()
        if key not in self.d:
            self.d[key] = tk.Detector(b["state"], 2, device=0)
        return self.d[key]

    def close(self):
        for d in self.d.values():
            d.close()


def model_of(m):
    return ca.Model(ids=m["ids"], corners=m["corners"], model_size=m["size"], base=m["base"], axis=m["axis"])


def device_poses(det, recs, model, cam):
    """POSE_DT records of ctag_pose_batch_device for host detection records."""
    import torch
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).cuda()
    total = int(sum(min(max(int(r["n_markers"]), 0), 100) for r in recs if r["status"] == 0))
    d_off = torch.zeros(len(recs) + 1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(max(total, 1) * ca.POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    det.pose_batch_device(d_recs.data_ptr(), len(recs), model, cam, d_off.data_ptr(), d_out.data_ptr(), max(total, 1))
    det.sync()
    assert int(d_off[-1].item()) == total
    return d_out.cpu().numpy()[:total * ca.POSE_DT.itemsize].view(ca.POSE_DT).copy()


def observation_cost(poses, obs, m):
    """Rule 3's sum: the cost fields of model m's observation records, in record order."""
    total = 0.0
    for o in obs:
        if o is not None and o["model"] == m:
            total += float(poses[o["w"]]["cost"])
    return total
