"""Robust refit rate on the device, by the method of tools/cov_rate.py: 4096 frames of synthetic detection
records in HBM, six markers per frame (stacked copies of CTag_2f12c.model's model 0, four inner features = 32 points each) -- 24 576
markers, or rigs of 3 and of 6 markers.  For each kind the pose call and, on the records it left, the robust call (default options:
Cauchy, automatic scale, up to 50 iterations; and max_iterations = 0, the evaluation alone) are timed in the same run.
Device-resident records; host clock around a synchronised call, median of 10 after 3 warm-ups; the whole measurement runs twice.
Prints one JSON line per run.
usage (GPU): python tools/robust_rate.py [n_frames]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cylindertag_amd as ca  # noqa: E402
from ctag_testlib import GOLDEN, RESULT_DT  # noqa: E402
from pose_testlib import read_camera_yml, read_model_file  # noqa: E402
from rig_rate import timed  # noqa: E402
from rig_testlib import stacked_rig_model, synth_rig_frame  # noqa: E402


def main():
    import torch
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    model = stacked_rig_model(read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model")), 6, 70.0)
    rng = np.random.default_rng(1)
    recs = np.zeros(n_frames, RESULT_DT)
    for f in range(n_frames):
        recs[f] = synth_rig_frame(rng, model, [list(range(6))], K, dist, 0.2, feats=(4, 4))[0]
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = ca.Detector(state, fs, device=0)
    M = ca.Model(ids=model["ids"], corners=model["corners"], model_size=model["size"], base=model["base"], axis=model["axis"])
    cam = ca.load_camera(os.path.join(GOLDEN, "cameraParams.yml"))
    d = torch.from_numpy(recs.view(np.uint8).reshape(n_frames, -1)).cuda()
    n_markers = int(recs["n_markers"].sum())
    off = torch.zeros(n_frames + 1, dtype=torch.int32, device="cuda")
    poses = torch.zeros(n_markers * ca.POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    full, evaluate = ca.robust_opts(), ca.robust_opts(max_iterations=0)

    def report(n_items, rob, tp, tr, te):
        R = rob.cpu().numpy().view(ca.ROBUST_POSE_DT)
        ok = R["status"] == 0
        return {"items": n_items, "robust_ok": int(ok.sum()), "points_per_item": float(R["n_points"][ok].mean()),
                "iterations_per_item": float(R["iterations"][ok].mean()), "pose_s": tp, "robust_s": tr, "evaluate_s": te,
                "robust_items_per_s": n_items / tr, "evaluate_items_per_s": n_items / te, "robust_over_pose": tr / tp}
    for run in range(2):
        out = {"run": run, "n_frames": n_frames}
        rob = torch.zeros(n_markers * ca.ROBUST_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
        tp = timed(lambda: det.pose_batch_device(d.data_ptr(), n_frames, M, cam, off.data_ptr(), poses.data_ptr(), n_markers), det.sync)
        te = timed(lambda: det.robust_pose_batch_device(d.data_ptr(), n_frames, M, cam, off.data_ptr(), poses.data_ptr(), n_markers, rob.data_ptr(), evaluate), det.sync)
        tr = timed(lambda: det.robust_pose_batch_device(d.data_ptr(), n_frames, M, cam, off.data_ptr(), poses.data_ptr(), n_markers, rob.data_ptr(), full), det.sync)
        out["marker"] = report(n_markers, rob, tp, tr, te)
        for members in (3, 6):
            rigs = ca.Rigs(M, np.arange(6) // members)
            n_items = n_frames * rigs.n_rigs
            buf = torch.zeros(n_items * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
            rob = torch.zeros(n_items * ca.ROBUST_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
            tp = timed(lambda: det.rig_pose_batch_device(d.data_ptr(), n_frames, M, rigs, cam, buf.data_ptr()), det.sync)
            te = timed(lambda: det.robust_rig_pose_batch_device(d.data_ptr(), n_frames, M, rigs, cam, buf.data_ptr(), rob.data_ptr(), evaluate), det.sync)
            tr = timed(lambda: det.robust_rig_pose_batch_device(d.data_ptr(), n_frames, M, rigs, cam, buf.data_ptr(), rob.data_ptr(), full), det.sync)
            out["rig%d" % members] = report(n_items, rob, tp, tr, te)
        print(json.dumps(out), flush=True)
    det.close()


if __name__ == "__main__":
    main()
