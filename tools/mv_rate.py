"""Multi-view rig pose rate on the device: 4096 instants of synthetic detection records in HBM, six markers
(stacked copies of CTag_2f12c.model's model 0) in rigs of 3 and 6 members seen by 2 and 4 cameras 30 degrees apart, three inner
features = 24 points per member and camera, through ctag_mv_rig_pose_batch_device.  In the same run, for comparison,
ctag_rig_pose_batch_device on ONE camera's records with the same points per item (every member shown with 3 x n_cameras features).
Device-resident records (256 distinct instants, repeated); host clock around a synchronised call, median of the timed repeats.  Prints one JSON line.
usage (GPU): python tools/mv_rate.py [n_frames]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cylindertag_amd as ca  # noqa: E402
from ctag_testlib import GOLDEN, RESULT_DT  # noqa: E402
from mv_statement import ring_poses  # noqa: E402
from mv_testlib import synth_mv_instant  # noqa: E402
from pose_testlib import read_camera_yml, read_model_file  # noqa: E402
from rig_testlib import stacked_rig_model, synth_rig_frame  # noqa: E402


def timed(fn, sync, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_frames = int(args[0]) if args else 4096
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    model = stacked_rig_model(read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model")), 6, 70.0)
    centre = model["corners"].reshape(-1, 3).astype(np.float64).mean(0)
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = ca.Detector(state, fs, device=0)
    M = ca.Model(ids=model["ids"], corners=model["corners"], model_size=model["size"], base=model["base"], axis=model["axis"])
    cam = ca.load_camera(os.path.join(GOLDEN, "cameraParams.yml"))
    out = {"lib": ca.lib_path(), "n_frames": n_frames}
    for n_cam in (2, 4):
        rng = np.random.default_rng(n_cam)
        cameras = [(K, dist)] * n_cam
        poses = ring_poses(centre, [30.0 * c for c in range(n_cam)])
        recs = np.zeros((n_cam, n_frames), RESULT_DT)
        one = np.zeros(n_frames, RESULT_DT)  # one camera, the same points per member
        distinct = min(n_frames, 256)  # planted poses; the batch repeats them
        for f in range(distinct):
            recs[:, f] = synth_mv_instant(rng, model, [list(range(6))], cameras, poses, 0.2, feats=(3, 3))[0]
            one[f] = synth_rig_frame(rng, model, [list(range(6))], K, dist, 0.2, feats=(3 * n_cam, 3 * n_cam))[0]
        for f in range(distinct, n_frames):
            recs[:, f] = recs[:, f % distinct]
            one[f] = one[f % distinct]
        d = [torch.from_numpy(recs[c].view(np.uint8).reshape(n_frames, -1)).cuda() for c in range(n_cam)]
        d1 = torch.from_numpy(one.view(np.uint8).reshape(n_frames, -1)).cuda()
        cs = ca.CameraSet([cam] * n_cam, poses)
        for members in (3, 6):
            rigs = ca.Rigs(M, np.arange(6) // members)
            n_items = n_frames * rigs.n_rigs
            buf = torch.zeros(n_items * ca.MV_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
            t = timed(lambda: det.mv_rig_pose_batch_device([x.data_ptr() for x in d], n_frames, M, rigs, cs, buf.data_ptr()), det.sync)
            R = buf.cpu().numpy().view(ca.MV_POSE_DT)
            ok = R["status"] == 0
            buf1 = torch.zeros(n_items * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
            t1 = timed(lambda: det.rig_pose_batch_device(d1.data_ptr(), n_frames, M, rigs, cam, buf1.data_ptr()), det.sync)
            R1 = buf1.cpu().numpy().view(ca.RIG_POSE_DT)
            ok1 = R1["status"] == 0
            out["mv_%dcam_rig%d" % (n_cam, members)] = {
                "items": n_items, "ok": int(ok.sum()), "points_per_item": float(R["n_points"][ok].mean()), "s": t, "items_per_s": n_items / t,
                "points_per_s": float(R["n_points"][ok].sum()) / t, "iterations_cam": float(R["iterations_cam"][ok].mean()),
                "iterations": float(R["iterations"][ok].mean()),
                "rig_one_camera": {"ok": int(ok1.sum()), "points_per_item": float(R1["n_points"][ok1].mean()), "s": t1, "items_per_s": n_items / t1,
                                   "iterations": float(R1["iterations"][ok1].mean())},
                "mv_over_rig": t / t1}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
