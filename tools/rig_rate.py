"""Rig pose rate on the device: 4096 frames of synthetic detection records in HBM, six markers per frame
(stacked copies of CTag_2f12c.model's model 0, four inner features = 32 points each), through ctag_rig_pose_batch_device with
rigs of 1, 3 and 6 members (6, 2 and 1 rig per frame), and the same records through the per-marker ctag_pose_batch_device.
Device-resident records; host clock around a synchronised call, median of the timed repeats.  Prints one JSON line.
usage (GPU): python tools/rig_rate.py [n_frames] [--marker-only]   (--marker-only: the per-marker rate alone, for a package
without the rig entry points, e.g. PYTHONPATH=<an older checkout>)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # after PYTHONPATH: another build of the package can be measured with --marker-only
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cylindertag_amd as ca  # noqa: E402
from ctag_testlib import GOLDEN, RESULT_DT  # noqa: E402
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
    marker_only = "--marker-only" in sys.argv
    n_frames = int(args[0]) if args else 4096
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
    t = timed(lambda: det.pose_batch_device(d.data_ptr(), n_frames, M, cam, off.data_ptr(), poses.data_ptr(), n_markers), det.sync)
    P = poses.cpu().numpy().view(ca.POSE_DT)
    ok = P["status"] == 0
    out = {"lib": ca.lib_path(), "n_frames": n_frames, "marker": {"items": n_markers, "ok": int(ok.sum()), "s": t, "items_per_s": n_markers / t,
                                                                   "points_per_s": float(P["n_points"][ok].sum()) / t}}
    if not marker_only:
        for members in (1, 3, 6):
            rig_of_model = np.arange(6) // members
            rigs = ca.Rigs(M, rig_of_model)
            n_items = n_frames * rigs.n_rigs
            buf = torch.zeros(n_items * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
            t = timed(lambda: det.rig_pose_batch_device(d.data_ptr(), n_frames, M, rigs, cam, buf.data_ptr()), det.sync)
            R = buf.cpu().numpy().view(ca.RIG_POSE_DT)
            ok = R["status"] == 0
            out["rig%d" % members] = {"items": n_items, "ok": int(ok.sum()), "points_per_item": float(R["n_points"][ok].mean()), "s": t,
                                      "items_per_s": n_items / t, "points_per_s": float(R["n_points"][ok].sum()) / t}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
