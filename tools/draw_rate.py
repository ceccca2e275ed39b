"""Rate of the drawAxis overlay (ctag_draw_axis_batch_device, k_draw.hip) at 1080p and 4K with 0, 1 and 5 posed markers per
frame (0: the gray -> 3-channel expand alone), on device-resident frames, results and pose records.  Prints one line per case:
frames/s, the expand's HBM traffic (1 B read + 3 B written per pixel) as GB/s and as a fraction of the 8.0 TB/s peak.
usage (GPU box): python tools/draw_rate.py [reps=20]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, "tests")
sys.path.insert(0, ".")
import cylindertag_amd as ca
import testkit as tk
from ctag_testlib import GOLDEN
from pose_testlib import read_camera_yml, read_model_file, synth_pose_results

HBM_PEAK = 8.0e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
model = read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model"))
state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
det = tk.Detector(state, fs)
M = ca.Model(os.path.join(GOLDEN, "CTag_2f12c.model"))


def batch(n, rows, cols, per_frame):
    """n frames with `per_frame` modelled markers each (poses of the synthetic generator, principal point at the centre)."""
    Kc = K.copy()
    Kc[0, 2], Kc[1, 2] = cols / 2.0, rows / 2.0
    recs, truth = synth_pose_results(model, Kc, dist, 2048, 3, max_markers=5)
    cand = [(r, [(i, t) for i, t in enumerate(tf) if t[0] >= 0]) for r, tf in zip(recs, truth)]
    cand = [(r, g) for r, g in cand if len(g) >= per_frame]  # frames with enough modelled markers, used in turn
    res = np.zeros(n, recs.dtype)
    P = np.zeros(n * per_frame, ca.POSE_DT)
    k = 0
    for f in range(n):
        r, good = cand[f % len(cand)]
        res[f] = r
        for i, (mi, rv, tv) in good[:per_frame]:
            P[k]["model_index"], P[k]["frame"], P[k]["marker"], P[k]["rvec"], P[k]["tvec"] = mi, f, i, rv, tv
            k += 1
    off = np.arange(n + 1, dtype=np.int32) * per_frame
    return Kc, res, P, off


for rows, cols, n in ((1080, 1920, 512), (1080, 1920, 4096), (2160, 3840, 128), (2160, 3840, 1024)):
    frames = torch.randint(0, 256, (n, rows, cols), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, rows, cols * 3), dtype=torch.uint8, device="cuda")
    for per in (0, 1, 5):
        Kc, res, P, off = batch(n, rows, cols, per)
        cam = ca.make_camera(Kc, dist)
        d_res = torch.from_numpy(res.view(np.uint8).reshape(n, -1)).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_p = torch.from_numpy(P.view(np.uint8).copy() if len(P) else np.zeros(1, np.uint8)).cuda()

        def run():
            det.draw_axis_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, d_res.data_ptr(), d_off.data_ptr(), d_p.data_ptr(),
                                       len(P), M, cam, 30, out.data_ptr(), cols * 3, rows * cols * 3)

        run()
        det.sync()
        t0 = time.perf_counter()  # the calls are enqueued back to back on the handle's stream: wall time of the batch / reps
        for _ in range(reps):
            run()
        det.sync()
        ms = (time.perf_counter() - t0) * 1e3 / reps
        fps = n / (ms * 1e-3)
        bw = n * rows * cols * 4 / (ms * 1e-3)
        print("%dx%d markers/frame %d: %d frames in %.3f ms = %.0f frames/s; expand traffic %.2f TB/s = %.0f %% of HBM peak"
              % (cols, rows, per, n, ms, fps, bw / 1e12, 100 * bw / HBM_PEAK), flush=True)
det.close()
