"""Calibration of the pose covariance with the detector in the loop, on the CPU (no GPU).

The ray-cast frames of tools/dense_study.py (planted poses, 1920x1080, f = 2600 px, the camera's cx, cy moved by -0.5 px as
there) go through the oracle's detect(), the pose oracle (EPnP + PoseBA) and the covariance of tests/cov_statement.py with
sigma2_hat.  For every decoded marker with a pose, d = (Log(R_est R_true^T), t_est - t_true) and d^T cov^-1 d are formed; with
independent pixel errors its mean would be about 6.  The corners of one feature share their edge fits, so their errors are
correlated and the figure lies above 6: the mean is the factor by which a user should inflate the covariance.

    python tools/cov_study.py --frames 64
    python tools/cov_study.py --frames 64 --degraded        # blur sigma 1 px, then noise sigma 6 gray levels
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import cov_statement as cs  # noqa: E402
import dense_testlib as dt  # noqa: E402
import mv_statement as ms  # noqa: E402
import testkit as tk  # noqa: E402
from ctag_testlib import Oracle  # noqa: E402
from pose_statement import rodrigues  # noqa: E402
from pose_testlib import PoseOracle, make_camera, make_model_view  # noqa: E402


def run(frames, first=0, degraded=False, seed=1000):
    """d^T cov^-1 d and the point count of every decoded marker with a pose."""
    state, fs, model, K = dt.synth_scene()
    orc, po = Oracle(), PoseOracle()
    mv, cam, camera = make_model_view(model), make_camera(K, np.zeros(5)), (K, np.zeros(5, np.float32))
    m2, pts = [], []
    for f in range(first, first + frames):
        img, truth = tk.synth3d_frame_host(state, f, dt.K_PLANTED, rows=dt.ROWS, cols=dt.COLS)
        if degraded:
            img = dt.degrade(img, seed + f)
        res = orc.detect_fast(img, state, fs)
        if res["status"] != 0:
            continue
        for p in po.pose_frame(res, mv, cam):
            ks = [i for i in range(truth["n_markers"]) if truth["dict_row"][i] == model["ids"][p["model_index"]]] if p["status"] == 0 else []
            if not ks:
                continue
            P = p.copy()
            P["frame"] = 0
            e = cs.expected_marker(P, [res], model, camera, cs.default_opts())
            if e["status"] != cs.COV_OK:
                continue
            Rt, tt = truth["R"][ks[0]].reshape(3, 3), truth["t"][ks[0]]
            d = np.concatenate([ms.rotvec(rodrigues(p["rvec"]) @ Rt.T), p["tvec"] - tt])
            m2.append(float(d @ np.linalg.solve(e["cov"], d)))
            pts.append(int(e["n_points"]))
    return np.array(m2), np.array(pts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--degraded", action="store_true")
    a = ap.parse_args()
    t0 = time.time()
    m2, pts = run(a.frames, a.first, a.degraded)
    print(json.dumps({"set": "degraded" if a.degraded else "clean", "frames": a.frames, "markers": int(len(m2)),
                      "points": [int(pts.min()), int(pts.max())] if len(pts) else [], "mean": float(m2.mean()) if len(m2) else None,
                      "median": float(np.median(m2)) if len(m2) else None, "p90": float(np.percentile(m2, 90)) if len(m2) else None,
                      "seconds": round(time.time() - t0, 1)}))


if __name__ == "__main__":
    main()
