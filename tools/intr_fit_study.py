"""How well views of CylinderTag rigs fix a camera: the independent statement alone, on the CPU.

Cylinders of cylindertag_amd/models.py-like geometry (tests/rig_fit_shapes.rig_truth) with 4 visible columns per marker are carried
through the frame of a planted camera; the pixels are the statement's forward projection plus 0.1 px noise, rounded to float32.  The
statement's own loop (tests/intr_fit_statement.fit, float32 camera every trial) starts 5 % off in focal length, 25 px off in the
principal point and without distortion, and fits fx fy cx cy k1 k2 p1 p2.  Printed per row: a single marker against a three-marker rig,
a 1400 px against a 4328 px camera, 16 against 64 views -- the error of fx, cx, cy against the planted camera, the sigma the call
would return for each, and the error in sigmas.  One seed, reported only: no test depends on these figures.

    python tools/intr_fit_study.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intr_fit_statement as it  # noqa: E402
import pose_statement as ps  # noqa: E402
from ctag_testlib import RESULT_DT  # noqa: E402
from pose_testlib import FRAME, FULL, in_frame, place_marker  # noqa: E402
from rig_fit_shapes import rig_truth  # noqa: E402

MASK = 0xFF
NOISE = 0.1


def views_of(rng, truth, K, dist, n_views):
    X = truth["corners"].astype(np.float64)
    X = X - X.reshape(-1, 3).mean(0)
    truth = dict(truth, corners=X.astype(np.float32))
    fx, fy, cx, cy = ps._intrinsics(K)
    n, size = len(truth["ids"]), truth["size"]
    recs, planted = [], []
    depth = 0.16 * fx      # the rig about as large in the image whatever the focal length
    for _ in range(n_views):
        r = np.zeros((), RESULT_DT)
        p0 = int(rng.integers(0, size - 4 + 1))
        used = np.concatenate([X[m][8 * p0:8 * p0 + 32] for m in range(n)])
        while True:
            rv = rng.normal(0, 0.35, 3)
            z = rng.uniform(0.8 * depth, 1.4 * depth)
            u, v = rng.uniform(60, FRAME[0] - 60), rng.uniform(60, FRAME[1] - 60)
            tv = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) - ps.rodrigues(rv) @ used.mean(0)
            if in_frame(ps.project12(K, dist, rv, tv, used), FRAME, margin=4.0):
                break
        for m in range(n):
            pts = ps.project12(K, dist, rv, tv, X[m]) + rng.normal(0, NOISE, (len(X[m]), 2))
            place_marker(r, int(truth["ids"][m]), pts, size, list(range(p0, p0 + 4)), [FULL] * 4)
        recs.append(r)
        planted.append(np.concatenate([rv, tv]))
    return truth, np.array(recs, RESULT_DT), np.array(planted)


def main():
    dist = np.float32([-0.12, 0.25, 0.0005, -0.0003])
    for focal in (1400.0, 4328.0):
        K = np.float32([[focal, 0, 953.3], [0, focal * 0.9998, 596.0], [0, 0, 1]])
        for markers in (1, 3):
            for n_views in (16, 64):
                rng = np.random.default_rng(5)
                truth, recs, planted = views_of(rng, rig_truth(markers, 12), K, dist, n_views)
                V = it.Views(recs, truth, np.zeros(markers, np.int32), 1)
                p_true = it.camera_vector(K, dist)
                p0 = p_true.copy()
                p0[:2] *= 1.05
                p0[2] += 25.0
                p0[3] -= 25.0
                p0[4:] = 0.0
                F = it.fit(V, p0, 4, MASK, None, planted, rel_tol=1e-12)
                sg, s2 = it.sigma(F["S"], MASK, F["cost"], sum(V.n_points), V.R)
                err = F["p"] - p_true
                print(json.dumps({"focal_px": focal, "markers": markers, "views": n_views, "rounds": F["rounds"], "rms_px": float("%.3g" % np.sqrt(2 * F["cost"] / sum(V.n_points))),
                                  "error": {it.PARAMS[i]: float("%.3g" % err[i]) for i in (0, 2, 3)}, "sigma": {it.PARAMS[i]: float("%.3g" % sg[i]) for i in (0, 2, 3)},
                                  "error_in_sigmas": {it.PARAMS[i]: float("%.2g" % (err[i] / sg[i])) for i in range(8)}}))


if __name__ == "__main__":
    main()
