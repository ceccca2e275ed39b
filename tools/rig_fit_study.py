"""Rig assembly end to end on planted three-marker rigs (needs a GPU).

A rig of three markers on one tube, 600 mm from the camera (tests/rig_fit_shapes.py: rig_truth), is seen in hand-built detection
records with --noise px of corner noise, 4-6 columns a marker.  The input model has markers 1 and 2 moved by 0.5 rad and 50 mm: each
in its own frame, as Detector.fit_model leaves them.  Detector.fit_rigs assembles it from the first N frames, N = 8, 16, ...; the rig
poses of --test fresh frames are then estimated with the assembled model and with the planted-frame model (the truth) and held against
the planted poses.  Reported per N: the corner distance of the assembled model from the truth, and the median / 90th percentile of
the rig pose error (degrees, mm) with both models -- in rig_study's style.  Measured against nothing but itself.

    python tools/rig_fit_study.py --noise 0.2
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import cylindertag_amd as ca  # noqa: E402
import rig_fit_shapes as sh  # noqa: E402
import testkit as tk  # noqa: E402
from pose_testlib import golden_camera_and_model, test_cameras  # noqa: E402
from rig_fit_testlib import device_rig_poses, model_of  # noqa: E402
from rig_testlib import rot_err_deg  # noqa: E402


def frames(builder, n):
    first = len(builder.frames)
    for _ in range(n):
        builder.frame([(m, int(builder.rng.integers(4, 7))) for m in range(3)])
    return builder.records()[first:], [builder.planted[(f, 0)] for f in range(first, first + n)]


def errors(recs, planted):
    ok = recs["status"] == 0
    rot = np.array([rot_err_deg(r["rvec"], p[0]) for r, p, k in zip(recs, planted, ok) if k])
    tr = np.array([np.linalg.norm(r["tvec"] - p[1]) for r, p, k in zip(recs, planted, ok) if k])
    return {"posed": int(ok.sum()), "rot_deg": [round(float(np.median(rot)), 4), round(float(np.percentile(rot, 90)), 4)],
            "trans_mm": [round(float(np.median(tr)), 3), round(float(np.percentile(tr, 90)), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--test", type=int, default=200)
    ap.add_argument("--counts", type=int, nargs="+", default=[8, 16, 32, 64, 128])
    a = ap.parse_args()
    K, dist = golden_camera_and_model()[0], test_cameras()["n_dist5"]
    truth = sh.rig_truth(3, 12)
    b = sh._Builder(31, truth, [0, 0, 0], K, dist, a.noise)
    model, _ = sh.moved_model(truth, b.rng, keep=(0,))       # model 0 keeps its frame: it becomes the anchor, the rig's frame is the truth's
    train, _ = frames(b, max(a.counts))
    test, planted = frames(b, a.test)
    det = tk.Detector(np.zeros((3, 12), np.int32), 2, device=0)
    cam = ca.make_camera(K, dist)
    M_in, M_true = model_of(model), model_of(truth)
    rigs = ca.Rigs(M_in, [0, 0, 0], 1)
    print(json.dumps({"model": "planted frame", **errors(device_rig_poses(det, test, M_true, ca.Rigs(M_true, [0, 0, 0], 1), cam), planted)}))
    for n in a.counts:
        R, rig_stats, model_stats, placed = det.fit_rigs(train[:n], M_in, rigs, cam)
        d = sh.corner_distance(R.view()["corners"], truth["corners"], [m for m in range(3) if placed[m] >= 0])
        e = errors(device_rig_poses(det, test, R, ca.Rigs(R, placed, 1), cam), planted)
        print(json.dumps({"model": "assembled", "frames": n, "placed": int((placed >= 0).sum()), "rounds": int(rig_stats[0]["rounds"]),
                          "rms_px": round(float(rig_stats[0]["rms_px"]), 4), "corners_from_truth_mm": round(d, 4), **e}))
    det.close()


if __name__ == "__main__":
    main()
