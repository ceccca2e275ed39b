"""Accuracy of one pose per rig against one pose per marker, on the CPU (pose oracle only, no GPU): a rig of three copies of
CTag_2f12c.model's model 0 stacked 70 mm apart along its axis, random planted poses, 2-5 consecutive features per marker and
Gaussian pixel noise.  Prints rotation (deg) / translation (mm) errors, median and p95, per noise level.
usage: python tools/rig_study.py [n_frames] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ctag_testlib import GOLDEN  # noqa: E402
from pose_testlib import PoseOracle, make_camera, make_model_view, read_camera_yml, read_model_file  # noqa: E402
from rig_testlib import rig_study, stacked_rig_model  # noqa: E402


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    rig = stacked_rig_model(read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model")), 3, 70.0)
    po, cam, mv = PoseOracle(), make_camera(K, dist), make_model_view(rig)
    print("%d frames, seed %d; errors: rotation deg / translation mm, median (p95)" % (n_frames, seed))
    for noise in (0.2, 0.5):
        s = rig_study(po, rig, K, dist, cam, mv, n_frames, noise, seed)
        line = []
        for k in ("marker", "rig"):
            r, t = s[k]
            line.append("%s (%d poses): %.3f / %.2f (%.3f / %.2f)" % (k, len(r), np.median(r), np.median(t), np.percentile(r, 95), np.percentile(t, 95)))
        (mr, mt), (rr, rt) = s["marker"], s["rig"]
        print("noise %.1f px | %s | median ratio rot %.1fx trans %.1fx" % (noise, " | ".join(line), np.median(mr) / np.median(rr), np.median(mt) / np.median(rt)))


if __name__ == "__main__":
    main()
