"""Accuracy of one multi-view pose per rig against the best single camera's rig pose, on the CPU (pose oracle and the statement
of tests/mv_statement.py, no GPU): a rig of three copies of CTag_2f12c.model's model 0 stacked 70 mm apart along its axis, random
planted poses, equal cameras on a ring round it, 2-5 consecutive features per marker and camera, Gaussian pixel noise.  Prints
rotation (deg) / translation (mm) errors in the reference frame, median and p95.
usage: python tools/mv_study.py [n_frames] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ctag_testlib import GOLDEN  # noqa: E402
from mv_testlib import mv_study  # noqa: E402
from pose_testlib import PoseOracle, make_model_view, read_camera_yml, read_model_file  # noqa: E402
from rig_testlib import stacked_rig_model  # noqa: E402

RINGS = {"2 cameras 60 deg apart": (0, 60), "2 cameras 90 deg apart": (0, 90), "4 cameras 30 deg apart": (0, 30, 60, 90),
         "4 cameras 60 deg apart": (-90, -30, 30, 90)}


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    K, dist = read_camera_yml(os.path.join(GOLDEN, "cameraParams.yml"))
    rig = stacked_rig_model(read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model")), 3, 70.0)
    po, mv = PoseOracle(), make_model_view(rig)
    print("%d instants, seed %d, 0.2 px; errors: rotation deg / translation mm, median (p95)" % (n_frames, seed))
    for name, angles in RINGS.items():
        s = mv_study(po, rig, mv, (K, dist), angles, n_frames, 0.2, seed)
        best = min(s["single"], key=lambda rt: np.median(rt[1]))
        (br, bt), (mr, mt) = best, s["mv"]
        print("%s | best single camera: %.3f / %.2f (%.3f / %.2f) | multi-view: %.3f / %.2f (%.3f / %.2f) | median ratio rot %.1fx trans %.1fx"
              % (name, np.median(br), np.median(bt), np.percentile(br, 95), np.percentile(bt, 95), np.median(mr), np.median(mt),
                 np.percentile(mr, 95), np.percentile(mt, 95), np.median(br) / np.median(mr), np.median(bt) / np.median(mt)))


if __name__ == "__main__":
    main()
