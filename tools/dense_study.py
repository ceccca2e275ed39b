"""Accuracy of the dense edge-based pose refinement against PoseBA, on the CPU, with known answers (no GPU).

Ray-cast cylinders with planted poses (ctag_synth3d_frame_host, 1920x1080, f = 2600 px) go through the oracle's detect(),
the pose oracle (EPnP + PoseBA) and the numpy statement of the dense refinement (tests/dense_testlib.py).  Each decoded
marker's rotation error (degrees) and translation error (relative to the distance) against the planted pose are taken for
the PoseBA pose and for the dense pose; the medians are printed as one JSON line per parameter set.

The synthetic renderer puts pixel (x, y)'s centre at (x + 0.5, y + 0.5) of the pinhole model (supersampling at
x + (s + 0.5) / 4), while OpenCV, the detector and the pose back end put it at (x, y); the camera used here is therefore
the planted one with cx, cy moved by -0.5 px, so that neither pose carries the half-pixel shift as a pose error.

    python tools/dense_study.py --frames 64                       # clean frames, default parameters
    python tools/dense_study.py --frames 64 --degraded            # blur sigma 1 px, then noise sigma 6 gray levels
    python tools/dense_study.py --frames 64 --params '{"dense_weight": 3.0}'
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

import dense_testlib as dt  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--degraded", action="store_true")
    ap.add_argument("--params", default="{}", help="JSON object of dense parameters (dense_testlib.DEFAULTS keys)")
    a = ap.parse_args()
    params = json.loads(a.params)
    t0 = time.time()
    E, st = dt.run(a.frames, a.first, a.degraded, params)
    print(json.dumps({"set": "degraded" if a.degraded else "clean", "frames": a.frames, "first": a.first, "params": params,
                      "markers": int(E.shape[0]), "status_counts": np.bincount(st, minlength=5).tolist(),
                      "median_rot_deg": {"poseba": float(np.median(E[:, 0])), "dense": float(np.median(E[:, 2]))},
                      "median_rel_t": {"poseba": float(np.median(E[:, 1])), "dense": float(np.median(E[:, 3]))},
                      "seconds": round(time.time() - t0, 1)}))


if __name__ == "__main__":
    main()
