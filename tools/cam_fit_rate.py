"""Device time of the camera set fit by kernel kind (needs a GPU).

Fits cases of tests/cam_fit_shapes.py with CTAG_OPT_TIMING and prints, per case, the observation records, the rounds taken and the
milliseconds of the whole call by kind -- per-camera rig pose (once), multi-view pose, record + assemble, solve -- and per round.
Measured against nothing but itself: no test depends on these figures.

    python tools/cam_fit_rate.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cam_fit_shapes as sh  # noqa: E402
import testkit as tk  # noqa: E402
from cam_fit_testlib import input_of  # noqa: E402
from cylindertag_amd import capi  # noqa: E402


def main():
    for name in [n for n in sh.NAMES if n.endswith("0.1 px")]:
        b = sh.case(name)
        det = tk.Detector(b["state"], 2, device=0)
        det.set_option(capi.OPT_TIMING, 1)
        M, rigs, cams = input_of(b)
        det.fit_camera_set(b["recs"], M, rigs, cams, min_items=b["min_items"])   # warm-up: allocations, code objects
        t0 = time.perf_counter()
        _, stat, _ = det.fit_camera_set(b["recs"], M, rigs, cams, min_items=b["min_items"])
        wall = (time.perf_counter() - t0) * 1e3
        ms = det.camera_fit_last_ms()
        rounds = int(stat["rounds"])
        out = {"case": name, "cameras": len(cams), "instants": int(b["recs"].shape[1]), "records": int(stat["n_records"]), "points": int(stat["n_points"]),
               "rounds": rounds, "wall_ms": round(wall, 2), "ms": {k: round(v, 3) for k, v in ms.items()},
               "ms_per_round": {k: round(ms[k] / max(rounds, 1), 4) for k in ("mv_pose", "record", "solve")}}
        print(json.dumps(out))
        det.close()


if __name__ == "__main__":
    main()
