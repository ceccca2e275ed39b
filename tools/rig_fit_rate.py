"""Device time of the rig assembly by kernel kind (needs a GPU).

Assembles batches of tests/rig_fit_shapes.py with CTAG_OPT_TIMING and prints, per batch, the observation records, the rounds taken
and the milliseconds of the whole call by kind -- marker pose (once), rig pose, record + assemble, solve -- and per round.  Measured
against nothing but itself: no test depends on these figures.

    python tools/rig_fit_rate.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cylindertag_amd as ca  # noqa: E402
import rig_fit_shapes as sh  # noqa: E402
import testkit as tk  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from rig_fit_testlib import input_of  # noqa: E402


def main():
    for name in sh.NAMES:
        b = sh.batch(name)
        det = tk.Detector(b["state"], 2, device=0)
        det.set_option(capi.OPT_TIMING, 1)
        cam = ca.make_camera(b["K"], b["dist"])
        M, rigs = input_of(b)
        opts = ca.rig_fit_opts(min_frames=b["min_frames"])
        det.fit_rigs(b["recs"], M, rigs, cam, opts)   # warm-up: allocations, code objects
        t0 = time.perf_counter()
        _, rig_stats, _, _ = det.fit_rigs(b["recs"], M, rigs, cam, opts)
        wall = (time.perf_counter() - t0) * 1e3
        ms = det.rig_fit_last_ms()
        rounds = int(rig_stats["rounds"].max())
        out = {"batch": name, "frames": len(b["recs"]), "records": int(rig_stats["n_records"].sum()), "points": int(rig_stats["n_points"].sum()), "rounds": rounds,
               "wall_ms": round(wall, 2), "ms": {k: round(v, 3) for k, v in ms.items()},
               "ms_per_round": {k: round(ms[k] / max(rounds, 1), 4) for k in ("rig_pose", "record", "solve")}}
        print(json.dumps(out))
        det.close()


if __name__ == "__main__":
    main()
