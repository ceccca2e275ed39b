"""Device time of the intrinsics fit by kernel kind, and the figure its default rel_tol comes from (needs a GPU).

Fits the 0.1 px cases of tests/intr_fit_shapes.py with CTAG_OPT_TIMING and prints, per case, the observation records, the rounds taken
and the milliseconds of the whole call by kind -- rig pose (the seed pass and the closing pass), view pose, record + assemble, solve --
and per round.  Then, per case, the relative change of the cost when one field of the returned camera moves by one float32 ulp and
the view poses are solved again (the probe of rule 4 from the returned poses), worst over the free fields: the default rel_tol is to be
4 x the worst over the cases.  Measured against nothing but itself: no test depends on these figures.

    python tools/intr_fit_rate.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intr_fit_shapes as sh  # noqa: E402
import intr_fit_statement as it  # noqa: E402
import testkit as tk  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from intr_fit_testlib import camera_c, cost_sum, input_of, opts_of, vector_of  # noqa: E402


def one_ulp_cost_change(det, c, M, rigs, cam, poses, items):
    """The worst relative cost change over the free fields of `cam`, each moved up and down by one float32 ulp."""
    p = vector_of(cam)
    recs = poses.copy()
    recs["status"][[i for i in range(len(recs)) if i not in items]] = 5
    base, _ = det.intrinsics_fit_poses(c["recs"], recs, M, rigs, cam)
    cost = cost_sum(base, items)
    worst = 0.0
    for i in it.free_rows(c["mask"], sh.tie_of(c)):
        for up in (np.inf, -np.inf):
            q = p.copy()
            q[i] = float(np.nextafter(np.float32(p[i]), np.float32(up)))
            if c["tie"]:
                q[1] = q[0] * (p[1] / p[0])
            got, usable = det.intrinsics_fit_poses(c["recs"], base, M, rigs, camera_c(it.round_camera(q, c["n_dist"]), c))
            if usable:
                worst = max(worst, abs(cost_sum(got, items) - cost) / cost)
    return worst


def main():
    rel = 0.0
    for name in [n for n in sh.NAMES if n.endswith("0.1 px") and sh.case(n)["shape"] in sh.END_TO_END]:
        c = sh.case(name)
        det = tk.Detector(c["state"], 2, device=0)
        det.set_option(capi.OPT_TIMING, 1)
        M, rigs, seed = input_of(c)
        det.fit_intrinsics(c["recs"], M, rigs, seed, **opts_of(c))   # warm-up: allocations, code objects
        t0 = time.perf_counter()
        cam, stat, poses = det.fit_intrinsics(c["recs"], M, rigs, seed, **opts_of(c))
        wall = (time.perf_counter() - t0) * 1e3
        ms = det.intrinsics_fit_last_ms()
        rounds = int(stat["rounds"])
        items = sh.views(name).items
        ulp = one_ulp_cost_change(det, c, M, rigs, cam, poses, items)
        rel = max(rel, ulp)
        out = {"case": name, "records": int(stat["n_records"]), "points": int(stat["n_points"]), "free": int(stat["n_free"]), "rounds": rounds,
               "wall_ms": round(wall, 2), "ms": {k: round(v, 3) for k, v in ms.items()},
               "ms_per_round": {k: round(ms[k] / max(rounds, 1), 4) for k in ("view_pose", "record", "solve")}, "one_ulp_rel_cost_change": float("%.3g" % ulp)}
        print(json.dumps(out))
        det.close()
    print(json.dumps({"one_ulp_rel_cost_change_worst": float("%.4g" % rel), "rel_tol_4x": float("%.4g" % (4 * rel))}))


if __name__ == "__main__":
    main()
