"""The figure behind ctag_camera_fit_opts' default rel_tol (needs a GPU).

Every 0.1 px case of tests/cam_fit_shapes.py is fitted with rel_tol 1e-9; then each entry of each moving camera's (rvec, tvec) in the
returned set is changed by one ulp, up and down, the public multi-view call re-solves the observation items under that set, and the
relative change of their summed cost is taken.  Prints the worst per case and overall; the default rel_tol is 4 x the overall worst,
and tests/cam_fit_statement.py holds it as REL_TOL_ULP.

    python tools/cam_fit_rel_tol.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import cam_fit_shapes as sh
import cylindertag_amd as ca
from cam_fit_testlib import Detectors, device_mv_poses, input_of

dets = Detectors()
worst = 0.0
lines = []
for name in [n for n in sh.NAMES if n.endswith("0.1 px")]:
    b, A = sh.case(name), sh.assembled(name)
    det = dets.of(b)
    M, rigs, cams = input_of(b)
    cs, stat, cam_stats = det.fit_camera_set(b["recs"], M, rigs, cams, min_items=b["min_items"], rel_tol=1e-9)
    placed = A["init"]["placed"]
    recs = np.ascontiguousarray(b["recs"][placed])

    def cost_of(poses):
        s = ca.CameraSet([ca.make_camera(*b["cameras"][c]) for c in placed], poses)
        mvp = device_mv_poses(det, recs, M, rigs, s)
        items = [w for w in range(len(mvp)) if mvp[w]["status"] == 0 and mvp[w]["n_cameras"] >= 2]
        return sum(float(mvp[w]["cost"]) for w in items)

    base_poses = [(cam_stats[c]["rvec"].copy(), cam_stats[c]["tvec"].copy()) for c in placed]
    c0 = cost_of(base_poses)
    assert c0 == stat["cost"]
    case_worst = 0.0
    for k, c in enumerate(placed):
        if c == A["init"]["anchor"]:
            continue
        for part in (0, 1):
            for i in range(3):
                for direction in (np.inf, -np.inf):
                    poses = [(rv.copy(), tv.copy()) for rv, tv in base_poses]
                    poses[k][part][i] = np.nextafter(poses[k][part][i], direction)
                    case_worst = max(case_worst, abs(cost_of(poses) - c0) / c0)
    lines.append("%s: cost %.9g, worst relative change %.4e" % (name, c0, case_worst))
    worst = max(worst, case_worst)
lines.append("worst %.4e, 4 x worst %.4e" % (worst, 4 * worst))
print("\n".join(lines))
dets.close()
