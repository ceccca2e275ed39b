"""The camera set fit end to end, on the CPU with the independent statement alone (tests/cam_fit_statement.py).

tools/mv_study.py's ring of 2 and 4 equal cameras round a three-marker rig about a metre away, 0.2 px corner noise.  The camera poses
are fitted (rules 1-4 of the statement, from the planted start's basin) from the first 8 / 16 / 64 / 128 instants; then the
multi-view rig pose of 100 fresh instants is solved under the fitted set and under the planted set, and its error against the planted
rig pose is compared (rotation in degrees, translation in mm; median / 90th percentile).  One seed, reported only.

    python tools/cam_fit_study.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cam_fit_shapes as sh  # noqa: E402
import cam_fit_statement as cf  # noqa: E402
import mv_statement as mv  # noqa: E402
import pose_statement as ps  # noqa: E402
from pose_testlib import golden_camera_and_model  # noqa: E402
from rig_fit_shapes import rig_truth  # noqa: E402

FIT_FROM = (8, 16, 64, 128)
FRESH = 100
NOISE = 0.2


def instants(n_cameras, angles, n, seed):
    K, dist = golden_camera_and_model()[:2]
    b = sh._Builder(seed, rig_truth(3, 12), [0, 0, 0], n_cameras, NOISE)
    b.cameras = [(K, dist)] * n_cameras
    b.poses = mv.ring_poses(sh.CENTRE, angles)
    b.limit = 0.3   # mv_study.py's rig fills more of the frame than the test cases do
    for _ in range(n):
        b.instant({c: [(m, int(b.rng.integers(2, 6))) for m in range(3)] for c in range(n_cameras)})
    return b.finish("study", 1, {})


def errors(b, first, count, R, t, anchor):
    """Rig pose errors on instants first .. first + count - 1 under the camera state (R, t) in the anchor's frame."""
    sub = dict(b, recs=b["recs"][:, first:first + count], planted={(f - first, g): p for (f, g), p in b["planted"].items() if first <= f < first + count})
    O = cf.Observations(sub["recs"], b["model"], b["rig_of_model"], 1, b["cameras"], list(range(len(b["cameras"]))))
    want = sh.planted_rig_poses(sub, O, anchor)
    got = O.solve_poses(R, t, want)
    rot = np.array([np.degrees(np.linalg.norm(mv.rotvec(ps.rodrigues(g[:3]) @ ps.rodrigues(w[:3]).T))) for g, w in zip(got, want)])
    tr = np.linalg.norm(got[:, 3:] - want[:, 3:], axis=1)
    return rot, tr


def main():
    for angles in ((-25.0, 25.0), (-45.0, -15.0, 15.0, 45.0)):
        nc = len(angles)
        b = instants(nc, angles, max(FIT_FROM) + FRESH, 7)
        placed = list(range(nc))
        Rp, tp = sh.planted_set(b, placed, 0)
        rot, tr = errors(b, max(FIT_FROM), FRESH, Rp, tp, 0)
        print("%d cameras, planted set: rotation %.3f / %.3f deg, translation %.3f / %.3f mm" % (nc, np.median(rot), np.percentile(rot, 90), np.median(tr),
                                                                                             np.percentile(tr, 90)))
        for n in FIT_FROM:
            sub = dict(b, recs=b["recs"][:, :n], planted={k: v for k, v in b["planted"].items() if k[0] < n})
            rr = cf.rig_records(sub["recs"], b["model"], b["rig_of_model"], 1, b["cameras"], sh.planted_start(sub))
            init = cf.initial_assembly(rr, nc, n)
            assert init["placed"] == placed and init["anchor"] == 0
            O = cf.Observations(sub["recs"], b["model"], b["rig_of_model"], 1, b["cameras"], placed)
            out = cf.fit(O, np.array([init["T"][c][0] for c in placed]), np.array([init["T"][c][1] for c in placed]), 0, sh.planted_rig_poses(sub, O, 0))
            d = sh.set_distance(out["R"], out["t"], Rp, tp)
            rot, tr = errors(b, max(FIT_FROM), FRESH, out["R"], out["t"], 0)
            print("%d cameras, fitted from %3d instants (%d rounds, set %.2e rad %.2e of the distance from the planted): rotation %.3f / %.3f deg, "
                  "translation %.3f / %.3f mm" % (nc, n, out["rounds"], d[0], d[1], np.median(rot), np.percentile(rot, 90), np.median(tr), np.percentile(tr, 90)))


if __name__ == "__main__":
    main()
