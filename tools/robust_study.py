"""What the robust refit is worth, on the CPU (no GPU): planted detections of the golden model under the golden
camera, as tools/rig_study.py plants them, 0.2 px of pixel noise, and ONE feature whose 8 corners are moved together by `shift`
pixels in a random direction -- a half-occluded feature, or corners refined onto a neighbouring edge.  Per case the least-squares
pose (the statement's loop with every weight 1, from the planted pose: what the pose call returns), then the refit of
tests/robust_statement.py from it under Huber and under Cauchy with the default options.  Reported per case: the median rotation
error (degrees) and translation error (model units) of the three poses against the planted one, in how many trials Cauchy's pose is
closer to the planted rotation than the least-squares pose, and in how many Cauchy's inlier set is exactly the clean points.

    python tools/robust_study.py --trials 200
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

import cov_statement as cs  # noqa: E402
import rig_statement as rs  # noqa: E402
import robust_statement as rb  # noqa: E402
from pose_testlib import golden_camera_and_model  # noqa: E402
from rig_testlib import rot_err_deg, stacked_rig_model, synth_rig_frame  # noqa: E402


def trial(rng, model, rig, K, dist, features, shift):
    """One planted frame: ((rotation error, translation error) of plain / Huber / Cauchy, Cauchy's inlier set is the clean set)."""
    rec, truth = synth_rig_frame(rng, model, [rig], K, dist, 0.2, feats=(features, features))
    k = int(rng.integers(0, int(rec["n_markers"])))
    j = int(rec["markers"][k]["first_feature"]) + int(rng.integers(0, features))
    th = rng.uniform(0, 2 * np.pi)
    rec["features"][j]["corners"] += np.tile(np.float32([shift * np.cos(th), shift * np.sin(th)]), 8)
    rig_of_model = np.full(len(model["ids"]), -1, np.int32)
    rig_of_model[rig] = 0
    H, obj, img = rs.expected_header(rec, model, rig_of_model, 0, 0)
    pp = cs.problem_parts([(0, obj, img)], [(K, dist)], [cs.IDENTITY_POSE])
    planted = np.zeros(len(obj), bool)  # the moved points, in the builder's order: members in marker order, features in order, 8 each
    at = 0
    for m in range(int(rec["n_markers"])):
        f0 = int(rec["markers"][m]["first_feature"])
        if f0 <= j < f0 + features:
            planted[at + (j - f0) * 8:at + (j - f0) * 8 + 8] = True
        at += features * 8
    ls = rb.refit(pp, truth[0][0], truth[0][1], rb.default_opts(loss=rb.HUBER, scale_px=1e9))
    out = [ls] + [rb.refit(pp, ls["rvec"], ls["tvec"], rb.default_opts(loss=loss)) for loss in (rb.HUBER, rb.CAUCHY)]
    errs = [(rot_err_deg(e["rvec"], truth[0][0]), float(np.linalg.norm(e["tvec"] - truth[0][1]))) for e in out]
    inl = np.array([bool(out[2]["inlier_mask"][i >> 5] >> (i & 31) & 1) for i in range(len(obj))])
    return errs, bool(np.array_equal(~inl, planted))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--trials", type=int, default=200)
    a = ap.parse_args()
    K, dist, golden = golden_camera_and_model()
    stacked = stacked_rig_model(golden, 3, 70.0)
    cases = [("marker", golden, [0], f) for f in (2, 3, 4, 5, 6, 8, 10)] + [("rig of 3", stacked, [0, 1, 2], f) for f in (2, 3, 5)]
    for what, model, rig, features in cases:
        for shift in (5.0, 2.0):
            rng = np.random.default_rng(1900 + features)
            t0 = time.time()
            got = [trial(rng, model, rig, K, dist, features, shift) for _ in range(a.trials)]
            E = np.array([g[0] for g in got])  # trials x (plain, huber, cauchy) x (rot, transl)
            med = np.median(E, 0)
            print(json.dumps({"what": what, "features_per_marker": features, "points": 8 * features * len(rig), "moved_points": 8, "shift_px": shift,
                              "trials": a.trials, "median_rot_deg": [round(float(v), 4) for v in med[:, 0]],
                              "median_transl": [round(float(v), 3) for v in med[:, 1]],
                              "cauchy_beats_plain": round(float((E[:, 2, 0] < E[:, 0, 0]).mean()), 3),
                              "cauchy_inliers_are_the_clean_points": round(float(np.mean([g[1] for g in got])), 3),
                              "seconds": round(time.time() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
