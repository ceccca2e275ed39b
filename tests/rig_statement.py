"""An independent statement of the rig pose (k_rig_count, k_rig_solve<160,64>, k_rig_solve<800,256>; include/ctag_pose.h, the
rig section), in numpy / scipy only.

Nothing here comes from oracle/, cylindertag_amd/csrc, testkit or rig_testlib.compose_rig_poses.  It reuses pose_statement.py's
correspondences, model_lookup, rodrigues and Problem.  A detection record is read through the field names of its dtype, a model is
{"ids", "size", "corners"}, a camera (K 3x3, dist[n_dist]).

  membership         rule 2: markers 0 .. clamp(n_markers, 0, 100)-1 in order; the first model with the id; rig_of_model; the
                     first marker with an id claims it, whatever became of that marker; builder rejection; the 800-point bound,
                     where an excluded member does not end the scan.  A frame that is not CTAG_OK has no member and no exclusion.
  expected_header    status, rig, frame, n_members, n_excluded, n_points, member_mask, reserved
  check_rig_records  what ctag_rig_pose_rec records must satisfy

EPnP and the LM loop are NOT restated step by step: check_rig_records states what they must reach."""
import numpy as np

from pose_statement import MIN_POINTS_FOR_MINIMUM, Problem, correspondences, model_lookup, rodrigues

OK, TOO_FEW, DEGENERATE, NOT_SEEN = 0, 2, 4, 5
MAX_MARKERS = 100
RIG_MAX_POINTS = 800
RIG_POSE_DT = np.dtype([("status", "<i4"), ("rig", "<i4"), ("frame", "<i4"), ("n_members", "<i4"), ("n_excluded", "<i4"),
                        ("n_points", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"), ("member_mask", "<u4", (4,)),
                        ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("rvec0", "<f8", (3,)), ("tvec0", "<f8", (3,)),
                        ("cost0", "<f8"), ("cost", "<f8")])
HEADER_FIELDS = ("status", "rig", "frame", "n_members", "n_excluded", "n_points", "member_mask", "reserved")
POSE_FIELDS = ("iterations", "rvec", "tvec", "rvec0", "tvec0", "cost0", "cost")


def membership(rec, model, rig_of_model, g):
    """Rule 2 for rig g in one detection record.  Returns (members [marker indices], excluded count, obj float32 [n,3],
    img float32 [n,2]), the points concatenated in marker order."""
    members, excluded, objs, imgs, total = [], 0, [], [], 0
    if int(rec["status"]) == 0:
        claimed = set()
        for k in range(min(max(int(rec["n_markers"]), 0), MAX_MARKERS)):
            marker_id = int(rec["markers"][k]["marker_id"])
            mi = model_lookup(model, marker_id)
            if mi < 0 or int(rig_of_model[mi]) != g:
                continue
            first = marker_id not in claimed
            claimed.add(marker_id)
            if not first:
                excluded += 1
                continue
            st, obj, img = correspondences(rec, k, model, mi)
            if st != OK or total + len(obj) > RIG_MAX_POINTS:
                excluded += 1
                continue
            members.append(k)
            objs.append(obj)
            imgs.append(img)
            total += len(obj)
    obj = np.concatenate(objs) if objs else np.zeros((0, 3), np.float32)
    img = np.concatenate(imgs) if imgs else np.zeros((0, 2), np.float32)
    return members, excluded, obj, img


def expected_header(rec, model, rig_of_model, g, frame):
    """The integer fields of the record of (frame, rig g) as a RIG_POSE_DT record with zero pose fields, and the concatenated
    (obj, img).  Status OK stands for "EPnP + PoseBA run" (OK or DEGENERATE)."""
    members, excluded, obj, img = membership(rec, model, rig_of_model, g)
    H = np.zeros((), RIG_POSE_DT)
    H["rig"], H["frame"], H["n_members"], H["n_excluded"], H["n_points"] = g, frame, len(members), excluded, len(obj)
    for k in members:
        H["member_mask"][k >> 5] |= np.uint32(1 << (k & 31))
    H["status"] = NOT_SEEN if not members else (TOO_FEW if len(obj) < 4 else OK)
    return H, obj, img


last_stats = {}  # worst figures of the most recent check_rig_records call, for reports


def check_rig_records(got, recs, model, rig_of_model, n_rigs, camera, degenerate=None, planted=None, max_minimum_checks=None):
    """Asserts that `got` (len(recs) * n_rigs ctag_rig_pose_rec records, record f * n_rigs + g) are the rig poses of the detection
    records `recs` under `model`, `rig_of_model` and `camera` = (K, dist):

      1. every header field (status, rig, frame, n_members, n_excluded, n_points, member_mask, reserved) equals the statement's.
         DEGENERATE is accepted exactly where degenerate(frame, rig) says so; there, and for every status but OK, all pose fields
         are zero.
      2. status OK: |cost0 - cost_at(rvec0, tvec0)| and |cost - cost_at(rvec, tvec)| <= 1e-9 * max(1, cost) over the
         concatenated points; cost <= cost0; 0 <= iterations <= 50.
      3. status OK and n_points >= 16: cost <= min.cost * (1 + 1e-9) + 1e-12, |rvec - min.x[:3]| < 1e-6,
         |tvec - min.x[3:]| < 1e-4 * max|tvec|, min = Problem.minimum_from(rvec0, tvec0).  With max_minimum_checks the eligible
         records are thinned evenly to about that many, but every distinct n_points keeps at least one checked record.
      4. planted[frame][rig] = (rvec, tvec) given (noise-free input), n_points >= 16: |R(rvec0) - R(planted)| < 2e-4 per entry
         and |tvec0 - planted| < 0.2, and the same of (rvec, tvec).

    The bars are pose_statement.check_pose_records' own.  Returns how many records got check 3."""
    K, dist = camera
    degenerate = degenerate or (lambda frame, rig: False)
    assert len(got) == len(recs) * n_rigs, "%d records for %d items" % (len(got), len(recs) * n_rigs)
    stats = {"records": len(got), "ok": 0, "minimum_checks": 0, "planted_checks": 0, "cost_rel": 0.0, "min_cost_excess": 0.0,
             "drvec": 0.0, "dtvec_rel": 0.0, "planted_dR": 0.0, "planted_dt": 0.0, "checked_sizes": set()}
    problems = {}
    for f in range(len(recs)):
        for g in range(n_rigs):
            w = f * n_rigs + g
            P = got[w]
            what = "frame %d rig %d" % (f, g)
            H, obj, img = expected_header(recs[f], model, rig_of_model, g, f)
            st = int(H["status"])
            if st == OK and degenerate(f, g):
                st = DEGENERATE
            assert int(P["status"]) == st, (what, "status", int(P["status"]), st)
            for k in HEADER_FIELDS[1:]:
                assert np.array_equal(P[k], H[k]), (what, k, P[k], H[k])
            if st != OK:
                for k in POSE_FIELDS:
                    assert not np.any(P[k]), (what, k, "set on status %d" % st)
                continue
            problems[w] = Problem(K, dist, obj, img)
    stats["ok"] = len(problems)
    for w, pb in problems.items():
        P = got[w]
        what = "frame %d rig %d (%d points)" % (int(P["frame"]), int(P["rig"]), int(P["n_points"]))
        assert len(pb.X) == int(P["n_points"]), what
        assert 0 <= int(P["iterations"]) <= 50, what
        assert P["cost"] <= P["cost0"], (what, float(P["cost"]), float(P["cost0"]))
        for ck, rk, tk in (("cost0", "rvec0", "tvec0"), ("cost", "rvec", "tvec")):
            d = abs(pb.cost_at(P[rk], P[tk]) - float(P[ck])) / max(1.0, float(P["cost"]))
            stats["cost_rel"] = max(stats["cost_rel"], d)
            assert d <= 1e-9, (what, ck, d)
    eligible = [w for w in problems if int(got[w]["n_points"]) >= MIN_POINTS_FOR_MINIMUM]
    if max_minimum_checks is not None and len(eligible) > max_minimum_checks:
        pick = set(int(i) for i in np.unique(np.linspace(0, len(eligible) - 1, max_minimum_checks).round().astype(int)))
        sizes = set(int(got[eligible[i]]["n_points"]) for i in pick)
        for i, w in enumerate(eligible):  # the first record of every size the even spread left out
            if int(got[w]["n_points"]) not in sizes:
                pick.add(i)
                sizes.add(int(got[w]["n_points"]))
        eligible = [eligible[i] for i in sorted(pick)]
    for w in eligible:
        P, pb = got[w], problems[w]
        what = "frame %d rig %d (%d points)" % (int(P["frame"]), int(P["rig"]), int(P["n_points"]))
        sol = pb.minimum_from(P["rvec0"], P["tvec0"])
        dr = float(np.abs(P["rvec"] - sol.x[:3]).max())
        dt = float(np.abs(P["tvec"] - sol.x[3:]).max() / np.abs(P["tvec"]).max())
        stats["min_cost_excess"] = max(stats["min_cost_excess"], (float(P["cost"]) - sol.cost) / max(sol.cost, 1e-300))
        stats["drvec"], stats["dtvec_rel"] = max(stats["drvec"], dr), max(stats["dtvec_rel"], dt)
        assert P["cost"] <= sol.cost * (1 + 1e-9) + 1e-12, (what, float(P["cost"]), sol.cost)
        assert dr < 1e-6, (what, "rvec", dr)
        assert dt < 1e-4, (what, "tvec", dt)
        stats["minimum_checks"] += 1
        stats["checked_sizes"].add(int(P["n_points"]))
    if planted is not None:
        for w in problems:
            P = got[w]
            if int(P["n_points"]) < MIN_POINTS_FOR_MINIMUM or planted[int(P["frame"])] is None:
                continue
            truth = planted[int(P["frame"])][int(P["rig"])]
            if truth is None:
                continue
            what = "frame %d rig %d (%d points)" % (int(P["frame"]), int(P["rig"]), int(P["n_points"]))
            for rk, tk in (("rvec0", "tvec0"), ("rvec", "tvec")):
                dr = float(np.abs(rodrigues(P[rk]) - rodrigues(truth[0])).max())
                dt = float(np.abs(P[tk] - truth[1]).max())
                stats["planted_dR"], stats["planted_dt"] = max(stats["planted_dR"], dr), max(stats["planted_dt"], dt)
                assert dr < 2e-4, (what, "planted rotation", rk, dr)
                assert dt < 0.2, (what, "planted translation", tk, dt)
            stats["planted_checks"] += 1
    last_stats.clear()
    last_stats.update(stats)
    return stats["minimum_checks"]


def report(what):
    """One line: the counts and the worst figures of the most recent check_rig_records call."""
    s = last_stats
    return ("%s: %d records, %d OK, %d held against scipy (%d sizes), %d against planted poses; worst cost mismatch %.1e (relative), "
            "cost above the minimum %.1e, |d rvec| %.1e, |d tvec|/|t| %.1e; planted |d R| %.1e, |d t| %.1e" %
            (what, s["records"], s["ok"], s["minimum_checks"], len(s["checked_sizes"]), s["planted_checks"], s["cost_rel"],
             s["min_cost_excess"], s["drvec"], s["dtvec_rel"], s["planted_dR"], s["planted_dt"]))
