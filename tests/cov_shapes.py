"""Source pose records and their detection records for the pose covariance (k_pose_cov.hip), shared by
tests/test_cov_statement_cpu.py (which measures the statement's own float64 error on them: cov_statement.MEASURED_F64_DEVIATION)
and tests/test_pose_cov_gpu.py (the device): both build the same cases here.

A case is {"kind": "marker" | "rig" | "mv", "name", "recs", "model", "cameras", "camera_poses", "sources", "n_rigs"}: recs is the
detection record array [n_frames] (mv: [n_cameras][n_frames]); sources the pose records of the kind's dtype, hand-built: planted
poses on pixels with 0.2 px noise, the headers by rig_statement / mv_statement, cost by the statements' residuals.  Every builder
is deterministic.  Nothing here touches the oracle or the device.

  marker_case     per-marker point counts 4 8 60 64 68 96 160 (fewer points than lanes, the lane-stride boundary, both model
                  sizes of k_pose's tiers), a second marker in every frame; one planted 5 px outlier
  rig_case        rig point counts 164 256 796 800 (uneven points per lane, the bound)
  mv_cases        two cameras with 8 + 8 points; three cameras with their own intrinsics and n_dist 0, 5, 12; eight cameras; the
                  virtual split: three equal cameras at the reference that share out the markers of a rig record
  rules_case      every source status, every cause of CTAG_COV_BAD_RECORD, four coincident points and a collinear set"""
import numpy as np

import cov_statement as cs
import mv_statement as ms
import pose_statement as ps
import rig_statement as rs
from ctag_testlib import RESULT_DT
from mv_testlib import synth_mv_instant
from pose_testlib import POSE_DT, golden_camera_and_model, make_cylinder_model, test_cameras
from rig_shapes import FULL, HALF, _pixels, _place, _place_rig, _pose, layout
from rig_testlib import cylinder_model

MARKER_COUNTS = (4, 8, 60, 64, 68, 96, 160)
RIG_COUNTS = (164, 256, 796, 800)
OUTLIER_PX = 5.0
ZERO_POSE = (np.zeros(3), np.zeros(3))
GRID = 4096  # wavefronts of one k_pose_cov launch at most


def marker_patterns(n):
    """The features of one marker with exactly n = 8a + 4b points: the 4-point feature second, where the end-feature rule cannot
    skip it."""
    full, half = n // 8, (n % 8) // 4
    p = [FULL] * (full + half)
    if half:
        p[min(1, len(p) - 1)] = HALF
    return p


def _fill_costs(case):
    """cost of every OK source record whose points can be rebuilt: the statements' residual at the record's pose."""
    for P in case["sources"]:
        if int(P["status"]) != 0:
            continue
        if case["kind"] == "marker":
            parts = cs.parts_of_marker(P, case["recs"], case["model"])
        elif case["kind"] == "rig":
            parts = cs.parts_of_rig(P, case["recs"], case["model"])
        else:
            parts = cs.parts_of_mv(P, case["recs"], case["model"])
        if parts is None:
            continue
        pb = ms.MvProblem(case["cameras"], case["camera_poses"], parts)
        with np.errstate(all="ignore"):
            P["cost"] = pb.cost_at(P["rvec"], P["tvec"])
    return case


def marker_case(size, dist_name, counts=MARKER_COUNTS, outlier_at=64, seed=0):
    """One frame per count: marker 0 is a marker of that many points of model (frame % 3), marker 1 one of 16 points of the next
    model.  The marker of `outlier_at` points has OUTLIER_PX added to u of corner 4 of its feature 2 (point 18 of the builder's
    order)."""
    K, golden_dist, _ = golden_camera_and_model()
    dist = golden_dist if dist_name == "golden" else test_cameras()[dist_name]
    model = make_cylinder_model(3, size)
    rng = np.random.default_rng(1400 + size + seed)
    recs = np.zeros(len(counts), RESULT_DT)
    src = []
    for f, n in enumerate(counts):
        for m, (mi, pat) in enumerate(((f % 3, marker_patterns(n)), ((f + 1) % 3, [FULL, FULL]))):
            pose = _pose(rng, model["corners"][mi])
            p0 = int(rng.integers(0, size - len(pat) + 1))
            k = _place(recs[f], int(model["ids"][mi]), _pixels(rng, model, mi, K, dist, pose, 0.2), p0, pat)
            if m == 0 and n == outlier_at:
                recs[f]["features"][int(recs[f]["markers"][k]["first_feature"]) + 2]["corners"][2 * 4] += np.float32(OUTLIER_PX)
            P = np.zeros((), POSE_DT)
            P["model_index"], P["frame"], P["marker"], P["n_points"] = mi, f, k, n if m == 0 else 16
            P["rvec"], P["tvec"] = pose
            src.append(P)
    return _fill_costs({"kind": "marker", "name": "marker size %d %s" % (size, dist_name), "recs": recs, "model": model, "cameras": [(K, dist)],
                        "camera_poses": [ZERO_POSE], "sources": np.array(src), "n_rigs": None, "outlier": (counts.index(outlier_at) * 2, 18)
                        if outlier_at in counts else None})


def rig_case(dist_name="golden", counts=RIG_COUNTS):
    """One rig, one frame per count, members by rig_shapes.layout over markers of 20 columns."""
    K, golden_dist, _ = golden_camera_and_model()
    dist = golden_dist if dist_name == "golden" else test_cameras()[dist_name]
    model = cylinder_model(6, 20)
    rig_of_model = np.zeros(6, np.int32)
    rng = np.random.default_rng(1450)
    recs = np.zeros(len(counts), RESULT_DT)
    src = np.zeros(len(counts), rs.RIG_POSE_DT)
    for f, n in enumerate(counts):
        members = layout(n, 20)
        pose = _pose(rng, model["corners"][:len(members)])
        _place_rig(recs[f], rng, model, range(len(members)), members, K, dist, pose, 0.2)
        src[f] = rs.expected_header(recs[f], model, rig_of_model, 0, f)[0]
        assert src[f]["status"] == 0 and src[f]["n_points"] == n
        src[f]["rvec"], src[f]["tvec"] = pose
    return _fill_costs({"kind": "rig", "name": "rig %s" % dist_name, "recs": recs, "model": model, "cameras": [(K, dist)], "camera_poses": [ZERO_POSE],
                        "sources": src, "n_rigs": 1, "rig_of_model": rig_of_model})


def _mv_case(name, model, rig_of_model, n_rigs, cameras, poses, recs, truths):
    """recs[f][c] -> the case; truths[f][g] the planted poses."""
    recs = np.array([[recs[f][c] for f in range(len(recs))] for c in range(len(cameras))])
    src = np.zeros(recs.shape[1] * n_rigs, ms.MV_POSE_DT)
    for f in range(recs.shape[1]):
        for g in range(n_rigs):
            H = ms.expected_header([recs[c][f] for c in range(len(cameras))], model, rig_of_model, g, f)[0]
            src[f * n_rigs + g] = H
            if H["status"] == 0:
                src[f * n_rigs + g]["rvec"], src[f * n_rigs + g]["tvec"] = truths[f][g]
    return _fill_costs({"kind": "mv", "name": name, "recs": recs, "model": model, "cameras": cameras, "camera_poses": poses, "sources": src,
                        "n_rigs": n_rigs, "rig_of_model": rig_of_model})


def _own_cameras(n, K, dist_names):
    tc = test_cameras()
    out = []
    for c in range(n):
        Kc = K.copy()
        s = 0.85 + 0.05 * c
        Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2] = K[0, 0] * s, K[1, 1] * (s + 0.01), K[0, 2] + 11 * c, K[1, 2] - 7 * c
        out.append((Kc, tc[dist_names[c % len(dist_names)]]))
    return out


def mv_cases():
    K, dist, golden = golden_camera_and_model()
    rig_of_model = np.zeros(len(golden["ids"]), np.int32)
    centre = golden["corners"].reshape(-1, 3).astype(np.float64).mean(0)
    rng = np.random.default_rng(1470)
    cases = []
    # two cameras, one 8-point feature of one marker each
    poses = ms.ring_poses(centre, [-20.0, 25.0])
    inst = [synth_mv_instant(rng, golden, [[0]], [(K, dist)] * 2, poses, 0.2, feats=(1, 1), patterns=(FULL,)) for _ in range(2)]
    c = _mv_case("mv 8 + 8", golden, np.array([0, -1, -1, -1, -1, -1], np.int32), 1, [(K, dist)] * 2, poses, [i[0] for i in inst], [i[1] for i in inst])
    assert [int(v) for v in c["sources"]["n_points"]] == [16, 16]
    cases.append(c)
    # three cameras with their own intrinsics, n_dist 0, 5, 12; two rigs
    cams = _own_cameras(3, K, ("n_dist0", "n_dist5", "n_dist12"))
    poses = ms.ring_poses(centre, [-35.0, 0.0, 40.0], shifts=[(10.0, -5.0, 30.0), (0.0, 0.0, 0.0), (-20.0, 8.0, 60.0)])
    two = np.array([0, 0, 0, 1, 1, 1], np.int32)
    inst = [synth_mv_instant(rng, golden, [[0, 1, 2], [3, 4, 5]], cams, poses, 0.2) for _ in range(3)]
    cases.append(_mv_case("mv three own cameras", golden, two, 2, cams, poses, [i[0] for i in inst], [i[1] for i in inst]))
    # eight cameras
    cams = _own_cameras(8, K, ("n_dist0", "n_dist5", "n_dist8", "n_dist12"))
    poses = ms.ring_poses(centre, [(i - 3.5) * 14.0 for i in range(8)])
    inst = [synth_mv_instant(rng, golden, [list(range(6))], cams, poses, 0.2, feats=(1, 3)) for _ in range(2)]
    cases.append(_mv_case("mv eight cameras", golden, rig_of_model, 1, cams, poses, [i[0] for i in inst], [i[1] for i in inst]))
    return cases


def virtual_split(rig):
    """The markers of every frame of rig_case's records shared out, in order, to three equal cameras at the reference: camera c gets
    a contiguous third.  The mv source record has the rig record's pose and cost.  Its covariance record must be the rig record's,
    byte for byte."""
    recs = np.zeros((3, len(rig["recs"])), RESULT_DT)
    for f, r in enumerate(rig["recs"]):
        nm = int(r["n_markers"])
        cuts = [0, (nm + 2) // 3, (2 * nm + 2) // 3, nm]
        for c in range(3):
            o = recs[c][f]
            for k in range(cuts[c], cuts[c + 1]):
                M = r["markers"][k]
                f0, nf = int(o["n_features"]), int(M["n_features"])
                o["markers"][int(o["n_markers"])] = (M["marker_id"], f0, nf, M["n_pos"])
                o["features"][f0:f0 + nf] = r["features"][int(M["first_feature"]):int(M["first_feature"]) + nf]
                o["n_markers"], o["n_features"] = int(o["n_markers"]) + 1, f0 + nf
    cams, poses = [rig["cameras"][0]] * 3, [ZERO_POSE] * 3
    src = np.zeros(len(rig["sources"]), ms.MV_POSE_DT)
    for f, S in enumerate(rig["sources"]):
        src[f] = ms.expected_header([recs[c][f] for c in range(3)], rig["model"], rig["rig_of_model"], 0, f)[0]
        assert src[f]["status"] == 0 and src[f]["n_points"] == S["n_points"]
        src[f]["rvec"], src[f]["tvec"], src[f]["cost"] = S["rvec"], S["tvec"], S["cost"]
    return {"kind": "mv", "name": "mv virtual split", "recs": recs, "model": rig["model"], "cameras": cams, "camera_poses": poses, "sources": src,
            "n_rigs": 1, "rig_of_model": rig["rig_of_model"]}


def rules_case():
    """Per-marker source records over two frames (frame 1 is not CTAG_OK) of a model list whose model 1 is collinear and whose model
    2 has all corners of a feature in one point.  "expect" lists the status every record must get."""
    K, dist, _ = golden_camera_and_model()
    model = make_cylinder_model(3, 12)
    model["corners"] = model["corners"].copy()
    model["corners"][1][:, 1:] = 0.0     # collinear: along the model's x axis
    for p in range(12):                  # coincident: the eight corners of a feature in its first corner
        model["corners"][2][p * 8:p * 8 + 8] = model["corners"][2][p * 8]
    rng = np.random.default_rng(1490)
    recs = np.zeros(2, RESULT_DT)
    poses = [_pose(rng, model["corners"][mi]) for mi in range(3)]
    # the line seen without a rotation: turning about it moves no point, the first rotation column of J is exactly zero in both
    # parametrisations.  (A line seen obliquely leaves a last pivot of about +-1e-11, rounding of a rank-5 matrix: the 1e-12
    # threshold does not classify it one way or the other, so it is not a test case.)
    poses[1] = (np.zeros(3), np.array([5.0, -3.0, 480.0]))
    r = recs[0]
    _place(r, 0, _pixels(rng, model, 0, K, dist, poses[0], 0.2), 3, [FULL, FULL])   # marker 0: 16 points
    _place(r, 1, _pixels(rng, model, 1, K, dist, poses[1], 0.2), 2, [FULL, FULL])   # marker 1: collinear
    _place(r, 2, _pixels(rng, model, 2, K, dist, poses[2], 0.2), 5, [HALF])         # marker 2: four coincident points
    m = _place(r, 0, _pixels(rng, model, 0, K, dist, poses[0], 0.2), 3, [FULL, FULL])
    r["features"][int(r["markers"][m]["first_feature"]) + 1]["pos"] = 12             # marker 3: the builder rejects it
    recs[1] = recs[0]
    recs[1]["status"] = 1

    def rec(marker, mi, n, frame=0, status=0, pose=None):
        P = np.zeros((), POSE_DT)
        P["status"], P["model_index"], P["frame"], P["marker"], P["n_points"] = status, mi, frame, marker, n
        P["rvec"], P["tvec"] = poses[mi % 3] if pose is None else pose
        return P

    nan_pose = (np.array([0.1, np.nan, 0.0]), poses[0][1])
    inf_pose = (poses[0][0], np.array([0.0, 0.0, np.inf]))
    items = [(rec(0, 0, 16), cs.COV_OK)]
    items += [(rec(0, 0, 16, status=s), cs.COV_NO_POSE) for s in (1, 2, 3, 4, 5)]
    items += [(rec(0, 0, 16, frame=5, status=2), cs.COV_NO_POSE)]        # a record without a pose is not looked at further
    items += [(rec(0, 0, 16, frame=2), cs.COV_BAD_RECORD), (rec(0, 0, 16, frame=-1), cs.COV_BAD_RECORD),   # frame outside the batch
              (rec(4, 0, 16), cs.COV_BAD_RECORD), (rec(-1, 0, 16), cs.COV_BAD_RECORD),                     # marker outside the frame
              (rec(0, 3, 16), cs.COV_BAD_RECORD), (rec(0, -1, 16), cs.COV_BAD_RECORD),                     # model outside the list
              (rec(0, 0, 16, frame=1), cs.COV_BAD_RECORD),                                                 # the frame is not CTAG_OK
              (rec(3, 0, 16), cs.COV_BAD_RECORD),                                                          # the builder rejects the marker
              (rec(0, 0, 12), cs.COV_BAD_RECORD),                                                          # another point count
              (rec(0, 0, 16, pose=nan_pose), cs.COV_BAD_RECORD), (rec(0, 0, 16, pose=inf_pose), cs.COV_BAD_RECORD),
              (rec(2, 2, 4), cs.COV_SINGULAR), (rec(1, 1, 16), cs.COV_SINGULAR)]
    case = {"kind": "marker", "name": "rules", "recs": recs, "model": model, "cameras": [(K, dist)], "camera_poses": [ZERO_POSE],
            "sources": np.array([i[0] for i in items]), "n_rigs": None, "expect": [i[1] for i in items]}
    return _fill_costs(case)


def rig_rules(rig):
    """rig_case's first record bent three ways: a member bit past the frame's markers, a member whose id has no model (the caller
    passes recs_unknown), a frame outside the batch; and every source status without a pose."""
    S = rig["sources"][0]
    out, expect = [S.copy()], [cs.COV_OK]
    a = S.copy()
    a["member_mask"][3] |= np.uint32(1 << 31)
    b = S.copy()
    b["frame"] = len(rig["recs"])
    out += [a, b]
    expect += [cs.COV_BAD_RECORD, cs.COV_BAD_RECORD]
    for s in (2, 4, 5):
        c = S.copy()
        c["status"] = s
        out.append(c)
        expect.append(cs.COV_NO_POSE)
    recs = rig["recs"].copy()
    case = dict(rig, name="rig rules", sources=np.array(out), expect=expect, recs=recs)
    # the last record: frame 1 with the id of its first marker changed to one no model has
    d = rig["sources"][1].copy()
    case["recs"][1]["markers"][0]["marker_id"] = 77
    case["sources"] = np.concatenate([case["sources"], np.array([d])])
    case["expect"] = expect + [cs.COV_BAD_RECORD]
    return case


def mv_rules(mv):
    """An mv case's first record with a member mask on a camera the set does not have."""
    S = mv["sources"][0]
    a = S.copy()
    a["member_mask"][len(mv["cameras"])][0] = 1
    b = S.copy()
    b["status"] = 5
    return dict(mv, name="mv rules", sources=np.array([S.copy(), a, b]), expect=[cs.COV_OK, cs.COV_BAD_RECORD, cs.COV_NO_POSE],
                n_rigs=3, recs=mv["recs"][:, :1])


def all_cases():
    """Every case the GPU tests run, in one list (the CPU test measures the statement's float64 error over all of them)."""
    rig = rig_case()
    mv = mv_cases()
    return ([marker_case(20, "golden"), marker_case(12, "n_dist8", counts=(4, 8, 60, 64, 68, 96)), marker_case(16, "n_dist12", counts=(4, 68, 96), outlier_at=0),
             rig, rig_case("n_dist12", counts=(164, 800))] + mv + [virtual_split(rig), rules_case(), rig_rules(rig), mv_rules(mv[0])])


def expected_of(case, opts, ft=np.float64):
    """The statement's dicts for every source record of a case."""
    cam = case["cameras"][0]
    if case["kind"] == "marker":
        return [cs.expected_marker(P, case["recs"], case["model"], cam, opts, ft) for P in case["sources"]]
    if case["kind"] == "rig":
        return [cs.expected_rig(P, case["recs"], case["model"], cam, opts, ft) for P in case["sources"]]
    return [cs.expected_mv(P, case["recs"], case["model"], case["cameras"], case["camera_poses"], opts, ft) for P in case["sources"]]
