"""Record batches for the rig pose (k_rig_pose.hip), shared by tests/test_rig_statement_cpu.py (the oracle's composition) and
tests/test_rig_forms_gpu.py (the device): both build the same batches here, so what the statement accepts from the oracle is what
it is asked about the kernels.

Every builder is deterministic and returns {"recs", "model", "rig_of_model", "n_rigs", "K", "dist", "planted"}; planted[f] is
None or one (rvec, tvec) per rig (noise-free frames).  Pixels come from pose_statement.project12, expectations from
tests/rig_statement.py: nothing here touches the oracle.

  size_edges          one rig per frame at every point count next to 64, 128, 160 (the switch of work lists), 256, 512, 768, 800
  stride_batch        more items than twice either solve grid in one call, of nine kinds in a fixed permutation
  count_stride_batch  just over 1024 x 256 (frame, rig) items: k_rig_count's own stride
  rule_batch          member_mask words 1-3, the clamp of n_markers, the bound that skips and then fits, duplicates, markers
                      that point outside the record, a model list with one id twice, members without points"""
import numpy as np

import rig_statement as rs
from ctag_testlib import RESULT_DT
from pose_statement import project12, rodrigues
from pose_testlib import golden_camera_and_model, planar_model
from rig_testlib import cylinder_model

FULL, HALF = (3, 4), (7, 4)  # id pairs: 8 points; 4 points (skipped at the ends of a marker of more than three features)
SMALL_COUNTS = (4, 8, 60, 64, 68, 124, 128, 132, 156, 160)
LARGE_COUNTS = (164, 168, 252, 256, 260, 508, 512, 516, 764, 768, 772, 796, 800)
SMALL_GRID, LARGE_GRID = 4096, 256  # workgroups of k_rig_solve<160,64> and k_rig_solve<800,256> at most
COUNT_GRID = 1024 * 256             # threads of k_rig_count at most


def _pose(rng, X, rot_sigma=0.1, shift=(20.0, 20.0, 40.0)):
    """A random pose that keeps the points X about where they are."""
    centre = np.asarray(X, np.float64).reshape(-1, 3).mean(0)
    rv = rng.normal(0, rot_sigma, 3)
    return rv, centre - rodrigues(rv) @ centre + rng.normal(0, 1, 3) * np.asarray(shift)


def _pixels(rng, model, mi, K, dist, pose, noise):
    pts = project12(K, dist, pose[0], pose[1], model["corners"][mi].astype(np.float64))
    return pts + rng.normal(0, noise, pts.shape) if noise else pts


def _place(r, marker_id, pts, p0, patterns):
    """Appends one marker whose feature j sits at position p0 + j with the id pair patterns[j]; corners from the projected model
    points pts."""
    m, f0, nf = int(r["n_markers"]), int(r["n_features"]), len(patterns)
    assert m < 100 and f0 + nf <= 100
    r["markers"][m] = (marker_id, f0, nf, nf)
    for j, (il, ir) in enumerate(patterns):
        F = r["features"][f0 + j]
        F["pos"], F["id_left"], F["id_right"], F["id"] = p0 + j, il, ir, 8 * il + ir
        F["corners"] = pts[(p0 + j) * 8:(p0 + j) * 8 + 8].astype(np.float32).ravel()
    r["n_markers"], r["n_features"] = m + 1, f0 + nf
    return m


def layout(n, size):
    """Members (lists of id pairs) of a rig with exactly n = 8a + 4b points from markers of `size` columns: members are filled
    to `size` features one after the other, so the concatenation crosses from member to member at multiples of size * 8; 16
    points or more always come from at least two members.  The 4-point feature sits second in the last member, where the
    end-feature rule cannot skip it (or in a member of at most two features)."""
    assert n % 4 == 0 and 4 <= n <= 800
    full, half = n // 8, (n % 8) // 4
    total = full + half
    counts = [size] * (total // size) + ([total % size] if total % size else [])
    if len(counts) == 1 and n >= 16:
        counts = [total - total // 2, total // 2]
    members = [[FULL] * c for c in counts]
    if half:
        members[-1][min(1, len(members[-1]) - 1)] = HALF
    return members


def _place_rig(r, rng, model, models, members, K, dist, pose, noise):
    """Member j of `members` as a marker of model models[j], from a random first position."""
    for mi, patterns in zip(models, members):
        p0 = int(rng.integers(0, model["size"] - len(patterns) + 1))
        _place(r, int(model["ids"][mi]), _pixels(rng, model, mi, K, dist, pose, noise), p0, patterns)


def _headers(b, recs=None):
    recs = b["recs"] if recs is None else recs
    return np.array([rs.expected_header(recs[f], b["model"], b["rig_of_model"], g, f)[0] for f in range(len(recs)) for g in range(b["n_rigs"])])


def size_edges(form, model_size, dist=None):
    """One rig per frame with exactly the point counts of the small list (form "small": 4 .. 160, k_rig_solve<160,64>) or the
    large list ("large": 164 .. 800, k_rig_solve<800,256>), built from members of model_size 20 (160-point members) or 12 (96-point
    members).  At model_size 12 the 8 points come from two members of 4.  Four frames per count: two noise-free with planted
    poses, two with 0.2 px noise.  dist: the camera's coefficients (default: the golden camera's)."""
    K, golden_dist, _ = golden_camera_and_model()
    dist = golden_dist if dist is None else np.asarray(dist, np.float32)
    counts = SMALL_COUNTS if form == "small" else LARGE_COUNTS
    model = cylinder_model(6, 20) if model_size == 20 else cylinder_model(9, 12)
    rng = np.random.default_rng(1200 + model_size + (0 if form == "small" else 100))
    recs = np.zeros(4 * len(counts), RESULT_DT)
    planted = []
    for i, n in enumerate(counts):
        members = [[HALF], [HALF]] if (n == 8 and model_size == 12) else layout(n, model_size)
        assert len(members) >= (2 if n >= 16 else 1) and len(members) <= len(model["ids"])
        for j in range(4):
            pose = _pose(rng, model["corners"][:len(members)])
            _place_rig(recs[4 * i + j], rng, model, range(len(members)), members, K, dist, pose, 0.0 if j < 2 else 0.2)
            planted.append([pose] if j < 2 else None)
    b = {"recs": recs, "model": model, "rig_of_model": np.zeros(len(model["ids"]), np.int32), "n_rigs": 1, "K": K, "dist": dist,
         "planted": planted, "counts": counts}
    H = _headers(b)
    assert (H["status"] == rs.OK).all() and [int(v) for v in H["n_points"]] == [n for n in counts for _ in range(4)]
    assert set(int(v) for v in H["n_points"]) == set(counts)
    return b


# kinds of one rig in one frame of stride_batch -> (point count, features used)
def _stride_rig(r, rng, model, kind, own, flat, K, dist):
    """Rig content of one kind: own = the rig's six model indices, flat = the two planar models of rig 1."""
    pose = _pose(rng, model["corners"][list(own)])
    if kind[1:].isdigit():
        members = layout(int(kind[1:]), 20)
        _place_rig(r, rng, model, own, members, K, dist, pose, 0.2)
    elif kind == "excluded":   # a marker that points outside the record: excluded, the rig has no member
        m = _place(r, int(model["ids"][own[0]]), _pixels(rng, model, own[0], K, dist, pose, 0.2), 0, [])
        r["markers"][m]["first_feature"], r["markers"][m]["n_features"] = -1, 1
    elif kind == "too few":    # a member without points
        _place(r, int(model["ids"][own[0]]), _pixels(rng, model, own[0], K, dist, pose, 0.2), 0, [])
    elif kind == "planar":     # 24 points of a planar model
        _place_rig(r, rng, model, flat[:1], [[FULL] * 3], K, dist, pose, 0.2)
    elif kind == "planar large":  # 168 points of two planar models
        _place_rig(r, rng, model, flat, [[FULL] * 20, [FULL]], K, dist, pose, 0.2)
    else:
        assert kind == "none"


# (rig 0, rig 1, frame is CTAG_OK, copies in the call)
STRIDE_FRAMES = (("p8", "p8", True, 1250), ("p8", "p8", True, 1250), ("p8", "p8", True, 1250), ("p160", "p8", True, 60), ("p8", "p160", True, 60),
                 ("p164", "p8", True, 100), ("p8", "p516", True, 100), ("p516", "p164", True, 60), ("p800", "too few", True, 40),
                 ("excluded", "p800", True, 40), ("p8", "p8", False, 50), ("excluded", "p8", True, 50), ("too few", "p160", True, 50),
                 ("p8", "planar", True, 60), ("p164", "planar large", True, 60), ("none", "p8", True, 50), ("p160", "p160", True, 40),
                 ("p800", "none", True, 40))


def stride_batch():
    """4610 frames x 2 rigs in one call, drawn from the 18 distinct frames of STRIDE_FRAMES in a fixed permutation: more than
    2 x 4096 items for the small list (8, 160 points, planar 24) and more than 2 x 256 for the large list (164, 516, 800 points,
    planar 168), so both solve kernels walk their list with a stride and reuse their LDS image after longer, shorter and
    degenerate items; frames that are not CTAG_OK, rigs with only an excluded marker and rigs without points in between.  In the
    frames of kinds 5, 6 and 14 one rig is a small-list item and the other a large-list item.
    Also returns "distinct" (the 18 frames), "order" (frame -> distinct frame), "degenerate" (for the distinct frames) and the two
    list lengths."""
    K, dist, _ = golden_camera_and_model()
    base = cylinder_model(14, 20)
    model = planar_model(base, [12, 13])  # pixels come from the cylinder, the model list holds the flattened corners
    rig_of_model = np.array([0] * 6 + [1] * 8, np.int32)
    rng = np.random.default_rng(1300)
    distinct = np.zeros(len(STRIDE_FRAMES), RESULT_DT)
    for d, (k0, k1, ok, _) in enumerate(STRIDE_FRAMES):
        _stride_rig(distinct[d], rng, base, k0, range(0, 6), None, K, dist)
        _stride_rig(distinct[d], rng, base, k1, range(6, 12), [12, 13], K, dist)
        distinct[d]["status"] = 0 if ok else 1
    order = np.concatenate([np.full(c, d) for d, (_, _, _, c) in enumerate(STRIDE_FRAMES)])
    order = order[np.random.default_rng(1301).permutation(len(order))]
    b = {"model": model, "rig_of_model": rig_of_model, "n_rigs": 2, "K": K, "dist": dist, "planted": None, "distinct": distinct,
         "order": order, "degenerate": lambda f, g: g == 1 and STRIDE_FRAMES[f][1].startswith("planar")}
    H = _headers(b, distinct)
    want_n = {"none": 0, "excluded": 0, "too few": 0, "planar": 24, "planar large": 168}
    for d, (k0, k1, ok, _) in enumerate(STRIDE_FRAMES):
        for g, kind in enumerate((k0, k1)):
            h = H[2 * d + g]
            n = (int(kind[1:]) if kind[1:].isdigit() else want_n[kind]) if ok else 0
            st = rs.NOT_SEEN if (not ok or kind in ("none", "excluded")) else (rs.TOO_FEW if kind == "too few" else rs.OK)
            assert (int(h["status"]), int(h["n_points"])) == (st, n), (d, g, kind, h)
            assert int(h["n_excluded"]) == (1 if ok and kind == "excluded" else 0)
    solved = (H["status"] == rs.OK).reshape(-1, 2)[order]
    points = H["n_points"].reshape(-1, 2)[order]
    b["small_items"], b["large_items"] = int((solved & (points <= 160)).sum()), int((solved & (points > 160)).sum())
    assert b["small_items"] > 2 * SMALL_GRID and b["large_items"] > 2 * LARGE_GRID, (b["small_items"], b["large_items"])
    b["recs"] = distinct[order]
    return b


def count_stride_batch():
    """4097 frames x 64 rigs = 262 208 items, 64 more than k_rig_count's 1024 x 256 threads, tiled from four distinct frames: "seen"
    (rig 0 with 8 points, rig 5 with a member without points, rig 63 with 16 points from two members), "other" (rig 17 with 24
    points), an empty frame and a frame that is not CTAG_OK.  Frames 4095 and 4096 are "seen": OK, TOO_FEW and NOT_SEEN items lie on
    both sides of item 262 144 and the last item is OK.  Most rigs have no model at all."""
    K, dist, _ = golden_camera_and_model()
    model = cylinder_model(6, 12)
    rig_of_model = np.array([0, 0, 5, 63, 63, 17], np.int32)
    rng = np.random.default_rng(1400)
    distinct = np.zeros(4, RESULT_DT)
    seen = distinct[0]
    pose = _pose(rng, model["corners"])
    _place_rig(seen, rng, model, [3], [[FULL]], K, dist, pose, 0.2)
    _place(seen, 2, _pixels(rng, model, 2, K, dist, pose, 0.2), 0, [])
    _place_rig(seen, rng, model, [0, 4], [[FULL], [FULL]], K, dist, pose, 0.2)
    _place_rig(distinct[1], rng, model, [5], [[FULL] * 3], K, dist, pose, 0.2)
    distinct[3] = seen
    distinct[3]["status"] = 2
    n_frames = COUNT_GRID // 64 + 1
    order = np.full(n_frames, 2)
    order[0::16], order[5::16], order[9::16], order[-2] = 0, 3, 1, 0
    b = {"model": model, "rig_of_model": rig_of_model, "n_rigs": 64, "K": K, "dist": dist, "planted": None, "distinct": distinct, "order": order}
    H = _headers(b, distinct).reshape(4, 64)
    assert [int(H[0][g]["status"]) for g in (0, 5, 63)] == [rs.OK, rs.TOO_FEW, rs.OK] and (H[0]["status"] == rs.NOT_SEEN).sum() == 61
    assert [int(H[0][g]["n_points"]) for g in (0, 5, 63)] == [8, 0, 16] and int(H[1][17]["n_points"]) == 24
    assert (H[2:]["status"] == rs.NOT_SEEN).all() and n_frames * 64 > COUNT_GRID and order[-1] == order[-2] == 0
    b["recs"] = distinct[order]
    return b


RULE_FRAMES = ("plain", "hundred markers", "n_markers 120", "n_markers -3", "bound: skip, then fit", "duplicate of a rejected marker",
               "first_feature -1", "features end at 101", "n_features -1", "one id, two models", "members without points", "plain again")
MASK_MEMBERS = (0, 31, 32, 63, 64, 95, 96, 99)  # marker indices: both ends of every member_mask word


def rule_batch():
    """Twelve frames (RULE_FRAMES) under a list of ten 20-column models: models 0-7 are rig 0, 8 and 9 rig 1, and model 9 repeats the
    id of model 3, so it can never be looked up.  The corrupted records lie in the middle of the batch.  Also returns "names"."""
    K, dist, _ = golden_camera_and_model()
    model = cylinder_model(10, 20, ids=[0, 1, 2, 3, 4, 5, 6, 7, 8, 3])
    rig_of_model = np.array([0] * 8 + [1, 1], np.int32)
    rng = np.random.default_rng(1500)
    recs = np.zeros(len(RULE_FRAMES), RESULT_DT)
    pix = lambda mi, pose: _pixels(rng, model, mi, K, dist, pose, 0.2)  # noqa: E731

    def plain(r, bad=None):
        """Model 0 with three features in rig 0, model 8 with two in rig 1; bad = (first_feature, n_features) of a marker of
        model 1 between them."""
        pose = _pose(rng, model["corners"][:2])
        _place(r, 0, pix(0, pose), 4, [FULL] * 3)
        if bad is not None:
            m = _place(r, 1, pix(1, pose), 0, [])
            r["markers"][m]["first_feature"], r["markers"][m]["n_features"], r["markers"][m]["n_pos"] = bad[0], bad[1], max(bad[1], 0)
        _place(r, 8, pix(8, _pose(rng, model["corners"][8])), 7, [FULL] * 2)

    plain(recs[0])
    plain(recs[11])
    # 100 one-feature markers: members of rig 0 at MASK_MEMBERS (models 0-7), id 8 (rig 1: a member, then duplicates) at every
    # seventh index from 3, unknown ids elsewhere
    pose = _pose(rng, model["corners"][:8])
    r = recs[1]
    for k in range(100):
        if k in MASK_MEMBERS:
            mi = MASK_MEMBERS.index(k)
            marker_id = mi
        else:
            mi, marker_id = (8, 8) if k % 7 == 3 else (0, 1000 + k)
        _place(r, marker_id, pix(mi, pose), k % 20, [FULL])
    recs[2] = recs[3] = r
    recs[2]["n_markers"], recs[3]["n_markers"] = 120, -3
    # 160 + 160 + 160 + 160 + 152 = 792 points; then 16 (808 > 800: excluded, and the scan goes on); then 8 (800: a member)
    pose = _pose(rng, model["corners"][:7])
    r = recs[4]
    for mi in range(4):
        _place(r, mi, pix(mi, pose), 0, [FULL] * 20)
    _place(r, 4, pix(4, pose), 0, [FULL] * 19)
    m = _place(r, 5, pix(5, pose), 0, [])
    r["markers"][m]["first_feature"], r["markers"][m]["n_features"], r["markers"][m]["n_pos"] = 0, 2, 2  # the first marker's features 0 and 1
    _place(r, 6, pix(6, pose), 9, [FULL])
    # the first marker with id 2 has a position outside the model, the second is good: both are excluded
    pose = _pose(rng, model["corners"][2])
    r = recs[5]
    _place(r, 2, pix(2, pose), 3, [FULL] * 3)
    r["features"][1]["pos"] = 20
    _place(r, 2, pix(2, pose), 8, [FULL] * 3)
    plain(recs[6], bad=(-1, 2))
    plain(recs[7], bad=(99, 2))
    plain(recs[8], bad=(3, -1))
    _place(recs[9], 3, pix(3, _pose(rng, model["corners"][3])), 5, [FULL] * 3)
    pose = _pose(rng, model["corners"][:2])
    _place(recs[10], 0, pix(0, pose), 0, [])
    _place(recs[10], 1, pix(1, pose), 0, [])
    b = {"recs": recs, "model": model, "rig_of_model": rig_of_model, "n_rigs": 2, "K": K, "dist": dist, "planted": None, "names": RULE_FRAMES}
    H = _headers(b).reshape(len(recs), 2)
    col = lambda k: [[int(v) for v in row] for row in H[k]]  # noqa: E731
    OK, FEW, NS = rs.OK, rs.TOO_FEW, rs.NOT_SEEN
    assert col("status") == [[OK, OK], [OK, OK], [OK, OK], [NS, NS], [OK, NS], [NS, NS], [OK, OK], [OK, OK], [OK, OK], [OK, NS], [FEW, NS], [OK, OK]]
    assert col("n_points") == [[24, 16], [64, 8], [64, 8], [0, 0], [800, 0], [0, 0], [24, 16], [24, 16], [24, 16], [24, 0], [0, 0], [24, 16]]
    assert col("n_excluded") == [[0, 0], [0, 12], [0, 12], [0, 0], [1, 0], [2, 0], [1, 0], [1, 0], [1, 0], [0, 0], [0, 0], [0, 0]]
    assert col("n_members") == [[1, 1], [8, 1], [8, 1], [0, 0], [6, 0], [0, 0], [1, 1], [1, 1], [1, 1], [1, 0], [2, 0], [1, 1]]
    assert [int(v) for v in H[1][0]["member_mask"]] == [0x80000001] * 3 + [0x9] and [int(v) for v in H[1][1]["member_mask"]] == [8, 0, 0, 0]
    assert int(H[4][0]["member_mask"][0]) == 0b1011111
    return b
