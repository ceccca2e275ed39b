"""Stages a5-a10 of the oracle against the independent statements in `tests/marker_testlib.py` (a5 `featureRecovery` +
`featureOrganization`, a6 `cornerObtain`, a8 `markerOrganization`, a9 `featureExtraction`, a10 `markerDecoder` + `match_dictionary`)
and `tests/refine_testlib.py` (a7 `edgeRefine`), on test.bmp, the 64-frame sequence, the 8 golden synthetic frames, 16 random-shape
frames, the frames of `tests/strip_shapes.py` and 8 many-marker frames.

Stage by stage, "ref" fed with the oracle's previous stage: every integer exact and every float of a5, a6, a8, a9, a10 equal byte
for byte (those stages use only IEEE + - * / sqrt and the shared atan2f, so the reference's types give the oracle's bytes); a7
corners within 1e-3 px.  Nothing is excused against the oracle.  "ref" against "f64" (the statement against itself, same
inputs): integers equal unless a margin recorded for the differing item (quad, feature, marker) lies below EXCUSE_MARGIN, corners within 1e-3 px; at most 0.3 % of the compared
features may be excused and at most 5 % may lie beyond 1e-3 px.  Once end to end: labels -> `edge_testlib.extract_frame` -> a5 ...
a10 with no oracle value in between."""
import math

import numpy as np
import pytest

import edge_testlib as et
import marker_testlib as mt
import refine_testlib as rt
import strip_shapes as ss
from sequences import avi_substitute

EXCUSE_MARGIN = et.EXCUSE_MARGIN      # 1e-5, as for a4
EXCUSE_SHARE = 3e-3
BEYOND_SHARE = 0.05
REF_TOL_PX = 1e-3                     # a7 corners, "ref" against the oracle: the project's bar
F64_TOL_PX = 1e-3                     # corners, centres and edge lengths, "f64" against "ref"; a7 corners: plus refine_testlib's
                                      # DIRECTION_RESOLUTION term, for at most BEYOND_SHARE of the features
# Cross ratios (:1075): (l0 + l1) (l2 + l1) / (l1 l3) of four float distances between the same float corners in both modes.  Each
# distance carries at most 4 float roundings (two squares, a sum, a root), the ratio 5 more: below 10 * 2^-24 = 6e-7 of a value
# below 10.  The bar leaves a factor of 10 for cancellation in `a - b` of nearby corners being exact only up to the corners' own ulp.
F64_TOL_CR = 1e-4
ALL_DISTS = (0, 1, 3, 5, 8, 9)


def _frames(state, test_bmp):
    """(name, frame, cornerSubPixDist values, also with cornerSubPix off)"""
    import testkit as tk
    yield "test.bmp", test_bmp, ALL_DISTS, True
    for k, f in enumerate(avi_substitute(test_bmp)):
        yield "sequence %d" % k, f, ALL_DISTS if k in (0, 21, 42, 63) else (5,), k == 0
    for f in range(8):
        yield "synthetic %d" % f, tk.synth_frame_host(state, f)[0], ALL_DISTS if f < 2 else (5,), f == 0
    for seed in range(16):
        rows, cols = ((720, 1152), (540, 960), (1080, 1920), (601, 1023))[seed % 4]
        yield "random shapes %d" % seed, et.random_shapes_frame(state, seed, rows, cols), (5,), False
    for name, f, _ in ss.strip_frames_tagged(state):
        yield "strips " + name, f, ALL_DISTS if name in ("borders", "carry", "long_edges") else (5,), name == "codes"
    for mk in (6, 8):  # the frames of test_gpu_parity.test_many_markers_per_frame
        for idx in (5, 6, 7, 8):
            yield "many markers %d/%d" % (mk, idx), tk.synth_frame_host(state, idx, markers=mk)[0], (5,), False


class Tally:
    def __init__(self):
        self.features = self.markers = self.decoded = self.runs = 0
        self.failed, self.excused, self.excused_items, self.beyond = [], [], 0, 0
        self.a7_max = self.f64_max = self.cr_max = self.beyond_ratio = 0.0
        self.count = {}

    def merge(self, traces):
        for tr in traces:
            for k, v in tr.count.items():
                self.count[k] = self.count.get(k, 0) + v

    def report(self):
        return ("%d runs: %d features, %d markers before decoding, %d decoded; largest a7 corner difference to the oracle %.2e px; "
                "f64 against ref: largest corner difference %.2e px, largest cross-ratio difference %.2e, %d features beyond "
                "%.0e px but within a7's float32 resolution (at most %.2f of it), %d features excused by a margin below %.0e%s") % (
            self.runs, self.features, self.markers, self.decoded, self.a7_max, self.f64_max, self.cr_max, self.beyond, F64_TOL_PX, self.beyond_ratio,
            self.excused_items, EXCUSE_MARGIN, "".join("\n  excused: " + e for e in self.excused))


def _same(what, mine, theirs, tally):
    if np.asarray(mine).tobytes() != np.asarray(theirs).tobytes():
        tally.failed.append("%s differs from the oracle" % what)


def _stage_by_stage(name, img, o, state, fs, subpix, dist, tally):
    """One oracle run against "ref" fed with the oracle's stages, and "ref" against "f64" on the same inputs."""
    what = "%s (subpix %s, dist %d)" % (name, subpix, dist)
    tally.runs += 1
    T = {m: {k: mt.Trace() for k in ("a5", "a7", "a8", "a10")} for m in ("ref", "f64")}
    if o["status"] == mt.NO_CORNER:
        assert len(o["quads"]) == 0, what
        return
    assert o["status"] in (mt.OK, mt.NO_FEATURE), (what, o["status"])
    f0 = {m: mt.recover_features(o["quads"], m, None, T[m]["a5"]) for m in T}
    _same(what + " a5 features", f0["ref"][0], o["features"][0], tally)
    assert (o["status"] == mt.NO_FEATURE) == (len(f0["ref"][0]) < fs), what
    items = len(f0["ref"][0])
    tally.features += items
    misses = []  # (what differs, the margin of that item, features it stands for)

    def margin_of(stage, *items):
        return min(T[m][stage].item_margin.get(it, math.inf) for m in T for it in items)

    pairs = {m: {tuple(p) for p in f0[m][1].tolist()} for m in T}
    for p in sorted(pairs["ref"] ^ pairs["f64"]):  # a feature one mode pairs and the other does not: the margins of its two quads
        misses.append(("a5 pairing of quads %d, %d" % p[:2], margin_of("a5", p[0], p[1]), 1))
    if o["status"] == mt.OK:
        f1 = {m: mt.obtain_corners(o["features"][0], m) for m in T}
        _same(what + " a6 features", f1["ref"], o["features"][1], tally)
        if subpix:
            f2 = {m: rt.refine_features(img, o["features"][1], dist, m, T[m]["a7"]) for m in T}
            d = np.abs(f2["ref"].astype(np.float64) - o["features"][2])
            tally.a7_max = max(tally.a7_max, float(d[:, :16].max()))
            if d[:, :16].max() > REF_TOL_PX or d[:, 16:].max() != 0:
                tally.failed.append("%s a7: corners %.2e px off the oracle's" % (what, d.max()))
            d = np.abs(f2["f64"] - f2["ref"])[:, :16].max(1)
            tally.f64_max = max(tally.f64_max, float(d.max()))
            for k in np.nonzero(d > F64_TOL_PX)[0]:  # beyond the plain bar: within what a7's float32 line directions resolve
                res = T["ref"]["a7"].resolution.get(int(k), 0.0)
                tally.beyond += 1
                tally.beyond_ratio = max(tally.beyond_ratio, (d[k] - F64_TOL_PX) / max(res, 1e-30))
                if d[k] > F64_TOL_PX + res:
                    tally.failed.append("%s a7: f64 corners of feature %d %.2e px off ref (float32 resolution %.1e)" % (what, k, d[k], res))
        else:
            _same(what + " stage 2 with cornerSubPix off", o["features"][2], o["features"][1], tally)
        pre = {m: mt.organize_markers(o["features"][2], m, None, T[m]["a8"]) for m in T}
        _same(what + " a8 + a9 premarkers", pre["ref"], o["premarkers"], tally)
        res = {m: mt.decode_markers(o["premarkers"], state, fs, m, T[m]["a10"]) for m in T}
        _same(what + " a10 result", res["ref"], o["result"], tally)
        tally.markers += int(o["premarkers"]["n_markers"])
        tally.decoded += int(o["result"]["n_markers"])
        # a8 + a9 by input feature: its marker, its place there and its ids; a10 by marker: what the dictionary made of it
        by_feature = {m: {k: (int(np.searchsorted(pre[m]["markers"]["first_feature"][:pre[m]["n_markers"]], s, "right")) - 1,
                               s, int(pre[m]["features"]["id"][s]), int(pre[m]["features"]["id_left"][s]), int(pre[m]["features"]["id_right"][s]))
                           for s, k in enumerate(T[m]["a8"].slot_feature)} for m in T}
        differing = [k for k in by_feature["ref"] if by_feature["ref"][k] != by_feature["f64"].get(k)]
        for k in differing:
            misses.append(("a8 + a9 record of feature %d" % k, margin_of("a8", k), 1))
        if not differing and mt.record_integers(pre["ref"]) != mt.record_integers(pre["f64"]):
            misses.append(("a8 + a9 integers", math.inf, items))
        for mi in sorted(set(T["ref"]["a10"].outcome) | set(T["f64"]["a10"].outcome)):
            if T["ref"]["a10"].outcome.get(mi) != T["f64"]["a10"].outcome.get(mi):
                misses.append(("a10 outcome of marker %d" % mi, margin_of("a10", mi), int(o["premarkers"]["markers"]["n_features"][mi])))
        for stage, rec in (("a8", pre), ("a10", res)):
            if mt.record_integers(rec["ref"]) == mt.record_integers(rec["f64"]):
                d = np.abs(mt.record_reals(rec["ref"]) - mt.record_reals(rec["f64"]))
                if d.size:
                    tally.cr_max = max(tally.cr_max, float(d[:, 19:].max()))
                    if d[:, :19].max() > F64_TOL_PX or d[:, 19:].max() > F64_TOL_CR:
                        tally.failed.append("%s %s: f64 reals %.2e / %.2e off ref" % (what, stage, d[:, :19].max(), d[:, 19:].max()))
            elif not misses:
                misses.append((stage + " integers", math.inf, items))
    for item, margin, weight in misses:  # excused only by a margin of the item that differs, as the a4 test does per candidate
        entry = "%s: f64 and ref differ in %s (margin %.1e)" % (what, item, margin)
        if margin < EXCUSE_MARGIN:
            tally.excused.append(entry)
            tally.excused_items += weight
        else:
            tally.failed.append(entry)
    tally.merge(T["ref"].values())
    return T["ref"]


@pytest.fixture(autouse=True, scope="module")
def shared_math(oracle):
    """Every test of this file runs "ref" with the project's shared float functions (one object, edge_testlib's included)."""
    mt.use_shared_math(oracle)


@pytest.fixture(scope="module")
def back_runs(oracle, dictionary, test_bmp):
    """Every frame through the oracle at each of its settings, compared as it goes: (tally, {strip frame: trace counters})."""
    state, fs = dictionary
    tally, strips = Tally(), {}
    for name, img, dists, also_off in _frames(state, test_bmp):
        for dist in dists:
            o = oracle.detect(img, state, fs, subpix_dist=dist)
            T = _stage_by_stage(name, img, o, state, fs, True, dist, tally)
            if name.startswith("strips ") and T is not None:
                c = strips.setdefault(name[len("strips "):], {})
                for tr in T.values():
                    for k, v in tr.count.items():
                        c[k] = c.get(k, 0) + v
        if also_off:
            o = oracle.detect(img, state, fs, subpix=False)
            _stage_by_stage(name, img, o, state, fs, False, 0, tally)
    return tally, strips


def test_back_stages_match_independent_statement(back_runs):
    tally, _ = back_runs
    print("\nstages a5-a10, oracle vs statement: " + tally.report())
    assert not tally.failed, "%d misses:\n%s" % (len(tally.failed), "\n".join(tally.failed[:40]))
    assert tally.excused_items <= EXCUSE_SHARE * tally.features, tally.report()
    assert tally.beyond <= BEYOND_SHARE * tally.features, tally.report()
    assert tally.features >= 3000 and tally.markers >= 300, tally.report()
    assert tally.a7_max > 0 or tally.f64_max > 0  # (a7 had something to compute)


def test_strip_frames_reach_their_branches(back_runs):
    """Every tag of tests/strip_shapes.py is a counter of the statement's trace that its frame must have raised."""
    _, strips = back_runs
    assert set(strips) == set(ss.FRAMES)
    for name, (_, tags) in ss.FRAMES.items():
        missing = [t for t in tags if not strips[name].get(t)]
        assert not missing, (name, missing, strips[name])
    reached = set().union(*strips.values())
    print("\nstrip frames reached: " + ", ".join(sorted(reached)))
    # on some frame of the set: an edge without one usable sample (N == 0: NaN moments, the old corner kept, :773-775)
    assert {"a7.edge_without_sample", "a7.nan_determinant", "a7.corner_kept", "a9.zero_determinant_vanish", "a10.gap_0", "a10.gap_2",
            "a10.rejected", "a7.axis_aligned_edge_at_half_pixel"} <= reached


def test_end_to_end_from_labels(oracle, dictionary, test_bmp):
    """labels -> a4 ("ref" of edge_testlib) -> a5 ... a10 with no oracle value in between: the interfaces between the stages (which
    candidates become quads, in what order; the two early returns) are part of what is restated."""
    import testkit as tk
    state, fs = dictionary
    frames = [("test.bmp", test_bmp)] + [("synthetic %d" % f, tk.synth_frame_host(state, f)[0]) for f in range(8)]
    frames += [("strips " + n, f) for n, f, _ in ss.strip_frames_tagged(state)]
    frames.append(("blank", np.full((720, 1152), 200, np.uint8)))          # no corner
    one = np.full((720, 1152), 215, np.uint8)
    ss.box(one, 300, 300, 30, 120)
    frames.append(("one quad", one))                                        # no feature
    statuses = set()
    for name, img in frames:
        o = oracle.detect(img, state, fs)
        cands = et.extract_frame(o["labels"], "ref")
        quads = np.array([c.corners.ravel() for c in cands if c.has_quad], np.float32).reshape(-1, 8)
        b = rt.back_half(quads, img, state, fs, "ref")
        statuses.add(int(o["status"]))
        assert int(b["result"]["status"]) == o["status"], name
        if o["status"] == mt.OK:
            d = np.abs(b["features2"].astype(np.float64) - o["features"][2]).max()
            assert d <= REF_TOL_PX, (name, d)
        if o["status"] != mt.OK or np.array_equal(b["features2"], o["features"][2]):
            assert b["result"].tobytes() == o["result"].tobytes(), name
        else:  # a7 corners a float ulp apart: integers exact, reals within the a7 bar
            assert mt.record_integers(b["result"]) == mt.record_integers(o["result"]), name
            d = np.abs(mt.record_reals(b["result"]) - mt.record_reals(o["result"]))
            assert d[:, :19].max() <= REF_TOL_PX and d[:, 19:].max() <= F64_TOL_CR, (name, d.max())
    assert statuses == {mt.OK, mt.NO_CORNER, mt.NO_FEATURE}


def test_known_answers_of_branches_no_frame_reaches():
    """Branches a drawn frame cannot reach (docs/history.md), worked by hand.  (The fourth dropped tag, clause :543 failing alone, has
    no answer to work: no input reaches it.)

    a7, `fabs(det) <= 0.001` with finite lines (:769-775): corner 1 of a quad lies on the straight image edge that runs from corner 0
    to corner 2, so `lines_next[0]` and `lines_last[1]` are fits of the same vertical edge x = 100: both normals are (+-1, 0), det = 0,
    and the corner keeps its input position exactly.
    a10, C division in the reversed match (:1299): -2 / 8 = 0 and -2 % 8 = -2 give 7 + 9 * 8 = 79, -1 gives 7 + 8 * 8 = 71: neither
    is a dictionary code, so only the known codes count; [9, -2, 18] read backwards is 54, (no match), 45.
    a10, a decoded marker with a gap of 3 (:1223-1226): two features 37.5 px apart with edge lengths of 10: 37.5 / ((10 + 10) * 3 / 4) =
    2.5, `round` goes away from zero: the second code lands on position 3, and 45 . . 1 stands at columns 0 and 3 of the row."""
    img = np.full((200, 300), 230, np.uint8)
    img[:, :100] = 20
    f1 = np.zeros((1, 19), np.float32)
    # quad 1: corners 0, 1, 2 down the edge (estimated 1.5 px to the bright side), corner 3 far in the dark; quad 2 in flat bright ground
    f1[0, :16] = [101.5, 40, 101.5, 100, 101.5, 160, 30, 100, 200, 40, 260, 40, 260, 160, 200, 160]
    for mode in ("ref", "f64"):
        tr = mt.Trace()
        f2 = rt.refine_features(img, f1, 5, mode, tr)
        assert f2[0, 2] == 101.5 and f2[0, 3] == 100, f2[0, :8]      # corner 1 kept
        assert tr.item_margin[0] <= 0.001 and tr.count["a7.corner_kept"] >= 1
        # quad 2 lies in flat ground: N == 0 on its four edges, NaN lines, four corners kept.  Edges 2 -> 3 and 3 -> 0 of quad 1 have their
        # normals towards the dark side (g1 < g2 on every step: skipped), so corners 2, 3 and 0 meet a NaN line too: 4 + 3
        assert (f2[0] == f1[0]).all() and tr.count["a7.nan_determinant"] == 7 and tr.count["a7.corner_kept"] == 8
    assert mt._cdiv(-2, 8) == (0, -2) and mt._cdiv(-1, 8) == (0, -1) and mt._cdiv(-9, 8) == (-1, -1) and mt._cdiv(17, 8) == (2, 1)
    state = np.array([[45, 3, 54, 1, 2, 4, 5, 6, 7, 8, 10, 11]], np.int32)  # 54 = 7 - 9 // 8 + (7 - 9 % 8) * 8, 45 likewise of 18
    code = [9, -2, 18] + [-1] * 17
    good, ident, inverse, pos = mt.match_dictionary(code, state, 2, 2)
    assert (good, ident, inverse, pos) == (True, 0, True, [2, 1, 0])
    # a code that spans 14 positions of a 12-column dictionary.  Forwards (j + 13) % 12 wraps to the next column, so 45, 3
    # at columns 0, 1 cover both codes; backwards (j - 13 + 12) % 12 is -1 for j = 0 (C remainder): that column matches nothing
    tr = mt.Trace()
    good, ident, inverse, pos = mt.match_dictionary([45] + [-1] * 12 + [3] + [-1] * 6, state, 13, 2, tr)
    assert (good, ident, inverse, pos) == (True, 0, False, [0, 1]) and tr.count["a10.negative_column"] == 1  # j = 0, k = 13 only
    pre = mt._empty_result("ref")
    pre["n_markers"], pre["n_features"] = 1, 2
    pre["markers"][0] = (-1, 0, 2, 0)
    for k, (ident, x) in enumerate(((45, 0.0), (1, 37.5))):
        f = pre["features"][k]
        f["pos"], f["id"], f["id_left"], f["id_right"], f["center"], f["edge_length"] = -1, ident, ident // 8, ident % 8, (x, 0.0), 10.0
    for mode in ("ref", "f64"):
        tr = mt.Trace()
        res = mt.decode_markers(pre, state, 2, mode, tr)
        assert res["n_markers"] == 1 and res["markers"][0].tolist() == (0, 0, 2, 2) and res["features"]["pos"][:2].tolist() == [0, 3]
        assert tr.count["a10.accepted_with_gap_3"] == 1 and tr.count["a10.gap_3+"] == 1 and tr.item_margin[0] == 0  # 2.5: on the rounding edge
