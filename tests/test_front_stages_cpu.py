"""Stages a0-a3 of the oracle (BGR2GRAY, resize, adaptiveThreshold, labelling and the area filter) against the independent statement
in `tests/front_testlib.py`, on the frames of `tests/front_shapes.py`, test.bmp (every window), the 8-frame sequence, 12 synthetic
frames and 8 random-shape frames.  Every comparison is an equality: the half image, the binary image, the label IMAGE (OpenCV's
numbering, not only the partition), the areas and the candidate list (label, area, box, order) of `oracle.detect`, and
`oracle.bgr2gray`, `resize_half` (both lane variants), `threshold` and `ccl` as single calls.  The coverage conditions of the shape
frames are then asserted from the statement's own trace.

The chain is closed once: `front()` -> `edge_testlib.extract_frame` -> `refine_testlib.back_half` gives the result record of a frame
with no oracle value in the data path (the shared `exp32` / `atan2f` hooks aside), held to `tests/golden/golden_v1.npz` and to the
oracle with the bars `test_back_stages_cpu.py` uses: a7 corners 1e-3 px, everything else byte for byte."""
import os

import numpy as np
import pytest

import edge_testlib as et
import front_shapes as fs
import front_testlib as ft
import marker_testlib as mt
import refine_testlib as rt
from ctag_testlib import GOLDEN
from sequences import avi_substitute

REF_TOL_PX = 1e-3   # a7 corners against the oracle and the golden records: the project's bar (test_back_stages_cpu.py)
F64_TOL_CR = 1e-4   # cross ratios of records whose a7 corners differ by a float ulp (test_back_stages_cpu.py)
ALL_WINDOWS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 31, 32)


def _params(dark_cap=0.3, area_min=30, area_max_fraction=0.01):
    import cylindertag_amd as ca
    p = ca.default_params()
    p.dark_cap, p.area_min, p.area_max_fraction = dark_cap, area_min, area_max_fraction
    return p


def _cases(state, test_bmp):
    """(name, frame (gray or BGR), window, dark_cap, (area_min, area_max_fraction), tags)"""
    import testkit as tk
    default = fs.AREA_PARAMS[0]
    for cap in fs.CAPS:
        for k, f in enumerate(fs.knife_frames(cap, fs.cap_edge_cells(cap))):
            yield "knife edges cap %g frame %d" % (cap, k), f, 5, cap, default, ("knife",)
    for name, f, tw in fs.window_frames():
        yield name, f, tw, 0.3, default, ("window",)
    for name, f, tags in fs.resize_frames():
        yield name, f, 5, 0.3, default, tags
    for name, f, tw, area, tags in fs.labelling_frames():
        yield name, f, tw, 0.3, area, tags
        if "areas" in tags and area != default:  # the same drawing under the reference's limits
            yield name + " (reference limits)", f, tw, 0.3, default, ()
    for b, batch in enumerate(fs.slot_reuse_batches()):
        yield "slot reuse batch %d" % b, batch[0], 5, 0.3, default, ()
    for tw in ALL_WINDOWS:
        yield "test.bmp window %d" % tw, test_bmp, tw, 0.3, default, ()
    yield "test.bmp ragged crop", np.ascontiguousarray(test_bmp[3:1001, 5:1711]), 5, 0.3, default, ()
    yield "test.bmp odd crop", np.ascontiguousarray(test_bmp[1:1200, 3:1914]), 7, 0.3, default, ("odd",)
    for k, f in enumerate(avi_substitute(test_bmp, 8)):
        yield "sequence %d" % k, f, 5, 0.3, default, ()
    for k in range(12):
        yield "synthetic %d" % k, tk.synth_frame_host(state, k)[0], (5, 5, 5, 3, 8, 4)[k % 6], (0.3, 0.2, 0.45, 0.12)[k % 4] if k >= 8 else 0.3, default, ()
    for seed in range(8):
        rows, cols = ((720, 1152), (540, 960), (1080, 1920), (601, 1023))[seed % 4]
        yield "random shapes %d" % seed, et.random_shapes_frame(state, seed, rows, cols), (5, 6)[seed // 4], 0.3, fs.AREA_PARAMS[seed % 3], ()
    yield "coloured test.bmp", fs.colourise(test_bmp, 1), 5, 0.3, default, ("bgr",)
    yield "coloured labelling shapes", fs.colourise(fs.double(fs.labelling_design(3)), 2), 5, 0.3, default, ("bgr",)
    yield "primaries and grays", fs.primaries(), 3, 0.3, default, ("bgr",)


class Coverage:
    def __init__(self):
        self.frames = self.pixels = self.components = self.candidates = 0
        self.failed = []
        self.knife = {cap: dict(seen=set(), edge=set(), bounds=set(), sums=set(), bright_tiles=0) for cap in fs.CAPS}
        self.tags = {}
        self.windows = set()
        self.tile_counts = set()      # (window, tile rows, tile columns) of the frames with a short direction
        self.statuses = set()

    def tag(self, t, n=1):
        self.tags[t] = self.tags.get(t, 0) + n


def _knife_coverage(cov, cap, f):
    pairs_dim = 2 * int(ft.bound_of_extrema(255, 255, cap))
    k = cov.knife[cap]
    half, tiles = f["half"], f["trace"].tiles
    hr, hc = half.shape
    own = half.reshape(hr // 5, 5, hc // 5, 5)
    own_min = own.min((1, 3))
    for ti, tj, a, b, T in tiles.tolist():
        if a + b in (pairs_dim - 1, pairs_dim, pairs_dim + 1):
            k["sums"].add(a + b)
        if own_min[ti, tj] >= pairs_dim // 2 and a < pairs_dim // 2:
            k["bright_tiles"] += 1   # no pixel of its own below the cap's bound, a dark neighbour
        if a + b >= pairs_dim:
            continue
        k["seen"].add((a, b))
        blk = own[ti, :, tj, :]
        if (blk == T).any() and (blk == T - 1).any():
            k["edge"].add((a, b))
            k["bounds"].add(T)


@pytest.fixture(scope="module")
def front_runs(oracle, dictionary, test_bmp):
    """Every case through `oracle.detect` and through the statement, compared as it goes."""
    state, fsz = dictionary
    cov = Coverage()
    try:
        for name, frame, tw, cap, (amin, frac), tags in _cases(state, test_bmp):
            oracle.set_params(None if (cap, amin, frac) == (0.3, 30, 0.01) else _params(cap, amin, frac))
            f = ft.front(frame, tw, cap, amin, frac)
            gray = frame
            if frame.ndim == 3:
                gray = oracle.bgr2gray(frame)
                if not (gray == f["gray"]).all():
                    cov.failed.append(name + ": bgr2gray")
            o = oracle.detect(gray, state, fsz, tw)
            for key in ("half", "binary", "labels"):
                if o[key].shape != f[key].shape or not (o[key] == f[key]).all():
                    cov.failed.append("%s: %s" % (name, key))
            if len(o["areas"]) != len(f["areas"]) or not (o["areas"] == f["areas"]).all():
                cov.failed.append(name + ": areas")
            if o["candidates"].shape[0] != len(f["candidates"]) or not (o["candidates"][:, 0:6] == f["candidates"]).all():
                cov.failed.append(name + ": candidate list")
            if len(f["candidates"]) == 0 and o["status"] != 1:
                cov.failed.append(name + ": no candidate, but status %d" % o["status"])
            # the stages as single calls, each fed with the statement's previous stage
            if (cap, amin, frac) == (0.3, 30, 0.01):
                if not (oracle.resize_half(f["gray"]) == f["half"]).all():
                    cov.failed.append(name + ": resize_half alone")
                if not (oracle.threshold(f["half"], tw) == f["binary"]).all():
                    cov.failed.append(name + ": threshold alone")
                lab, areas = oracle.ccl(f["binary"])
                if not ((lab == f["labels"]).all() and len(areas) == len(f["areas"]) and (areas == f["areas"]).all()):
                    cov.failed.append(name + ": ccl alone")
            cov.frames += 1
            cov.pixels += f["half"].size
            cov.components += len(f["areas"]) - 1
            cov.candidates += len(f["candidates"])
            cov.windows.add(tw)
            cov.statuses.add(int(o["status"]))
            tr = f["trace"]
            hr, hc = f["half"].shape
            trows, tcols = -(-hr // tw), -(-hc // tw)
            if min(trows, tcols) <= 4:
                cov.tile_counts.add((tw, min(trows, 5), min(tcols, 5)))
                if min(trows, tcols) < 3 and (f["binary"].any() or o["status"] != 1):
                    cov.failed.append(name + ": fewer than 3 tiles in a direction must give all background and status 1")
            if "knife" in tags:
                _knife_coverage(cov, cap, f)
            if "saturation" in tags and not (tr.saturated_low >= 0.01 * f["half"].size and tr.saturated_high >= 0.01 * f["half"].size):
                cov.failed.append("%s: %d / %d of %d pixels saturate" % (name, tr.saturated_low, tr.saturated_high, f["half"].size))
            if "vertical_ties" in tags and tr.vertical_ties < 0.9 * hr * (hc & ~7):
                cov.failed.append("%s: %d vertical ties" % (name, tr.vertical_ties))
            if "tail_differs" in tags and tr.tail_columns_differing < 1:
                cov.failed.append(name + ": body and tail rounding agree in every tail column")
            if "odd" in tags and not (gray.shape[0] | gray.shape[1]) & 1:
                cov.failed.append(name + ": not an odd size")
            if "first_block" in tags:
                cov.tag("first_block", tr.raster_first_outside_first_block)
            if "areas" in tags:
                limit = ft.area_limit(hr, hc, frac)
                have = set(f["areas"][1:].tolist())
                if not {amin - 1, amin, limit, limit + 1} <= have:
                    cov.failed.append("%s: areas %s lack one of %s" % (name, sorted(have), (amin - 1, amin, limit, limit + 1)))
                kept = set(f["candidates"][:, 1].tolist())
                if kept != {a for a in have if amin <= a <= limit}:
                    cov.failed.append(name + ": kept areas")
                cov.tag("areas")
                if (frac * hc * hr) % 1 == 0.5:
                    cov.tag("area_limit_on_half")
            if "checkerboard" in tags and not (len(f["areas"]) == 2 and len(f["candidates"]) == 0 and f["areas"][1] > ft.area_limit(hr, hc)):
                cov.failed.append(name + ": not one oversize component")
            if "many_components" in tags:
                cov.tag("many_components", int(len(f["areas"]) - 1 >= 1500))
            if "bgr" in tags:
                cov.tag("bgr")
    finally:
        oracle.set_params(None)
    return cov


def test_front_stages_match_independent_statement(front_runs):
    cov = front_runs
    print("\nstages a0-a3, oracle vs statement: %d frames, %d half-size pixels, %d components, %d candidates, windows %s, statuses %s"
          % (cov.frames, cov.pixels, cov.components, cov.candidates, sorted(cov.windows), sorted(cov.statuses)))
    assert not cov.failed, "%d misses:\n%s" % (len(cov.failed), "\n".join(cov.failed[:40]))
    assert cov.frames >= 150 and cov.components >= 50000 and cov.candidates >= 5000
    assert set(ALL_WINDOWS) <= cov.windows and {0, 1, 2} <= cov.statuses


def test_shape_frames_reach_their_edges(front_runs):
    """The coverage conditions of tests/front_shapes.py, from the statement's trace."""
    cov = front_runs
    lines = []
    for cap in fs.CAPS:
        pairs = fs.pair_table(cap)
        cap_bound = int(ft.bound_of_extrema(255, 255, cap))
        k = cov.knife[cap]
        lines.append("dark_cap %g: %d of %d pairs below %d reached, %d with pixels at the bound and one below it, %d of %d bound values, sums %s, "
                     "%d bright tiles beside dark neighbours" % (cap, len(k["seen"]), len(pairs), 2 * cap_bound, len(k["edge"]), len(k["bounds"]), cap_bound,
                                                                  sorted(k["sums"]), k["bright_tiles"]))
        assert k["seen"] <= set(pairs)
        assert len(k["seen"]) >= 0.9 * len(pairs), lines[-1]
        assert len(k["edge"]) >= 0.8 * len(pairs), lines[-1]
        assert k["bounds"] >= set(range(1, cap_bound + 1)), lines[-1]
        assert k["sums"] == {2 * cap_bound - 1, 2 * cap_bound, 2 * cap_bound + 1}, lines[-1]
        assert k["bright_tiles"] >= 30, lines[-1]
    print("\n" + "\n".join(lines))
    assert len(fs.pair_table(0.3)) == 6006 and int(ft.bound_of_extrema(255, 255, 0.3)) == 77
    assert [int(ft.bound_of_extrema(255, 255, c)) for c in fs.CAPS] == [77, 51, 115, 31]
    for tw in (1, 2, 3, 5, 7, 32):  # exactly 2, 3 and 4 tiles, in rows and in columns
        for n in (2, 3, 4):
            if 2 * (n * tw - (tw // 2 if tw > 1 else 0)) < 4:
                continue
            assert (tw, n, 5) in cov.tile_counts and (tw, 5, n) in cov.tile_counts, (tw, n, sorted(cov.tile_counts))
    assert cov.tags.get("first_block", 0) >= 20
    assert cov.tags.get("areas", 0) >= 6 and cov.tags.get("area_limit_on_half", 0) >= 1
    assert cov.tags.get("many_components") == 1 and cov.tags.get("bgr") == 3
    print("tags: %s" % sorted(cov.tags.items()))


def test_resize_at_any_size_and_both_lane_variants(oracle):
    """`oracle.resize_half` alone against the statement: odd and tiny sizes, saturating content, tie columns, and the 16-lane variant
    on widths where eight columns change hands (hcols % 16 >= 8)."""
    rng = np.random.RandomState(31)
    sizes = list(fs.ODD_SIZES) + [(37, 4001), (201, 333), (1200, 1920), (4, 9), (11, 4)]
    pixels = 0
    for h, w in sizes:
        for img in (fs.noise(h, w, rng.randint(1 << 30)), fs.black_white(h, w, rng.randint(1 << 30)), fs.tie_columns(h, w)):
            assert (oracle.resize_half(img) == ft.resize_half(img)).all(), (h, w)
            pixels += (h // 2) * (w // 2)
    differ = 0
    try:
        for cols in fs.LANE16_WIDTHS:
            assert (cols // 2) % 16 >= 8
            for img in (fs.noise(1500, cols, cols), fs.tie_columns(90, cols)):
                want8, want16 = ft.resize_half(img, 8), ft.resize_half(img, 16)
                oracle.set_variants(0, 16)
                assert (oracle.resize_half(img) == want16).all(), cols
                oracle.set_variants(0, 8)
                assert (oracle.resize_half(img) == want8).all(), cols
                differ += int((want8 != want16).sum())
                pixels += 2 * want8.size
    finally:
        oracle.set_variants(0, 8)
    assert differ > 0  # the variants are different answers on these widths
    print("\nresize alone: %d pixels, %d differ between the lane variants" % (pixels, differ))


def test_bgr2gray_alone(oracle):
    for img in (fs.primaries(), fs.colourise(fs.noise(75, 97, 1), 4), np.random.RandomState(5).randint(0, 256, (33, 1921, 3)).astype(np.uint8)):
        assert (oracle.bgr2gray(img) == ft.bgr2gray(img)).all()
    assert ft.bgr2gray(fs.primaries())[[0, 4, 8, 12], 0].tolist() == [29, 150, 76, 255]
    assert (ft.bgr2gray(fs.primaries())[16] == np.arange(256)).all()


def test_statement_known_answers():
    """The statement against answers worked by hand."""
    # an exact 2x: weights [-192, 1216, 1216, -192] for every pixel
    sx, w = ft.resize_taps(20, 10)
    assert (sx == 2 * np.arange(10)).all() and (w == [-192, 1216, 1216, -192]).all()
    # 7 -> 3: scale 7/3; fx = (d + 0.5) * 7/3 - 0.5 = 0.6667, 3.0, 5.3333
    sx, w = ft.resize_taps(7, 3)
    assert sx.tolist() == [0, 3, 5] and w[1].tolist() == [0, 2048, 0, 0] and (w.sum(1) == 2048).all()
    # u < 0.3f  <=>  u <= 76 (A.2); the mean term of (10, 20) is 15 / 255: u < 15
    assert int(ft.bound_of_extrema(255, 255)) == 77 and int(ft.bound_of_extrema(10, 20)) == 15 and int(ft.bound_of_extrema(10, 21)) == 16
    # block-raster order: A begins on the odd row of block row 0 at block column 0, B on the even row at block column 3
    b = np.zeros((6, 12), np.uint8)
    b[1, 0] = b[0, 6] = 255
    lab, areas, boxes = ft.label(b)
    assert lab[1, 0] == 1 and lab[0, 6] == 2 and areas.tolist() == [70, 1, 1] and boxes[2].tolist() == [6, 0, 6, 0]
    assert ft.area_limit(101, 250) == 253 and ft.area_limit(540, 960) == 5184  # 252.5 rounds away from zero
    # border ring and too few tiles
    half = np.zeros((10, 40), np.uint8)
    assert not ft.adaptive_threshold(half, 5).any()
    half = np.full((15, 15), 200, np.uint8)
    half[5:10, 5:10] = 10
    out = ft.adaptive_threshold(half, 5)
    assert (out[5:10, 5:10] == 255).all() and out.sum() == 25 * 255


def _golden_frames(state, test_bmp):
    import testkit as tk
    g = np.load(os.path.join(GOLDEN, "golden_v1.npz"))
    yield "test.bmp", test_bmp, g["bmp_result"][0]
    for k, f in enumerate(avi_substitute(test_bmp, 8)):
        yield "sequence %d" % k, f, g["seq_results"][k]
    for k in range(3):
        yield "synthetic %d" % k, tk.synth_frame_host(state, k)[0], g["synth_results"][k]


def test_closed_chain_from_the_frame(oracle, dictionary, test_bmp):
    """frame -> front() -> a4 ("ref" of edge_testlib) -> a5 ... a10 ("ref" of marker_testlib / refine_testlib): no oracle call between the
    frame's bytes and its record.  Held to the golden records and to the oracle's."""
    mt.use_shared_math(oracle)
    state, fsz = dictionary
    statuses = set()
    extra = [("blank", np.full((720, 1152), 200, np.uint8), None)]
    for name, img, golden in list(_golden_frames(state, test_bmp)) + extra:
        f = ft.front(img)
        cands = et.extract_frame(f["labels"], "ref")
        quads = np.array([c.corners.ravel() for c in cands if c.has_quad], np.float32).reshape(-1, 8)
        b = rt.back_half(quads, img, state, fsz, "ref")
        o = oracle.detect(img, state, fsz)
        statuses.add(int(o["status"]))
        for what, want in (("oracle", o["result"]), ("golden", golden)):
            if want is None:
                continue
            assert int(b["result"]["status"]) == int(want["status"]), (name, what)
            if b["result"].tobytes() == want.tobytes():
                continue
            # a7 corners a float ulp apart: integers exact, reals within the a7 bar
            assert mt.record_integers(b["result"]) == mt.record_integers(want), (name, what)
            d = np.abs(mt.record_reals(b["result"]) - mt.record_reals(want))
            assert d[:, :19].max() <= REF_TOL_PX and d[:, 19:].max() <= F64_TOL_CR, (name, what, d.max())
        if golden is not None:
            assert int(golden["n_markers"]) >= 1, name
    assert statuses == {mt.OK, mt.NO_CORNER}
