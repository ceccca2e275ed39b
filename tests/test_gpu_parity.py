"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle and the committed
golden fixtures.  Bar: byte-identical result records (integer ids, positions, order AND float corners; the
north-star tolerance is 1e-3 px, we hold 0)."""
import os

import numpy as np
import pytest

import cylindertag_amd as ca
import testkit as tk
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, result_markers
from edge_testlib import random_shapes_frame as _random_shapes_frame  # shared with the CPU tests of stage a4
from sequences import avi_substitute

pytestmark = pytest.mark.gpu

CORNER_TOL_PX = 1e-3  # north_star tolerance; asserted in addition to byte equality where both are checked


def assert_same_record(got, want, what=""):
    assert got["status"] == want["status"], what
    assert got["n_markers"] == want["n_markers"] and got["n_features"] == want["n_features"], what
    n = int(want["n_features"])
    for f in ("pos", "id", "id_left", "id_right"):
        assert (got["features"][f][:n] == want["features"][f][:n]).all(), (what, f)
    assert (got["markers"][:want["n_markers"]] == want["markers"][:want["n_markers"]]).all(), what
    if n:
        assert np.abs(got["features"]["corners"][:n] - want["features"]["corners"][:n]).max() <= CORNER_TOL_PX, what
    assert got.tobytes() == want.tobytes(), what + " (byte equality)"


def test_device_math_is_bit_identical_to_host(detector, oracle):
    rng = np.random.RandomState(11)
    a = np.concatenate([rng.uniform(-1e3, 1e3, 40000), rng.uniform(-1, 1, 20000), [0.0, -0.0, 1.0, -1.0, 1e-30, 3.5e4]])
    b = np.concatenate([rng.uniform(-1e3, 1e3, 40000), rng.uniform(-1, 1, 20000), [1.0, -1.0, 0.0, 0.0, 1e30, -2.5]])
    for op in range(17):
        x, y = a, b
        if op in (3, 8):
            x = np.clip(a, -100, 80) if op == 3 else np.clip(a, -120, 80)
        if op == 15:  # the Welsch weights' form of exp32: non-positive arguments only
            x = np.concatenate([-np.abs(np.clip(a, -120, 120)), -np.exp(rng.uniform(-30, 4.8, 60000))])
            y = np.zeros_like(x)
        if op == 16:  # quotients through a shared reciprocal (ctm::div64): moments over weights, and harder ranges than the kernels see
            w = np.exp(rng.uniform(-40, 40, 300000))
            x = np.concatenate([rng.uniform(-4e3, 4e3, 300000) * w, np.exp(rng.uniform(-200, 200, 300000)) * rng.choice([-1.0, 1.0], 300000), np.zeros(1000)])
            y = np.concatenate([w, np.exp(rng.uniform(-200, 200, 300000)) * rng.choice([-1.0, 1.0], 300000), w[:1000]])
        if op == 4:
            x = np.clip(a, -1, 1).astype(np.float32).astype(np.float64)
        if op in (11, 13):
            x = np.abs(a)
        g, c = detector.math(op, x, y), oracle.math(op, x, y)
        assert g.tobytes() == c.tobytes(), "math op %d differs between gfx950 and x86-64" % op


def test_test_bmp_every_stage(detector, oracle, dictionary, test_bmp):
    state, fs = dictionary
    detector.set_option(capi.OPT_KEEP_PREMARKERS, 1)
    o = oracle.detect(test_bmp, state, fs)
    r = detector.detect(test_bmp)
    assert (detector.debug(0, tk.DBG_HALF).reshape(o["half"].shape) == o["half"]).all()
    lab = detector.debug(0, tk.DBG_LABELS).reshape(o["labels"].shape)
    assert ((lab > 0) == (o["binary"] > 0)).all()
    pairs = np.unique(np.stack([o["labels"].ravel(), lab.ravel()], 1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))  # same partition
    cand = detector.debug(0, tk.DBG_CANDIDATES)
    assert (cand[:, 0:5] == o["candidates"][:, 1:6]).all()  # area, bbox, in OpenCV label order
    assert (cand[:, 5] == o["candidates"][:, 6]).all() and (cand[:, 6] == o["candidates"][:, 7]).all()
    assert detector.debug(0, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes()
    for st, what in enumerate((tk.DBG_FEATURES0, tk.DBG_FEATURES1, tk.DBG_FEATURES2)):
        assert detector.debug(0, what).tobytes() == o["features"][st].tobytes()
    assert detector.debug(0, tk.DBG_PREMARKERS).tobytes() == o["premarkers"].tobytes()
    assert_same_record(r, o["result"], "test.bmp")
    assert [m["marker_id"] for m in result_markers(r)] == [23, 0, 1, 17, 5]


def test_golden_fixtures(detector, test_bmp, dictionary):
    g = np.load(os.path.join(GOLDEN, "golden_v1.npz"))
    state, fs = dictionary
    assert_same_record(detector.detect(test_bmp), g["bmp_result"][0], "golden test.bmp")
    seq = avi_substitute(test_bmp, 64)  # stand-in for the reference's missing test.avi (BASELINE config 2)
    res = detector.detect_batch(seq)
    for k in range(64):
        assert_same_record(res[k], g["seq_results"][k], "sequence frame %d" % k)
    syn = np.stack([tk.synth_frame_host(state, f)[0] for f in range(8)])
    res = detector.detect_batch(syn)
    for k in range(8):
        assert_same_record(res[k], g["synth_results"][k], "synthetic frame %d" % k)


@pytest.mark.parametrize("subpix,dist,tw", [(False, 3, 5), (True, 3, 5), (True, 5, 4), (True, 5, 7)])
def test_parameters(detector, oracle, dictionary, test_bmp, subpix, dist, tw):
    state, fs = dictionary
    img = test_bmp[60:1140]
    assert_same_record(detector.detect(img, tw, subpix, dist), oracle.detect_fast(img, state, fs, tw, subpix, dist),
                       "params subpix=%s dist=%d tw=%d" % (subpix, dist, tw))


def test_edge_cases(detector, oracle, dictionary, test_bmp):
    state, fs = dictionary
    blank = np.full((600, 800), 180, np.uint8)
    one = blank.copy()
    one[260:340, 300:330] = 10
    dark = np.zeros((400, 640), np.uint8)
    rng = np.random.RandomState(3)
    noise = rng.randint(0, 256, (360, 500)).astype(np.uint8)
    ragged = test_bmp[3:1001, 5:1711]  # 998 x 1706: not multiples of the CCL tile, the window or 16 bytes
    strided = np.ascontiguousarray(test_bmp[:, :1900])[:, :1888]
    # more accepted quads than k_features' all-pairs path holds (192): a marker frame plus a lattice of dark squares on
    # its bright areas -> the row-by-row path, with real features among the quads
    grid = tk.synth_frame_host(state, 7)[0].copy()
    for gy in range(20):
        for gx in range(24):
            y0, x0 = 20 + gy * 52 + (gx % 3), 20 + gx * 78 + (gy % 5)
            h, w = 22 + (gx + gy) % 7, 26 + (3 * gx + gy) % 9
            if grid[y0 - 6:y0 + h + 6, x0 - 6:x0 + w + 6].min() > 120:
                grid[y0:y0 + h, x0:x0 + w] = 20
    # 840 dark rectangles on a bright frame: > 2048 fitted edges, more than the one-wave-per-restart Welsch kernel of few-frame calls
    # holds -> the frame takes the batch kernel (k_welsch) although it arrives alone
    many = np.full((1080, 1920), 200, np.uint8)
    for gy in range(28):
        for gx in range(30):
            y0, x0 = 10 + gy * 38, 12 + gx * 63
            many[y0:y0 + 20 + (gx + gy) % 5, x0:x0 + 30 + (3 * gx + gy) % 7] = 25
    for name, img, want_status in (("blank", blank, 1), ("one quad", one, 2), ("all dark", dark, None),
                                   ("noise", noise, None), ("ragged", ragged, None), ("grid of squares", grid, None),
                                   ("840 rectangles", many, None)):
        got, want = detector.detect(img), oracle.detect_fast(img, state, fs)
        if want_status is not None:
            assert want["status"] == want_status
        assert_same_record(got, want, name)
    _stage_check(detector, oracle, state, fs, many, "840 rectangles, stage by stage")  # every fitted quad, not only the (empty) record
    # non-contiguous rows (row_stride > cols) through the raw ABI
    import ctypes as C
    res = np.zeros(1, ca.RESULT_DT)
    base = np.ascontiguousarray(test_bmp)
    st = detector.L.ctag_detect_u8(detector.h, base.ctypes.data, 1200, 1888, base.strides[0], 5, 1, 5, res.ctypes.data)
    assert st == 0
    assert_same_record(res[0], oracle.detect_fast(base[:, :1888], state, fs), "strided")


def test_odd_sizes_and_resize_row_tail(detector, oracle, dictionary, test_bmp):
    """Odd rows / cols: cv::resize to (cols/2, rows/2) is no longer an exact 2x, every output column and row has its
    own cubic taps (general kernel, host-built tap tables).  And the last hcols % 8 output columns are OpenCV's scalar
    row tail (round-half-up instead of the SIMD body's half-even) in both kernels."""
    state, fs = dictionary
    for name, img in (("odd width", test_bmp[:, :1919]), ("odd height", test_bmp[:1199, :1920]),
                      ("both odd", test_bmp[1:1200, 3:1914]), ("odd small", test_bmp[200:745, 300:1151])):
        img = np.ascontiguousarray(img)
        o = oracle.detect(img, state, fs)
        r = detector.detect(img)
        assert (detector.debug(0, tk.DBG_HALF).reshape(o["half"].shape) == o["half"]).all(), name
        assert_same_record(r, oracle.detect_fast(img, state, fs), name)
    # columns alternating 16 / 17 put every output pixel exactly on a rounding tie (V / 1024 = 16.5)
    tie = np.zeros((64, 2 * 853), np.uint8)
    tie[:, 0::2], tie[:, 1::2] = 16, 17
    want = oracle.resize_half(tie)
    assert (want[8:-8, 16:848] == 16).all() and (want[8:-8, 848:852] == 17).all()  # body: half-even, tail: half-up
    detector.detect(tie)
    assert (detector.debug(0, tk.DBG_HALF).reshape(want.shape) == want).all()
    # the general kernel on an even size equals the exact-2x kernel
    os.environ["CTAG_GENERAL_RESIZE"] = "1"
    try:
        detector.detect(tie)
        assert (detector.debug(0, tk.DBG_HALF).reshape(want.shape) == want).all()
        o = oracle.detect(test_bmp, state, fs)
        detector.detect(test_bmp)
        assert (detector.debug(0, tk.DBG_HALF).reshape(o["half"].shape) == o["half"]).all()
    finally:
        del os.environ["CTAG_GENERAL_RESIZE"]


def test_random_shapes_fuzz(detector, oracle, dictionary):
    """Differential test on frames that are NOT markers: every stage the debug interface exposes (half image, label
    partition, candidate list in OpenCV order, per-candidate quads, features, result record) equals the oracle's."""
    state, fs = dictionary
    detector.set_option(capi.OPT_KEEP_PREMARKERS, 1)
    try:
        nseeds = int(os.environ.get("CTAG_FUZZ_SEEDS", "16"))  # raise for a longer hunt
        # seed 32: a 576-wide half image (one-column last threshold tile) whose neighbour tile once read stale extrema
        for seed in list(range(nseeds)) + ([32] if nseeds <= 32 else []):
            rows, cols = ((720, 1152), (540, 960), (1080, 1920), (601, 1023))[seed % 4]
            img = _random_shapes_frame(state, seed, rows, cols)
            o = oracle.detect(img, state, fs)
            r = detector.detect(img)
            what = "fuzz seed %d" % seed
            assert (detector.debug(0, tk.DBG_HALF).reshape(o["half"].shape) == o["half"]).all(), what
            lab = detector.debug(0, tk.DBG_LABELS).reshape(o["labels"].shape)
            assert ((lab > 0) == (o["binary"] > 0)).all(), what
            pairs = np.unique(np.stack([o["labels"].ravel(), lab.ravel()], 1), axis=0)
            assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])), what
            cand = detector.debug(0, tk.DBG_CANDIDATES)
            assert cand.shape[0] == o["candidates"].shape[0] and (cand[:, 0:7] == o["candidates"][:, 1:8]).all(), what
            assert detector.debug(0, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes(), what
            for st, which in enumerate((tk.DBG_FEATURES0, tk.DBG_FEATURES1, tk.DBG_FEATURES2)):
                assert detector.debug(0, which).tobytes() == o["features"][st].tobytes(), (what, st)
            assert_same_record(r, oracle.detect_fast(img, state, fs), what)
    finally:
        detector.set_option(capi.OPT_KEEP_PREMARKERS, 0)


def test_components_across_tile_seams(detector, oracle, dictionary):
    """Dark blobs, bars and diagonal chains laid across the 320x30 CCL tile seams and their 4-tile corners (half-res
    x = 320, 640; y = 30, 60, ...): labels, areas, boxes and OpenCV order must equal the oracle's."""
    state, fs = dictionary
    rng = np.random.RandomState(21)
    img = np.full((1080, 1920), 200, np.uint8)
    for _ in range(160):
        cx = int(rng.choice([640, 1280])) + int(rng.randint(-40, 41))        # full-res column of a vertical seam
        cy = int(rng.randint(1, 17)) * 60 + int(rng.randint(-30, 31))         # full-res row of a horizontal seam
        w, h = int(rng.randint(4, 70)), int(rng.randint(4, 70))
        img[max(cy - h, 12):cy + h, max(cx - w, 12):cx + w] = 20
    for k in range(40):  # diagonal 2x2-pixel chains through tile corners (8-connectivity only)
        cx, cy = int(rng.choice([640, 1280])), int(rng.randint(1, 17)) * 60
        for t in range(-12, 12):
            x, y = cx + 2 * t, cy + (2 * t if k % 2 else -2 * t)
            img[y:y + 2, x:x + 2] = 20
    img[10:1070:7, 636:646] = 20  # thin bars crossing the vertical seam every few rows
    o = oracle.detect(img, state, fs)
    r = detector.detect(img)
    lab = detector.debug(0, tk.DBG_LABELS).reshape(o["labels"].shape)
    assert ((lab > 0) == (o["binary"] > 0)).all()
    pairs = np.unique(np.stack([o["labels"].ravel(), lab.ravel()], 1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
    cand = detector.debug(0, tk.DBG_CANDIDATES)
    assert len(cand) == len(o["candidates"]) and (cand[:, 0:5] == o["candidates"][:, 1:6]).all()
    assert_same_record(r, o["result"], "seam stress")


def _stage_check(detector, oracle, state, fs, img, what):
    o = oracle.detect(img, state, fs)
    r = detector.detect(img)
    lab = detector.debug(0, tk.DBG_LABELS).reshape(o["labels"].shape)
    assert ((lab != 0) == (o["binary"] > 0)).all(), what
    pairs = np.unique(np.stack([o["labels"].ravel(), lab.ravel()], 1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])), what  # same partition
    cand = detector.debug(0, tk.DBG_CANDIDATES)
    assert cand.shape[0] == o["candidates"].shape[0] and (cand[:, 0:7] == o["candidates"][:, 1:8]).all(), what
    assert detector.debug(0, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes(), what
    assert_same_record(r, o["result"], what)
    return o, r, lab


def test_dense_speckle_and_texture_take_the_second_ccl_pass(detector, oracle, dictionary):
    """Frames the reference labels without complaint but whose 320x30 CCL tiles do not fit the first pass's LDS caps (2048 row
    runs, 640 components) or whose specks would fill the frame's component pool: dark sensor noise (about half of the
    pixels below the local mid level), a noise band beside real markers, a lattice of dots.  Such tiles go through the
    overflow list to k_threshold_ccl_big; the frame must come out exactly as the oracle's, never as CTAG_ERR_LIMIT."""
    state, fs = dictionary
    rng = np.random.RandomState(41)
    detector.set_option(capi.OPT_KEEP_PREMARKERS, 1)
    try:
        # 1. dark sensor noise: every tile overflows the run cap
        dark = np.clip(rng.normal(22, 7, (540, 960)), 0, 255).astype(np.uint8)
        o, r, lab = _stage_check(detector, oracle, state, fs, dark, "dark noise")
        assert r["flags"] == 0 and (lab < 0).sum() > 100  # unpublished specks got private labels
        runs = (np.diff((o["binary"] > 0).astype(np.int8), axis=1, prepend=0) == 1)[:30, :320].sum()
        assert runs > 2048  # the first tile really exceeds the first pass
        # 2. a marker frame with a band of dark noise (640 x 60 and more): the markers elsewhere are still decoded
        frame, truth = tk.synth_frame_host(state, 11)
        band = frame.copy()
        band[300:420, 200:1500] = np.clip(rng.normal(25, 8, (120, 1300)), 0, 255).astype(np.uint8)
        o, r, lab = _stage_check(detector, oracle, state, fs, band, "noise band beside markers")
        assert r["status"] == 0 and r["flags"] == 0 and r["n_markers"] >= 2
        # 3. a lattice of 2x2 half-res dots around the markers of a 1080p frame: ~600 specks per tile fit the first pass, but
        # 54 tiles of them do not fit the frame's component pool -> the tiles that find it full are handed over and the
        # second pass publishes only what can matter
        dots, truth = tk.synth_frame_host(state, 12)
        dots = dots.copy()
        yy, xx = np.mgrid[0:1080, 0:1920]
        lattice = ((yy % 8) < 4) & ((xx % 8) < 4)
        for k in range(truth["n_markers"]):
            c = truth["corners"][k].reshape(4, 2)
            x0, y0, x1, y1 = c[:, 0].min() - 24, c[:, 1].min() - 24, c[:, 0].max() + 24, c[:, 1].max() + 24
            lattice &= ~((xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1))
        dots[lattice] = 15
        o, r, lab = _stage_check(detector, oracle, state, fs, dots, "dot lattice")
        assert r["status"] == 0 and r["flags"] == 0 and r["n_markers"] >= 2 and len(o["areas"]) - 1 > 13824
    finally:
        detector.set_option(capi.OPT_KEEP_PREMARKERS, 0)


def _draw_polyline(img, pts, width, value=12):
    """dark polyline of the given full-resolution width"""
    for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
        n = int(max(abs(x1 - x0), abs(y1 - y0))) + 1
        xs = np.linspace(x0, x1, n).round().astype(int)
        ys = np.linspace(y0, y1, n).round().astype(int)
        for dy in range(width):
            for dx in range(width):
                img[np.clip(ys + dy, 0, img.shape[0] - 1), np.clip(xs + dx, 0, img.shape[1] - 1)] = value


def test_long_thin_components_take_the_whole_wave_builds(detector, oracle, dictionary):
    """Components whose boundary does not fit a pack's LDS budget get a wave of their own: the 32 KB build (membership bitmap
    over the CCL tiles the box touches) and, beyond 8192 working-set words, the 144 KB build; a box over more than 96 tiles
    falls back to the gather test.  A 3840x2160 frame with a corner-to-corner band (both), a zig-zag with several labels per
    tile, a comb whose teeth join below a tile border, and a spiral; and the same shapes at 1080p around real markers."""
    state, fs = dictionary
    detector.set_option(capi.OPT_KEEP_PREMARKERS, 1)
    try:
        big = np.full((2160, 3840), 205, np.uint8)
        big[::7, ::5] = 190  # a little texture
        _draw_polyline(big, [(120, 90), (3700, 2050)], 6)                                        # ~2000 half-res points long
        _draw_polyline(big, [(150 + 90 * k, 1700 + (260 if k % 2 else 0)) for k in range(30)], 6)   # zig-zag
        for k in range(14):                                                                        # comb: teeth ...
            _draw_polyline(big, [(2300 + 60 * k, 200), (2300 + 60 * k, 560)], 8)
        _draw_polyline(big, [(2300, 560), (2300 + 60 * 13 + 8, 560)], 8)                           # ... joined at the bottom
        sp = [(3000 + int(r * np.cos(a)), 1400 + int(r * np.sin(a))) for a, r in ((0.35 * k, 30 + 9 * k) for k in range(60))]
        _draw_polyline(big, sp, 6)
        o, r, lab = _stage_check(detector, oracle, state, fs, big, "4K long thin components")
        cand = o["candidates"]
        w, h = cand[:, 4] - cand[:, 2] + 1, cand[:, 5] - cand[:, 3] + 1
        need = ((w + 1) & ~1) + 2 * h + 2 * (np.minimum(2 * (w + h), w * h) + 1) + 4
        assert (need > 8192).any() and ((need > 5120) & (need <= 8192)).any()  # both whole-wave builds had work
        frame, truth = tk.synth_frame_host(state, 21)
        hd = frame.copy()
        _draw_polyline(hd, [(40, 6), (1880, 40)], 5)  # a long shallow band along the top: a wave of its own, bitmap over 6 tiles
        for k in range(10):
            _draw_polyline(hd, [(60 + 44 * k, 60), (60 + 44 * k, 300)], 6)
        _draw_polyline(hd, [(60, 300), (60 + 44 * 9 + 6, 300)], 6)
        # a long band through CCL tiles that took the second labelling pass (400 specks on each tile's top row: more than the 128
        # labels the membership table covers) -> its label there is "ask root_of": the table-only scan flags it and the rescan build runs
        sp2 = np.full((1080, 1920), 205, np.uint8)
        for row in (300, 360, 420):
            for x in range(100, 1800, 4):
                sp2[row:row + 2, x:x + 2] = 0
        _draw_polyline(sp2, [(100, 310), (1800, 470)], 7)
        o, r, lab = _stage_check(detector, oracle, state, fs, sp2, "band through second-pass tiles")
        assert len(o["candidates"]) == 1 and (o["binary"][150] > 0).sum() > 128
        o, r, lab = _stage_check(detector, oracle, state, fs, hd, "1080p shapes beside markers")
        cand = o["candidates"]
        w, h = cand[:, 4] - cand[:, 2] + 1, cand[:, 5] - cand[:, 3] + 1
        assert r["status"] == 0 and (((w + 1) & ~1) + 2 * h + 2 * (np.minimum(2 * (w + h), w * h) + 1) + 4 > 2560).any()
    finally:
        detector.set_option(capi.OPT_KEEP_PREMARKERS, 0)


def _zoomed_marker_frame(oracle, state, fs, seed, k):
    """A 3840x2160 frame holding one planted marker of synthetic frame `seed`, enlarged k times (bilinear)."""
    from scipy.ndimage import zoom
    img, _ = tk.synth_frame_host(state, seed)
    r = oracle.detect_fast(img, state, fs)
    m = r["markers"][0]
    c = r["features"][m["first_feature"]:m["first_feature"] + m["n_features"]]["corners"].reshape(-1, 2)
    x0, y0 = np.maximum(c.min(0) - 12, 0).astype(int)
    x1, y1 = (c.max(0) + 12).astype(int)
    up = np.clip(zoom(img[y0:y1, x0:x1].astype(np.float32), k, order=1), 0, 255).astype(np.uint8)
    big = np.full((2160, 3840), 205, np.uint8)
    hh, ww = min(2160, up.shape[0]), min(3840, up.shape[1])
    big[:hh, :ww] = up[:hh, :ww]
    return big


def test_feature_edges_longer_than_1024_px(detector, oracle, dictionary):
    """edgeRefine (corner_detector.cpp:626-733) samples one point per pixel of an edge; the batch form's two kernels hold 1024
    samples per edge, and a quad with a longer edge flags its frame for k_edge_refine_long (the one-kernel form, which loops).
    Markers enlarged 5x in 4K frames have feature edges of 1110-1175 px: as single frames (few-frame path) and inside a batch
    next to ordinary frames, the records equal the oracle's."""
    state, fs = dictionary
    frames = []
    for i, seed in enumerate((22, 23, 21)):
        frames.append(_zoomed_marker_frame(oracle, state, fs, seed, 5.0))
        frames.append(tk.synth_frame_host(state, 40 + i, rows=2160, cols=3840)[0])
    want = [oracle.detect_fast(f, state, fs) for f in frames]
    longest = []
    for w in want[0::2]:
        c = w["features"][:w["n_features"]]["corners"].reshape(-1, 8, 2)
        assert len(c) >= 4
        longest.append(np.linalg.norm(c - np.roll(c, -1, axis=1), axis=2).max())
    assert min(longest) > 1060, longest
    assert all(w["n_markers"] >= 1 for w in want)
    for i in (0, 2):
        assert_same_record(detector.detect(frames[i]), want[i], "long edges, single frame %d" % i)
    got = detector.detect_batch(np.stack(frames))
    for i in range(len(frames)):
        assert_same_record(got[i], want[i], "long edges, batch frame %d" % i)


def test_many_markers_per_frame(detector, oracle, dictionary):
    """6 and 8 planted markers: 71-96 features per frame, i.e. both register halves of k_markers' wave-resident union-find / group
    numbering / rank sort (feature k lives in lane k & 63 of one of two registers) and its feature cap (100) within reach; one frame
    per call and as a batch."""
    state, fs = dictionary
    frames = [tk.synth_frame_host(state, idx, markers=mk)[0] for mk in (6, 8) for idx in (5, 6, 7, 8)]
    want = np.array([oracle.detect_fast(f, state, fs) for f in frames])
    assert (want["n_features"] > 64).all() and want["n_features"].max() >= 95 and (want["status"] == 0).all()
    for k, f in enumerate(frames):
        assert_same_record(detector.detect(f), want[k], "many markers, frame %d alone" % k)
    got = detector.detect_batch(np.stack(frames))
    for k in range(len(frames)):
        assert_same_record(got[k], want[k], "many markers, frame %d in the batch" % k)


def test_batch_equals_single_and_is_repeatable(detector, dictionary):
    state, fs = dictionary
    frames = np.stack([tk.synth_frame_host(state, 100 + f)[0] for f in range(6)])
    a = detector.detect_batch(frames)
    b = detector.detect_batch(frames[::-1].copy())[::-1]
    assert a.tobytes() == b.tobytes()  # results do not depend on batch order / neighbours
    detector.set_option(capi.OPT_MAX_CHUNK, 4)  # 6 frames in chunks of 4 + 2
    c = detector.detect_batch(frames)
    detector.set_option(capi.OPT_MAX_CHUNK, 1024)
    assert a.tobytes() == c.tobytes()
    for k in range(6):
        assert a[k].tobytes() == detector.detect(frames[k]).tobytes()


def test_graph_replay_option_gives_identical_records(detector, dictionary):
    """CTAG_OPT_GRAPH: the per-chunk kernel chain captured once and replayed as a hipGraph (off by default: no measured gain)
    returns the same bytes, across repeated calls, changing inputs behind the same pointers, and a changed batch size."""
    import torch
    state, fs = dictionary
    n, rows, cols = 24, 1080, 1920
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 900, n, rows, cols, cols, rows * cols)
    out = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")

    def run(m):
        out.zero_()
        torch.cuda.synchronize()
        detector.detect_batch_device(frames.data_ptr(), m, rows, cols, cols, rows * cols, out.data_ptr())
        detector.sync()
        return out[:m].cpu().numpy().tobytes()

    detector.set_option(capi.OPT_GRAPH, 0)
    want24, want7, want1, want3 = run(24), run(7), run(1), run(3)
    detector.set_option(capi.OPT_GRAPH, 1)
    try:
        assert run(24) == want24 and run(24) == want24 and run(7) == want7 and run(24) == want24
        # few-frame calls fork the boundary kernels onto a second stream: the fork / join is captured with the chain
        assert run(1) == want1 and run(3) == want3 and run(1) == want1 and run(3) == want3
        detector.synth_frames_device(frames.data_ptr(), 950, n, rows, cols, cols, rows * cols)  # new content, same pointers
        got = run(24)
        detector.set_option(capi.OPT_GRAPH, 0)
        assert got == run(24) and got != want24
        got1, got3 = run(1), run(3)
        detector.set_option(capi.OPT_GRAPH, 2)  # the default: few-frame calls only, from the second identical call on
        assert run(1) == got1 and run(1) == got1 and run(1) == got1 and run(3) == got3 and run(3) == got3 and run(24) == got
    finally:
        detector.set_option(capi.OPT_GRAPH, 2)


def test_whole_wave_components_give_identical_records(detector, oracle, dictionary, test_bmp):
    """CTAG_OPT_WAVE_POINTS moves components from the packed boundary kernel (8 lanes each) to the whole-wave builds
    (64 lanes, the 64-step speculative expand_line): any split returns the same bytes as the batch default, which equals the oracle;
    calls of up to 4 frames (the automatic latency mode: fork / join on a second stream) do too."""
    import torch
    state, fs = dictionary
    n, rows, cols = 24, 1080, 1920
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 0, n - 4, rows, cols, cols, rows * cols)
    for k in range(4):  # camera content: the reference's frame, shifted
        frames[n - 4 + k] = torch.from_numpy(np.ascontiguousarray(test_bmp[31 * k:31 * k + rows])).cuda()
    torch.cuda.synchronize()
    out = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")

    def run(first, m):
        out.zero_()
        torch.cuda.synchronize()
        detector.detect_batch_device(frames[first:].data_ptr(), m, rows, cols, cols, rows * cols, out.data_ptr())
        detector.sync()
        return out[:m].cpu().numpy().view(ca.RESULT_DT).reshape(m)

    want = run(0, n)
    host = frames.cpu().numpy()
    for k in (0, 11, n - 4, n - 1):
        assert want[k].tobytes() == oracle.detect_fast(host[k], state, fs).tobytes(), k
    assert (want["status"] == 0).all() and want["n_markers"].sum() >= 2 * n
    try:
        for wp in (1, 24, 60, 200, 1000):
            detector.set_option(capi.OPT_WAVE_POINTS, wp)
            assert run(0, n).tobytes() == want.tobytes(), wp
        detector.set_option(capi.OPT_WAVE_POINTS, 0)
        for first, m in ((0, 1), (5, 3), (n - 4, 4), (n - 1, 1), (n - 2, 2)):  # automatic latency mode
            assert run(first, m).tobytes() == want[first:first + m].tobytes(), (first, m)
    finally:
        detector.set_option(capi.OPT_WAVE_POINTS, 0)


def test_decoder_paths_on_other_dictionary_shapes(oracle, dictionary, test_bmp):
    """k_markers counts code matches bit-parallel over the dictionary's columns (<= 32 columns: a row per lane, symbol -> column-set
    table built per handle) and hypothesis by hypothesis otherwise.  Dictionaries of 12, 24 and 36 columns (the reference's rows
    repeated, so the best match is ambiguous and every marker is rejected or kept exactly as the oracle decides), 7 columns
    (shorter than a code: the reversed walk leaves columns negative) and a 41 x 33 random one."""
    state, fs = dictionary
    frames = [test_bmp, tk.synth_frame_host(state, 3)[0], tk.synth_frame_host(state, 11)[0]]
    rng = np.random.RandomState(5)
    for name, st in (("12", state), ("24", np.tile(state, (1, 2))), ("36", np.tile(state, (1, 3))), ("7", np.ascontiguousarray(state[:, :7])),
                     ("33 random", rng.randint(0, 64, (41, 33)).astype(np.int32)), ("5 rows", np.ascontiguousarray(state[:5]))):
        st = np.ascontiguousarray(st, dtype=np.int32)
        det = tk.Detector(st, fs)
        try:
            for k, img in enumerate(frames):
                got, want = det.detect(img), oracle.detect_fast(img, st, fs)
                assert_same_record(got, want, "dictionary %s, frame %d" % (name, k))
        finally:
            det.close()


def test_streamed_host_batch(detector, oracle, dictionary):
    """ctag_detect_batch_u8 streams sub-chunks through two device slabs (upload of k+1 overlapping detection of k): the
    records equal the ORACLE's for pinned and pageable frame memory, odd sub-chunk counts and strided rows."""
    state, fs = dictionary
    n = 7
    frames = np.stack([tk.synth_frame_host(state, 300 + f)[0] for f in range(n)])
    want = np.array([oracle.detect_fast(f, state, fs) for f in frames])
    assert (want["status"] == 0).all() and want["n_markers"].sum() >= 2 * n
    pinned = ca.pinned_empty(frames.shape, np.uint8)
    pinned[...] = frames
    res = ca.pinned_empty((n,), ca.RESULT_DT)
    try:
        for sub in (1, 2, 3, 128):
            detector.set_option(capi.OPT_HOST_SUBCHUNK, sub)
            assert detector.detect_batch(frames).tobytes() == want.tobytes(), sub
            got = detector.detect_batch(pinned, out=res)
            assert got.tobytes() == want.tobytes(), sub
        # rows with padding (row_stride > cols) take the per-frame 2-D copy path
        detector.set_option(capi.OPT_HOST_SUBCHUNK, 2)
        padded = np.zeros((n, frames.shape[1], frames.shape[2] + 64), np.uint8)
        padded[:, :, :frames.shape[2]] = frames
        view = padded[:, :, :frames.shape[2]]
        r = np.zeros(n, ca.RESULT_DT)
        st = detector.L.ctag_detect_batch_u8(detector.h, view.ctypes.data, n, view.shape[1], view.shape[2], view.strides[1],
                                             view.strides[0], 5, 1, 5, r.ctypes.data)
        assert st == 0 and r.tobytes() == want.tobytes()
        # per-stage timers accumulate over the sub-chunks of one call (they used to report the last sub-chunk only)
        detector.set_option(capi.OPT_HOST_SUBCHUNK, 2)
        detector.set_option(capi.OPT_TIMING, 1)
        assert detector.detect_batch(pinned, out=res).tobytes() == want.tobytes()
        t4 = detector.timings()
        detector.set_option(capi.OPT_HOST_SUBCHUNK, 128)
        detector.detect_batch(pinned, out=res)
        t1 = detector.timings()
        assert all(v > 0 for v in t4.values()) and sum(t4.values()) > 0.5 * sum(t1.values())
    finally:
        detector.set_option(capi.OPT_TIMING, 0)
        detector.set_option(capi.OPT_HOST_SUBCHUNK, 128)


def test_batch_with_many_oversize_components(detector, oracle, dictionary):
    """Wide components: long bars (260-360 half-res px wide) take the packed contour kernel's multi-pass silhouette scan
    (128 columns per pass); very long thin ones exceed its LDS budget and go through the oversize kernel, whose
    persistent blocks each own one global scratch slot (the first implementation ran out of scratch at 64 per launch)."""
    state, fs = dictionary
    rng = np.random.RandomState(77)
    frames = []
    for f in range(24):
        img = (rng.randint(0, 7, (1080, 1920)) + 190).astype(np.uint8)
        for k in range(24):
            y = 20 + k * 43 + rng.randint(0, 6)
            x = rng.randint(10, 400)
            img[y:y + rng.randint(10, 16), x:x + rng.randint(520, 720)] = 25 + (f + k) % 20
        frames.append(img)
    # shallow diagonal lines: bounding boxes ~940 x 120 half-res px with ~2100 boundary points exceed the packed kernel's
    # LDS budget -> the oversize kernel (global scratch, one persistent block per slot)
    for f in (3, 17):
        img = frames[f]
        yy, xx = np.mgrid[0:1080, 0:1920]
        for k in range(3):
            d = yy - (150 + 300 * k + 0.125 * xx)
            img[(np.abs(d) < 3.0) & (xx > 20) & (xx < 1900)] = 30
    frames = np.stack(frames)
    got = detector.detect_batch(frames)
    assert (got["flags"] == 0).all()
    for f in (0, 3, 13, 17, 23):
        want = oracle.detect_fast(frames[f], state, fs)
        assert_same_record(got[f], want, "bars frame %d" % f)
        detector.detect(frames[f])
        o = oracle.detect(frames[f], state, fs)
        assert detector.debug(0, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes()
        assert o["candidates"].shape[0] >= 10


def test_full_size_batch_properties(detector, oracle, dictionary):
    """BASELINE config 3 at full size through the device-resident entry point: frames generated on the GPU equal
    the host generator, every frame decodes exactly its planted dictionary rows, a second pass is byte-identical,
    and a sample of frames equals the oracle."""
    import torch
    state, fs = dictionary
    n, rows, cols = 512, 1080, 1920
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 0, n, rows, cols, cols, rows * cols)
    host0, truth0 = tk.synth_frame_host(state, 0)
    assert (frames[0].cpu().numpy() == host0).all()
    out = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, out.data_ptr())
    detector.sync()
    a = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, out.data_ptr())
    detector.sync()
    b = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    assert a.tobytes() == b.tobytes()
    # the only flag a clean frame may carry is CODE_OVERFLOW (a marker whose code position ran past code[20] is
    # dropped); flagged frames are compared with the oracle below
    assert (a["status"] == 0).all() and ((a["flags"] & ~np.uint32(4)) == 0).all()
    exact, inexact = 0, []
    for f in range(n):
        truth = tk.synth_truth(state, f)
        planted = sorted(int(x) for x in truth["dict_row"][:truth["n_markers"]])
        found = sorted(int(x) for x in a[f]["markers"]["marker_id"][:a[f]["n_markers"]])
        exact += planted == found
        if planted != found:
            inexact.append(f)
        assert set(found) <= set(planted), f  # never a wrong id
    # a planted marker that does not come out (cylinder-compressed end columns are occasionally too narrow to decode) is the ALGORITHM's miss, not
    # this implementation's: every such frame must be the oracle's record byte for byte, like the sampled ones
    assert exact >= int(0.94 * n)  # measured: 489 of these 512 frames decode EVERY planted marker (95.5 %; of the bench's 16 384 planted markers 99.2 % come out)
    flagged = [int(f) for f in np.nonzero(a["flags"])[0][:4]]
    for f in sorted(set(list(range(0, n, 16)) + [17, 255, 511] + flagged + inexact)):
        assert_same_record(a[f], oracle.detect_fast(frames[f].cpu().numpy(), state, fs), "synthetic frame %d" % f)


def test_bench_config_chunk4096(detector, oracle, dictionary):
    """The configuration the headline number is quoted on (bench.py: 4096 device-generated 1080p frames, ONE pass with
    CTAG_OPT_MAX_CHUNK = 4096, a 14 GB workspace): its records equal the chunk-1024 run byte for byte, and 72 sampled frames
    (first, last, every 64th, flagged ones) equal the oracle."""
    import torch
    state, fs = dictionary
    n, rows, cols = 4096, 1080, 1920
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 0, n, rows, cols, cols, rows * cols)
    out = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    try:
        detector.set_option(capi.OPT_MAX_CHUNK, 4096)
        detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, out.data_ptr())
        detector.sync()
        big = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
        out.zero_()
        detector.set_option(capi.OPT_MAX_CHUNK, 1024)
        detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, out.data_ptr())
        detector.sync()
        small = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    finally:
        detector.set_option(capi.OPT_MAX_CHUNK, 1024)
    assert big.tobytes() == small.tobytes()
    assert (big["status"] == 0).all() and ((big["flags"] & ~np.uint32(4)) == 0).all()
    flagged = [int(f) for f in np.nonzero(big["flags"])[0][:4]]
    sample = sorted(set(list(range(0, n, 64)) + [1, 1023, 1024, 2047, 3071, 4094, 4095] + flagged))
    assert len(sample) >= 64
    host = {f: frames[f].cpu().numpy() for f in sample}
    del frames
    for f in sample:
        assert_same_record(big[f], oracle.detect_fast(host[f], state, fs), "chunk-4096 frame %d" % f)


def test_records_do_not_depend_on_the_internal_stream_split(detector, dictionary, oracle):
    """CTAG_OPT_STREAMS (include/ctag.h): a chunk runs whole on the handle's stream or as halves / thirds on internal streams and
    workspaces -- chunks of 448..1023 frames always whole -- and the records are the same bytes either way.  Sizes on both sides of every
    threshold (256, 448, 1024), a ragged one, and a sample of frames against the oracle."""
    import torch
    state, fs = dictionary
    rows, cols = 1080, 1920
    nmax = 1100
    frames = torch.empty((nmax, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 7000, nmax, rows, cols, cols, rows * cols)
    frames[3] = 180
    frames[300, 500:560, 900:930] = 10
    torch.cuda.synchronize()
    out = torch.zeros((nmax, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    def run(n, streams):
        detector.set_option(capi.OPT_STREAMS, streams)
        out.zero_()
        torch.cuda.synchronize()
        detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, out.data_ptr())
        detector.sync()
        return out[:n].cpu().numpy().tobytes()
    try:
        detector.set_option(capi.OPT_MAX_CHUNK, 2048)
        ref = run(nmax, 1)
        item = ca.RESULT_DT.itemsize
        for n in (255, 257, 447, 449, 777, 1023, 1025, nmax):
            for streams in (2, 3):
                assert run(n, streams) == ref[:n * item], "n %d streams %d" % (n, streams)
        rec = np.frombuffer(ref, dtype=ca.RESULT_DT)
        for f in (0, 3, 128, 300, 448, 776, 1024, nmax - 1):
            assert_same_record(rec[f], oracle.detect_fast(frames[f].cpu().numpy(), state, fs), "frame %d" % f)
    finally:
        detector.set_option(capi.OPT_STREAMS, 2)
        detector.set_option(capi.OPT_MAX_CHUNK, 1024)


def test_packed_shards_and_rccl_gather_single_rank(detector, dictionary):
    """include/ctag_gather.h on one GPU: k_pack / k_unpack equal the host restatement of the packed-shard format
    (cylindertag_amd/dist.py) on real detector records, and ctag_gather with a world-1 RCCL communicator (ncclCommInitRank +
    two ncclAllGather calls through the dlopen'ed librccl) returns the input list."""
    import torch
    from cylindertag_amd.dist import pack_records, unpack_records
    state, fs = dictionary
    n, rows, cols = 96, 1080, 1920
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 40, n, rows, cols, cols, rows * cols)
    frames[5] = 180      # "No corner detected!"
    frames[6] = 0
    frames[7, 500:560, 900:930] = 10
    torch.cuda.synchronize()  # torch's stream wrote the three frames; the detector runs on the library's own stream
    rec = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, rec.data_ptr())
    detector.sync()
    host = rec.cpu().numpy()
    assert len(set(host.view(ca.RESULT_DT).ravel()["status"])) >= 2
    cap = capi.packed_capacity(n)
    packed = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    nbytes = detector.pack_results(rec.data_ptr(), n, packed.data_ptr(), cap)
    want = pack_records(host)
    assert nbytes == want.size and (packed[:nbytes].cpu().numpy() == want).all()
    back = torch.full((n, ca.RESULT_DT.itemsize), 0xCD, dtype=torch.uint8, device="cuda")
    detector.unpack_results(packed.data_ptr(), n, back.data_ptr())
    detector.sync()
    assert (back.cpu().numpy() == host).all() and (unpack_records(want) == host).all()
    # empty shard
    assert detector.pack_results(rec.data_ptr(), 0, packed.data_ptr(), cap) == 16
    # the collective path: world 1
    detector.comm_init(capi.comm_unique_id(), 0, 1)
    try:
        out = torch.full((n, ca.RESULT_DT.itemsize), 0xEE, dtype=torch.uint8, device="cuda")
        detector.gather(rec.data_ptr(), n, n, out.data_ptr())
        assert (out.cpu().numpy() == host).all()
        lb, pb = detector.gather_last_bytes()
        assert lb == want.size and pb >= lb and pb < n * ca.RESULT_DT.itemsize // 2
        # two-phase form with the next detection enqueued in between
        out.fill_(0x11)
        detector.gather_begin(rec.data_ptr(), n, n)
        rec2 = torch.zeros_like(rec)
        detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, rec2.data_ptr())
        detector.gather_end(out.data_ptr())
        detector.gather_wait()
        detector.sync()
        assert (out.cpu().numpy() == host).all() and (rec2.cpu().numpy() == host).all()
        # bench.py's N > 1 pattern: steps alternate between two handles that gather through ONE communicator (the second attaches
        # to the first's); the gather of a step ends while the next step's detection (other handle, other stream) runs
        det2 = tk.Detector(state, fs)
        assert detector.comm_native() and not det2.comm_native()
        det2.comm_attach(detector.comm_native(), 0, 1)
        try:
            dets, recs, outs = [detector, det2], [torch.zeros_like(rec) for _ in range(2)], [torch.zeros_like(rec) for _ in range(2)]
            pending = None
            for k in range(5):
                d = dets[k % 2]
                d.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, recs[k % 2].data_ptr())
                if pending is not None:
                    dets[pending % 2].gather_end(outs[pending % 2].data_ptr())
                d.gather_begin(recs[k % 2].data_ptr(), n, n)
                pending = k
            dets[pending % 2].gather_end(outs[pending % 2].data_ptr())
            for d in dets:
                d.gather_wait()
                d.sync()
            assert (outs[0].cpu().numpy() == host).all() and (outs[1].cpu().numpy() == host).all()
        finally:
            det2.comm_destroy()
            det2.close()
    finally:
        detector.comm_destroy()


def test_gather_deadline_aborts_instead_of_hanging(dictionary):
    """a dead or late peer must make the gather FAIL, not hang.  On one GPU a late peer is a stream that does not
    advance: a stall kernel (testkit) holds the handle's stream, the gather stream behind it and so the all-gather of the sizes for
    3 s; with a 300 ms deadline ctag_gather_end returns CTAG_ERR_HIP well before that, names the deadline, the communicator is
    aborted (ncclCommAbort), the handle that shares it fails its next gather at once, and everything tears down without a hang.
    Without a deadline (0) the same stall only delays the result."""
    import time
    import torch
    state, fs = dictionary
    n, rows, cols = 8, 1080, 1920
    det, det2 = tk.Detector(state, fs), tk.Detector(state, fs)
    try:
        frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
        det.synth_frames_device(frames.data_ptr(), 3, n, rows, cols, cols, rows * cols)
        rec = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
        out = torch.zeros_like(rec)
        det.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, rec.data_ptr())
        det.sync()
        host = rec.cpu().numpy()
        det.comm_init(capi.comm_unique_id(), 0, 1)
        det2.comm_attach(det.comm_native(), 0, 1)
        # no deadline: a 400 ms stall delays the gather, nothing else
        det.gather_set_timeout(0)
        det.stall_stream(400)
        t0 = time.perf_counter()
        det.gather(rec.data_ptr(), n, n, out.data_ptr())
        assert time.perf_counter() - t0 > 0.3 and (out.cpu().numpy() == host).all()
        # a deadline longer than the stall: same
        det.gather_set_timeout(5000)
        det.stall_stream(400)
        det.gather(rec.data_ptr(), n, n, out.data_ptr())
        assert (out.cpu().numpy() == host).all()
        # a deadline shorter than the stall: the call fails within the deadline (plus scheduling slack), long before the stall ends
        det.gather_set_timeout(300)
        det.stall_stream(3000)
        det.gather_begin(rec.data_ptr(), n, n)
        t0 = time.perf_counter()
        with pytest.raises(capi.CtagError) as ei:
            det.gather_end(out.data_ptr())
        dt = time.perf_counter() - t0
        assert ei.value.status == capi.ERR_HIP and 0.25 < dt < 2.0, (ei.value, dt)
        assert "300 ms" in str(ei.value) and "aborted" in str(ei.value)
        # the communicator is dead for every handle that shares it
        for d in (det, det2):
            with pytest.raises(capi.CtagError) as e2:
                d.gather_begin(rec.data_ptr(), n, n)
            assert "aborted" in str(e2.value)
        # the detector itself is unharmed
        det.sync()
        det.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, out.data_ptr())
        det.sync()
        assert (out.cpu().numpy() == host).all()
        # a fresh communicator works again
        det2.comm_destroy()
        det.comm_destroy()
        det.comm_init(capi.comm_unique_id(), 0, 1)
        det.gather_set_timeout(-1)
        out.zero_()
        det.gather(rec.data_ptr(), n, n, out.data_ptr())
        assert (out.cpu().numpy() == host).all()
    finally:
        t0 = time.perf_counter()
        det2.comm_destroy()
        det.comm_destroy()
        det2.close()
        det.close()
        assert time.perf_counter() - t0 < 10


def _gathered_buffer(records, world, width=None):
    """What the payload all-gather of a `world`-rank job delivers for `records` (uint8 [n_total, 11616]): every rank's packed shard
    (cylindertag_amd/dist.pack_records, the host restatement of the format) at r * width, padding filled with 0xA5."""
    from cylindertag_amd.dist import pack_records, shard_range
    n_total = records.shape[0]
    shards = [pack_records(records[slice(*shard_range(n_total, r, world))]) for r in range(world)]
    w = (max(s.size for s in shards) + 255) & ~255
    width = w if width is None else width
    assert width >= w and width % 256 == 0
    buf = np.full(world * width, 0xA5, np.uint8)
    for r, sh in enumerate(shards):
        buf[r * width:r * width + sh.size] = sh
    return buf, width


def test_multi_rank_unpack_on_one_gpu(detector, dictionary):
    """The device path of ctag_gather_end that only a communicator of more than one rank reaches -- the segment table (shard bases
    r * width, per-shard offset tables, uneven and EMPTY shards) and k_unpack_scan / k_unpack over several segments -- executed on
    one GPU: the gathered buffer is built on the host from real detector records exactly as the payload all-gather would deliver
    it, and the unpacked list must equal the one-GPU list byte for byte (include/ctag_testkit.h: ctag_testkit_unpack_gathered)."""
    import torch
    n, rows, cols = 160, 1080, 1920
    frames = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
    detector.synth_frames_device(frames.data_ptr(), 700, n, rows, cols, cols, rows * cols)
    frames[3] = 180      # "No corner detected!"
    frames[4] = 0
    frames[9, 500:560, 900:930] = 10   # one component, no feature
    frames[n - 1] = 200  # the last frame of the last shard is an early return
    torch.cuda.synchronize()
    rec = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    detector.detect_batch_device(frames.data_ptr(), n, rows, cols, cols, rows * cols, rec.data_ptr())
    detector.sync()
    del frames
    base = rec.cpu().numpy()
    assert len(set(base.view(ca.RESULT_DT).ravel()["status"])) >= 2
    rng = np.random.RandomState(5)

    def check(records, world, width=None):
        buf, width = _gathered_buffer(records, world, width)
        n_total = records.shape[0]
        g = torch.from_numpy(buf).cuda()
        out = torch.full((max(n_total, 1), ca.RESULT_DT.itemsize), 0xEE, dtype=torch.uint8, device="cuda")
        detector.unpack_gathered(g.data_ptr(), n_total, world, width, out.data_ptr())
        got = out.cpu().numpy()[:n_total]
        assert got.shape == records.shape and (got == records).all(), "world %d, %d frames" % (world, n_total)

    big = base[rng.randint(0, n, 4099)]  # 4099 = 8 * 512 + 3: the first three ranks own one frame more
    big[-1] = base[n - 1]
    for world in (2, 4, 8):
        check(big, world)
    check(big[:1031], 8, width=((capi.packed_capacity(129) + 255) & ~255))  # a width far above the packed sizes
    check(base[:3], 8)     # ranks 3..7 own no frame at all
    check(base[:1], 2)
    check(base[3:6], 4)    # early returns only: shards without any payload
    check(base[:0], 4)     # an empty job
    check(base, 64)        # the largest world the segment table holds
    check(base, 1)
    with pytest.raises(ca.CtagError):
        detector.unpack_gathered(rec.data_ptr(), n, 65, 256, rec.data_ptr())
    with pytest.raises(ca.CtagError):
        detector.unpack_gathered(rec.data_ptr(), n, 2, 100, rec.data_ptr())  # width not a multiple of 256


def test_two_rank_rccl_gather_when_two_gpus_are_present(dictionary):
    """A TRUE two-rank ctag_gather (uneven shards, a zero-frame job, two handles sharing one communicator) whenever the box has two
    GPUs; the one-GPU boxes of this pool skip it (RCCL refuses two ranks on one device)."""
    import socket
    import subprocess
    import sys
    import torch
    from ctag_testlib import ROOT
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: RCCL refuses two ranks on one device")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "gather_worker.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "GATHER_WORKER_OK" in p.stdout
    # a peer that never reaches its collective: the other rank's ctag_gather returns CTAG_ERR_HIP within the deadline and exits non-zero
    import time
    cmd[-1:] = [os.path.join(ROOT, "tests", "gather_worker.py"), "--dead-peer"]
    cmd[cmd.index("--master-port") + 1] = str(port + 1 if port < 65000 else port - 1)
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, CTAG_GATHER_TIMEOUT_MS="3000"))
    assert p.returncode != 0 and "DEAD_PEER_DETECTED" in p.stdout + p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    assert time.perf_counter() - t0 < 120


def _colourise(gray, seed):
    """A BGR frame whose channels differ (so that a wrong channel order or weight shows) but whose OpenCV gray value keeps the
    scene: each channel = gray plus a smooth offset / noise, clipped."""
    rng = np.random.RandomState(seed)
    h, w = gray.shape
    yy, xx = np.mgrid[0:h, 0:w]
    g16 = gray.astype(np.int32)
    b = np.clip(g16 + 25 * np.sin(xx / 97.0) + rng.randint(-6, 7, gray.shape), 0, 255)
    g = np.clip(g16 - 10 * np.cos(yy / 61.0) + rng.randint(-3, 4, gray.shape), 0, 255)
    r = np.clip(g16 + 18 * np.sin((xx + yy) / 143.0) + rng.randint(-6, 7, gray.shape), 0, 255)
    return np.stack([b, g, r], 2).astype(np.uint8)


def test_bgr_ingest_equals_gray_path(detector, oracle, dictionary, test_bmp):
    """ctag_detect_*bgr8*: cvtColor(BGR2GRAY) of the reference's stream loop (main.cpp:36,52-54) on the device.  The gray image
    the device computed equals the oracle's fixed-point conversion byte for byte (incl. odd widths, unaligned rows), and the
    records equal the oracle's detect() on that gray image -- one frame, a streamed host batch and a device-resident batch."""
    import torch
    state, fs = dictionary
    bgr = _colourise(test_bmp, 1)
    want_gray = oracle.bgr2gray(bgr)
    assert np.abs(want_gray.astype(int) - test_bmp.astype(int)).max() < 40 and (want_gray != test_bmp).mean() > 0.5
    got = detector.detect_bgr(bgr)
    assert (detector.debug(0, tk.DBG_GRAY).reshape(want_gray.shape) == want_gray).all()
    assert_same_record(got, oracle.detect_fast(want_gray, state, fs), "colourised test.bmp")
    assert got["n_markers"] == 5
    # primary colours / extremes: the weights and the rounding
    prim = np.zeros((8, 16, 3), np.uint8)
    prim[0, :, 0] = 255
    prim[1, :, 1] = 255
    prim[2, :, 2] = 255
    prim[3] = 255
    prim[4, :, :] = np.arange(16)[:, None] * 17
    prim[5:] = np.random.RandomState(2).randint(0, 256, (3, 16, 3))
    detector.detect_bgr(prim)
    g = detector.debug(0, tk.DBG_GRAY).reshape(8, 16)
    assert (g == oracle.bgr2gray(prim)).all() and g[0, 0] == 29 and g[1, 0] == 150 and g[2, 0] == 76 and g[3, 0] == 255
    # odd sizes, a row stride that is not a multiple of 4 (the byte path), a strided view
    for (h, w) in ((301, 403), (64, 67)):
        a = _colourise(tk.synth_frame_host(state, 3, rows=h, cols=w)[0], 3)
        assert_same_record(detector.detect_bgr(a), oracle.detect_fast(oracle.bgr2gray(a), state, fs), "bgr %dx%d" % (w, h))
        assert (detector.debug(0, tk.DBG_GRAY).reshape(h, w) == oracle.bgr2gray(a)).all()
    # batches: synthetic frames colourised; host (pinned, sub-chunk 3 -> several uploads) and device-resident
    n, rows, cols = 10, 1080, 1920
    host = ca.pinned_empty((n, rows, cols, 3), np.uint8)
    grays = []
    for f in range(n):
        host[f] = _colourise(tk.synth_frame_host(state, 200 + f)[0], f)
        grays.append(oracle.bgr2gray(host[f]))
    want = [oracle.detect_fast(g, state, fs) for g in grays]
    detector.set_option(capi.OPT_HOST_SUBCHUNK, 3)
    try:
        res = detector.detect_batch_bgr(host)
    finally:
        detector.set_option(capi.OPT_HOST_SUBCHUNK, 128)
    for f in range(n):
        assert_same_record(res[f], want[f], "bgr host batch frame %d" % f)
    dev = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    out = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    detector.set_option(capi.OPT_MAX_CHUNK, 4)  # three chunks through one gray slab
    detector.set_option(capi.OPT_BGR_DIRECT, 0)  # the two-step form: k_bgr2gray into a gray image, then the chain
    try:
        detector.detect_batch_bgr_device(dev.data_ptr(), n, rows, cols, cols * 3, rows * cols * 3, out.data_ptr())
        detector.sync()
    finally:
        detector.set_option(capi.OPT_MAX_CHUNK, 1024)
        detector.set_option(capi.OPT_BGR_DIRECT, 1)
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    for f in range(n):
        assert_same_record(got[f], want[f], "bgr device batch frame %d" % f)
    assert (detector.debug(1, tk.DBG_GRAY).reshape(rows, cols) == grays[9]).all()  # the last chunk held frames 8, 9
    # a call of a few frames takes the two-step form by itself (round 6: the direct form's decimation is one block per frame band group,
    # 10x the latency of the short-band kernels a few gray frames get): the gray image exists, the records are the same
    out.zero_()
    detector.detect_batch_bgr_device(dev.data_ptr(), n, rows, cols, cols * 3, rows * cols * 3, out.data_ptr())
    detector.sync()
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    for f in range(n):
        assert_same_record(got[f], want[f], "bgr device batch of a few frames, frame %d" % f)
    assert (detector.debug(9, tk.DBG_GRAY).reshape(rows, cols) == grays[9]).all()
    # the direct form (batches -- here forced by CTAG_OPT_FUSED_SWEEP 2 -- of 1080p / 4K / 8K frames with 16-byte aligned rows): the decimation kernel and
    # edgeRefine read the BGR bytes themselves and convert as they load -- no gray image exists (the probe says so), the records are the same; in one
    # chunk and in chunks of 4
    detector.set_option(capi.OPT_FUSED_SWEEP, 2)
    for chunk in (1024, 4):
        detector.set_option(capi.OPT_MAX_CHUNK, chunk)
        try:
            out.zero_()
            detector.detect_batch_bgr_device(dev.data_ptr(), n, rows, cols, cols * 3, rows * cols * 3, out.data_ptr())
            detector.sync()
        finally:
            detector.set_option(capi.OPT_MAX_CHUNK, 1024)
        got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
        for f in range(n):
            assert_same_record(got[f], want[f], "bgr device batch, direct form, chunk %d, frame %d" % (chunk, f))
        with pytest.raises(ca.CtagError):
            detector.debug(0, tk.DBG_GRAY)
    # ... and replayed as a hipGraph (CTAG_OPT_GRAPH 1: every chunk): the graph's key carries the channel count
    detector.set_option(capi.OPT_GRAPH, 1)
    try:
        for rep in range(2):
            out.zero_()
            detector.detect_batch_bgr_device(dev.data_ptr(), n, rows, cols, cols * 3, rows * cols * 3, out.data_ptr())
            detector.sync()
            got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
            for f in range(n):
                assert_same_record(got[f], want[f], "bgr device batch, direct form, graph replay %d, frame %d" % (rep, f))
    finally:
        detector.set_option(capi.OPT_GRAPH, 2)
        detector.set_option(capi.OPT_FUSED_SWEEP, 1)
    # rows that are not 16-byte aligned (a 4-byte pad per row) take the two-step form by themselves
    padded = torch.zeros((n, rows, cols * 3 + 4), dtype=torch.uint8, device="cuda")
    padded[:, :, :cols * 3] = dev.reshape(n, rows, cols * 3)
    torch.cuda.synchronize()
    out.zero_()
    detector.detect_batch_bgr_device(padded.data_ptr(), n, rows, cols, cols * 3 + 4, rows * (cols * 3 + 4), out.data_ptr())
    detector.sync()
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    for f in range(n):
        assert_same_record(got[f], want[f], "bgr device batch, padded rows, frame %d" % f)
    del padded
    # a 4K BGR frame pair through the direct form (two waves per row: the seam lanes convert their halo pixels too)
    big = np.stack([_colourise(tk.synth_frame_host(state, 300 + f, rows=2160, cols=3840)[0], 5 + f) for f in range(2)])
    want4k = [oracle.detect_fast(oracle.bgr2gray(b), state, fs) for b in big]
    bdev = torch.from_numpy(big).cuda()
    out4k = torch.zeros((2, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    detector.detect_batch_bgr_device(bdev.data_ptr(), 2, 2160, 3840, 3840 * 3, 2160 * 3840 * 3, out4k.data_ptr())
    detector.sync()
    got = np.frombuffer(out4k.cpu().numpy().tobytes(), dtype=ca.RESULT_DT)
    for f in range(2):
        assert_same_record(got[f], want4k[f], "4K bgr frame %d, direct form" % f)
    del bdev, big
    with pytest.raises(ca.CtagError):
        detector.detect_batch_bgr_device(dev.data_ptr(), n, rows, cols, cols * 3 - 1, rows * cols * 3, out.data_ptr())  # stride < 3 * cols
    # a gray call afterwards leaves no stale gray view
    detector.detect(test_bmp)
    with pytest.raises(ca.CtagError):
        detector.debug(0, tk.DBG_GRAY)


def test_non_default_params(oracle, dictionary, test_bmp):
    """ctag_create_ex / ctag_params: the reference's member constants and literals (header/corner_detector.h:90,110,122,135-137,144;
    corner_detector.cpp:71,88,285) as a struct.  With values other than the reference's, the records still equal the oracle's, which
    takes the same struct -- every field moved at least once, and in at least one setting the result differs from the default run."""
    state, fs = dictionary
    frames = [test_bmp, tk.synth_frame_host(state, 21)[0], tk.synth_frame_host(state, 22)[0]]
    base = [oracle.detect_fast(f, state, fs) for f in frames]

    def variant(**kw):
        p = ca.default_params()
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    getattr(p, k)[i] = x
            else:
                setattr(p, k, v)
        return p

    settings = [
        variant(threshold_line=1.3, threshold_expand=0.9),
        variant(threshold_line=2.6, threshold_expand=1.7, collinear_cost=1.5),
        variant(collinear_cost=2.1, threshold_RAC=0.12),
        variant(threshold_RAC=0.05, threshold_angle=2.0, threshold_vertical=0.2),
        variant(threshold_angle=9.0, threshold_vertical=0.8),
        variant(dark_cap=0.2, area_min=60, area_max_fraction=0.002),
        variant(dark_cap=0.45, area_min=12, area_max_fraction=0.03),
        variant(dark_cap=0.12),
        variant(ID_cr_correspond=[1.45, 1.52, 1.63, 1.70], cr_covariance_left=[0.05, 0.02, 0.05, 0.03], cr_covariance_right=[0.03, 0.05, 0.02, 0.06]),
    ]
    differs = 0
    try:
        for k, p in enumerate(settings):
            det = tk.Detector(state, fs, params=p)
            oracle.set_params(p)
            try:
                for i, f in enumerate(frames):
                    want = oracle.detect_fast(f, state, fs)
                    assert_same_record(det.detect(f), want, "params setting %d frame %d" % (k, i))
                    differs += want.tobytes() != base[i].tobytes()
                batch = np.stack([tk.synth_frame_host(state, 21 + j)[0] for j in range(6)])  # more than kLatencyFrames: the batch kernels
                got = det.detect_batch(batch)
                for j in range(len(batch)):
                    assert_same_record(got[j], oracle.detect_fast(batch[j], state, fs), "params setting %d batch frame %d" % (k, j))
            finally:
                det.close()
    finally:
        oracle.set_params(None)
    assert differs >= len(settings)  # the settings do change results: the fields are live
    # the default struct through ctag_create_ex is ctag_create
    det = tk.Detector(state, fs, params=ca.default_params())
    assert_same_record(det.detect(test_bmp), base[0], "default params through ctag_create_ex")
    det.close()
    for bad in (variant(dark_cap=0.5), variant(dark_cap=0.0), variant(area_min=0), variant(threshold_line=0.0), variant(area_max_fraction=1.5)):
        with pytest.raises(ca.CtagError):
            tk.Detector(state, fs, params=bad)


def test_cpp_cylindertag_class_demo(oracle, dictionary, test_bmp):
    """The C++ `CylinderTag` host layer (reference class interface) end to end: the demo binary reads test.bmp with the
    C++ BMP reader, calls CylinderTag::detect(img, markers, 5, true, 5) and prints the MarkerInfo vector."""
    import subprocess
    from ctag_testlib import ROOT
    exe = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_demo")
    out = subprocess.check_output([exe, os.path.join(GOLDEN, "CTag_2f12c.marker"), os.path.join(GOLDEN, "test.bmp")], timeout=120).decode()
    lines = [l for l in out.splitlines() if l.startswith("id ")]
    state, fs = dictionary
    want = result_markers(oracle.detect_fast(test_bmp, state, fs))
    assert out.splitlines()[0] == "markers %d" % len(want) and len(lines) == len(want)
    for line, m in zip(lines, want):
        head, corners = line.split("|")
        toks = head.split()
        assert int(toks[1]) == m["marker_id"] and int(toks[3]) == len(m["id"])
        feats = [tuple(int(v) for v in t.split(":")) for t in toks[5:]]
        assert [f[0] for f in feats][:len(m["pos"])] == m["pos"]
        assert [f[1] for f in feats] == m["id_left"] and [f[2] for f in feats] == m["id_right"]
        xy = np.array([[float(v) for v in c.split(",")] for c in corners.split()], np.float32)
        assert (xy == m["corners"][:, 0:2]).all()
    # early return: a blank frame prints the reference's message and leaves the vector untouched
    blank = os.path.join(os.path.dirname(exe), "blank_test.bmp")
    w, h = 640, 480
    hdr = b"BM" + (54 + 1024 + w * h).to_bytes(4, "little") + bytes(4) + (54 + 1024).to_bytes(4, "little") + (40).to_bytes(4, "little")
    hdr += w.to_bytes(4, "little") + h.to_bytes(4, "little") + (1).to_bytes(2, "little") + (8).to_bytes(2, "little") + bytes(24)
    pal = b"".join(bytes([i, i, i, 0]) for i in range(256))
    open(blank, "wb").write(hdr + pal + bytes([180]) * (w * h))
    out = subprocess.check_output([exe, os.path.join(GOLDEN, "CTag_2f12c.marker"), blank], timeout=120).decode()
    assert "No corner detected!" in out and "markers 0" in out
    os.remove(blank)


def test_4k_frame(detector, oracle, dictionary):
    """BASELINE config 5 (detect only): a 3840x2160 synthetic frame (strips of 440..840 px) equals the oracle."""
    state, fs = dictionary
    frame, truth = tk.synth_frame_host(state, 2, rows=2160, cols=3840)
    got, want = detector.detect(frame), oracle.detect_fast(frame, state, fs)
    assert_same_record(got, want, "4K synthetic frame")
    assert sorted(int(m["marker_id"]) for m in want["markers"][:want["n_markers"]]) == sorted(int(x) for x in truth["dict_row"][:truth["n_markers"]])


def test_expand_line_filter_equals_exact_path(oracle, dictionary, test_bmp):
    """expand_line's distance test is decided from a filtered double-precision estimate unless the estimate lies within a band of the
    threshold (k_quad.hip: sg_expand_line).  CTAG_OPT_EXPAND_EXACT widens the band to infinity -- the reference's own refit at every
    step -- and both forms must give the oracle's quads, stage by stage, on camera content, synthetic frames, noise and with
    threshold_expand / threshold_line away from the reference's values."""
    state, fs = dictionary
    rng = np.random.RandomState(77)
    frames = [test_bmp[60:1140]] + [tk.synth_frame_host(state, 300 + k)[0] for k in range(12)]
    frames.append(np.clip(rng.normal(120, 60, (1080, 1920)), 0, 255).astype(np.uint8))
    batch = np.stack(frames)
    for kw in ({}, {"threshold_expand": 0.7, "threshold_line": 1.4}, {"threshold_expand": 2.2, "threshold_line": 2.5}):
        p = ca.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        oracle.set_params(p)
        try:
            want, _ = oracle.detect_many(batch, state, fs)
            for exact in (0, 1):
                det = tk.Detector(state, fs, params=p)
                det.set_option(capi.OPT_EXPAND_EXACT, exact)
                try:
                    got = det.detect_batch(batch)
                    for k in range(len(batch)):
                        assert_same_record(got[k], want[k], "expand %s exact=%d frame %d" % (kw, exact, k))
                    one = det.detect(batch[0])  # the few-frame builds (whole-wave components) too
                    assert_same_record(one, want[0], "expand %s exact=%d single" % (kw, exact))
                    o = oracle.detect(batch[3], state, fs)
                    det.detect(batch[3])
                    assert det.debug(0, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes()
                finally:
                    det.close()
        finally:
            oracle.set_params(None)
