"""Frames of dark quad pairs on a bright ground for the rare branches of stages a5-a10 (`tests/marker_testlib.py`,
`tests/refine_testlib.py`): a deterministic numpy renderer (no random numbers), 1152 x 720 unless said otherwise.  Every frame is
tagged with the branches it is meant to reach, as counters of the statement's trace; `test_back_stages_cpu.py` asserts from the
trace that each tag was reached, so a frame that stops exercising its branch fails there.

A strip follows the layout of the reference's generator as `testkit/ctag_synth.h` describes it: columns of width L / 15, each two
dark quads around a bright gap whose centre lies at tl * L on the column's left edge and tr * L on its right edge; the cross ratio
of a side is 0.55 + 5 t (1 - t) for a gap of 0.2 L.  The pitch is 0.104 L instead of 0.1 L: three pitches are then 0.312 L, clear
of a8's `0.3 * |corner 0 - corner 5|` (:985), which an exact 0.1 L pitch would sit on.
"""
import math

import numpy as np

ROWS, COLS = 720, 1152
GROUND, DARK = 215, 25
PITCH, WIDTH = 0.104, 1.0 / 15
CR = (1.47, 1.54, 1.61, 1.68, 1.68, 1.61, 1.54, 1.47)
NO_INTERVAL = dict(tl=0.5, tr=0.5, hl=0.09, hr=0.09)  # cross ratio (t + h) (1 - t + h) / (2 h) = 1.934: above 1.68 + 0.1, in no interval of :1165-1189


def gap_centre(ident):
    """Gap centre (in L) of a half-code 0..7: the root of t (1 - t) = (cr - 0.55) / 5, the larger one for the long variants 4..7."""
    d = math.sqrt(1.0 - 4.0 * (CR[ident] - 0.55) / 5.0)
    return 0.5 * (1 + d) if ident >= 4 else 0.5 * (1 - d)


def fill(img, pts, level=DARK):
    """A convex polygon (x, y) at 4 x 4 samples per pixel, blended over what is there."""
    pts = np.asarray(pts, np.float64)
    rows, cols = img.shape
    x0, y0 = np.floor(pts.min(0)).astype(int) - 1
    x1, y1 = np.ceil(pts.max(0)).astype(int) + 1
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, cols), min(y1, rows)
    if x1 <= x0 or y1 <= y0:
        return
    s = (np.arange(4) + 0.5) / 4
    xs = (np.arange(x0, x1)[:, None] + s[None, :]).reshape(-1)
    ys = (np.arange(y0, y1)[:, None] + s[None, :]).reshape(-1)
    e0, e1 = pts[1] - pts[0], pts[2] - pts[1]
    sign = 1.0 if e0[0] * e1[1] - e0[1] * e1[0] >= 0 else -1.0
    inside = np.ones((len(ys), len(xs)), bool)
    for i in range(len(pts)):
        a, b = pts[i], pts[(i + 1) % len(pts)]
        inside &= sign * ((b[0] - a[0]) * (ys[:, None] - a[1]) - (b[1] - a[1]) * (xs[None, :] - a[0])) >= 0
    cover = inside.reshape(y1 - y0, 4, x1 - x0, 4).sum((1, 3)) / 16.0
    box = img[y0:y1, x0:x1].astype(np.float64)
    img[y0:y1, x0:x1] = np.rint(box + (level - box) * cover).astype(np.uint8)


def column(tl, tr, hl=0.1, hr=0.1, dtop=0.0):
    return dict(tl=tl, tr=tr, hl=hl, hr=hr, dtop=dtop)


def code_column(code, **kw):
    return column(gap_centre(code // 8), gap_centre(code % 8), **kw)


def strip(img, cx, cy, theta_deg, L, columns, pitch=PITCH):
    """Columns (None: a missing one) of a strip of height L centred on (cx, cy), turned by theta_deg."""
    n = len(columns)
    W = ((n - 1) * pitch + WIDTH) * L
    c, s = math.cos(math.radians(theta_deg)), math.sin(math.radians(theta_deg))
    at = lambda u, v: (cx + c * (u - W / 2) - s * (v - L / 2), cy + s * (u - W / 2) + c * (v - L / 2))  # noqa: E731
    for k, col in enumerate(columns):
        if col is None:
            continue
        u0, u1, d = k * pitch * L, (k * pitch + WIDTH) * L, col["dtop"]
        gl, gr, hl, hr = (col[key] * L for key in ("tl", "tr", "hl", "hr"))
        fill(img, [at(u0, d), at(u1, d), at(u1, d + gr - hr), at(u0, d + gl - hl)])
        fill(img, [at(u0, d + gl + hl), at(u1, d + gr + hr), at(u1, d + L), at(u0, d + L)])


def box(img, cx, cy, w, h, theta_deg=0.0):
    c, s = math.cos(math.radians(theta_deg)), math.sin(math.radians(theta_deg))
    fill(img, [(cx + c * dx - s * dy, cy + s * dx + c * dy) for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))])


def window(state, row, first, n):
    return [int(state[row, (first + k) % state.shape[1]]) for k in range(n)]


CELLS = [(192 + 384 * (k % 3), 180 + 360 * (k // 3)) for k in range(6)]  # a 3 x 2 grid of 384 x 360 cells


def _blank(rows=ROWS, cols=COLS):
    return np.full((rows, cols), GROUND, np.uint8)


def carry_frame(state):
    """B3: features whose cross ratios lie in no interval, as the first feature of the frame, inside a marker and as the first
    feature of later markers."""
    img = _blank()
    odd = column(**NO_INTERVAL)
    for k, (cx, cy) in enumerate(CELLS[:4]):
        cols = [code_column(c) for c in window(state, 3 + 5 * k, 2 * k, 6)]
        cols[0] = odd
        if k % 2 == 0:
            cols[3] = odd
        strip(img, cx, cy + 8 * k, 0.0, 200.0, cols)  # each later strip starts lower: the first strip holds feature 0
    return img


def codes_frame(state):
    """Gap lengths more than 5 % apart (feature_ID -2, also in the reversed match), one and two columns missing in the middle,
    a strip of one feature, a strip whose best two coverages tie, a strip accepted at exactly min(0.8 legal, legal - 1)."""
    img = _blank()
    cols = [code_column(c) for c in window(state, 7, 0, 6)]
    cols[2] = code_column(window(state, 7, 0, 6)[2], hl=0.112, hr=0.09)
    strip(img, *CELLS[0], 0.0, 200.0, cols)
    cols = [code_column(c) for c in window(state, 11, 3, 6)]
    cols[2] = None
    strip(img, *CELLS[1], 0.0, 200.0, cols)
    w = window(state, 19, 5, 5)  # two columns missing at a pitch of 0.095 L: 0.285 L apart, joined by a8, and a gap of round(1.9) = 2
    strip(img, *CELLS[2], 0.0, 200.0, [code_column(w[0]), code_column(w[1]), None, None, code_column(w[3]), code_column(w[4])], pitch=0.095)
    strip(img, CELLS[3][0] - 120, CELLS[3][1], 0.0, 200.0, [code_column(int(state[23, 0]))])  # shorter than featureSize
    # one known code and one -2: the known code stands in many places of the dictionary (codes of short halves only: a4 drops
    # the quads of a long-variant column with unequal gap sides)
    w = next(w for w in (window(state, r, 4, 2) for r in range(29, state.shape[0])) if all(c // 8 < 4 and c % 8 < 4 for c in w))
    strip(img, CELLS[3][0] + 63, CELLS[3][1] + 1, 0.0, 210.0, [code_column(w[0]), code_column(w[1], hl=0.112, hr=0.09)])
    w = window(state, 31, 1, 5)
    w[2] = (w[2] + 8) % 64 if (w[2] // 8) % 4 != 3 else (w[2] - 8) % 64  # another left half: 4 of 5 legal codes match
    strip(img, *CELLS[4], 0.0, 200.0, [code_column(c) for c in w])
    cols = [code_column(c) for c in window(state, 37, 6, 6)]
    cols[1] = code_column(window(state, 37, 6, 6)[1], hl=0.112, hr=0.09)
    strip(img, *CELLS[5], 180.0, 200.0, cols)  # upside down: decoded by the reversed match, with a -2 in its code
    return img


def angles_frame(state):
    """Mean long-edge angles on both sides of 45 and of 135 degrees (:1034), a strip lying on its side (the swap of :1058) and one
    upside down (`inverse`)."""
    img = _blank()
    for k, theta in enumerate((-48.0, -42.0, 42.0, 48.0, 90.0, 180.0)):
        strip(img, *CELLS[k], theta, 190.0, [code_column(c) for c in window(state, 2 + 6 * k, k, 5)])
    return img


CHAIN_RANK = (0, 2, 3, 1, 5, 6, 4)  # feature index by position in the line: leaves father[0] one step below its root (:986-1004)


def pairs_frame(state):
    """Quad pairs that fail one clause of :543-548 each (clause 0 cannot fail alone: both quads no longer than wide makes :546
    fail too), three quads in a column, three in a row where the greedy first match decides, and a line of columns whose tops are
    staggered so that the label order leaves father[0] pointing at a feature that is not the root."""
    img = _blank()
    # (dark regions stay at most 30 px wide: the adaptive threshold hollows out wider ones)
    # :544 edge angles more than 50 degrees apart: the far end of the lower quad is cut at 57 degrees
    fill(img, [(60, 60), (86, 60), (86, 160), (60, 160)])
    fill(img, [(60, 176), (86, 176), (86, 320), (60, 280)])
    # :545 short sides more than 33 % apart
    box(img, 200, 110, 20, 100)
    box(img, 200, 226, 30, 100)
    # :546 long sides together no longer than the short ones
    box(img, 300, 84, 30, 36)
    box(img, 300, 124, 30, 16)
    # :547 long sides 15 times the short ones
    box(img, 400, 160, 12, 190)
    box(img, 400, 360, 12, 190)
    # :548 too far apart
    box(img, 480, 100, 30, 80)
    box(img, 480, 270, 30, 80)
    # three in a row
    for k in range(3):
        box(img, 580, 110 + 116 * k, 30, 100)
    # the greedy first match decides: the middle box starts one block row above its neighbours, so it has the lowest label of the
    # three and both neighbours pass :543-548 with it; it takes the left one (next in label order) and never asks the right one
    box(img, 760, 362, 100, 30)
    box(img, 876, 358, 100, 30)
    box(img, 992, 362, 100, 30)
    w = window(state, 5, 0, 7)
    strip(img, 880, 130, 0.0, 200.0, [code_column(w[k], dtop=6.0 * CHAIN_RANK[k]) for k in range(7)])  # its first column is the topmost shape: feature 0
    strip(img, 300, 560, 0.0, 200.0, [code_column(c) for c in window(state, 9, 2, 8)])
    strip(img, 800, 570, 0.0, 200.0, [code_column(c) for c in window(state, 13, 4, 8)])
    return img


def fan_frame(state):
    """a8's `||` of :985 has `threshold_angle * 2` on one side and `threshold_angle` on the other.  Columns lying on their sides, two to
    a group, 0.2 L apart: the upper one level, so that its left quad is labelled first, the lower one turned so that its right quad
    starts higher and is labelled first: their feature angles are opposite, and differ from 180 degrees by the turn.  A turn of 4.2
    degrees joins the pair through the 180 clause alone; 7.5 degrees lies between threshold_angle and twice it: not joined."""
    img = _blank()
    w = window(state, 15, 0, 8)
    for k, turn in enumerate((4.2, 7.5, -4.2, -7.5)):
        cx, cy = CELLS[k if k < 3 else 4]
        strip(img, cx, cy - 20, 90.0, 200.0, [code_column(w[2 * k])])
        strip(img, cx, cy + 20, 90.0 + turn, 200.0, [code_column(w[2 * k + 1])])
    return img


def many_frame(state):
    """Six whole strips: 72 features."""
    img = _blank()
    for k, (cx, cy) in enumerate(CELLS):
        strip(img, cx, cy, (0.0, 3.0, -4.0, 180.0, 2.0, -2.0)[k], 200.0, [code_column(c) for c in window(state, 4 + 6 * k, 0, 12)])
    return img


def borders_frame(state):
    """Columns that run into each border and corner of the frame (a7's out-of-bounds `continue` and the truncation of negative
    coordinates to 0 need a wide search, cornerSubPixDist 8 and 9), axis-aligned edges between corners at x.5 (the trace counts them), and a column with
    crenellated long sides (at cornerSubPixDist 0 most samples of such an edge see the same level on both sides)."""
    img = _blank()
    w = window(state, 6, 0, 12)
    for k, (cx, cy) in enumerate(((6, 6), (COLS - 7, 6), (6, ROWS - 7), (COLS - 7, ROWS - 7))):  # corners
        strip(img, cx + (60 if cx < 100 else -60), cy + (96 if cy < 100 else -96), 0.0, 200.0, [code_column(w[k]), code_column(w[k + 1])])
    strip(img, 400, 96, 0.0, 200.0, [code_column(c) for c in w[:3]])             # top
    strip(img, 700, ROWS - 97, 0.0, 200.0, [code_column(c) for c in w[3:6]])     # bottom
    strip(img, 96, 360, 90.0, 200.0, [code_column(c) for c in w[6:9]])           # left
    strip(img, COLS - 97, 360, 90.0, 200.0, [code_column(c) for c in w[9:12]])   # right
    strip(img, 400, 420, 0.0, 200.0, [code_column(c) for c in window(state, 8, 0, 4)])
    for x in (600, 640):  # crenellated columns: teeth of 4 px every 8 px on the long sides
        for ya, yb in ((330, 410), (440, 520)):
            box(img, x, (ya + yb) / 2, 20, yb - ya)
            for y in range(ya, yb, 8):
                box(img, x - 12, y + 2, 4, 4)
                box(img, x + 12, y + 6, 4, 4)
    return img


def textured_box(img, cx, cy, w, h):
    """A dark box the adaptive threshold keeps whole: a lighter 2 x 2 dot every 8 px keeps each of its tiles' maxima up."""
    box(img, cx, cy, w, h)
    x0, y0 = int(cx - w / 2), int(cy - h / 2)
    for y in range(y0 + 10, int(cy + h / 2) - 10, 8):
        for x in range(x0 + 10, int(cx + w / 2) - 10, 8):
            img[y:y + 2, x:x + 2] = 70


def long_edges_frame(state):
    """3840 x 2160: quad pairs with sides longer than 1032 px (`nsamples = max(128.0, mag / 8)` above 128) beside ordinary strips."""
    img = _blank(2160, 3840)
    for y in (300, 700):
        textured_box(img, 600, y, 1040, 72)
        textured_box(img, 1700, y, 1040, 72)
    strip(img, 3000, 500, 0.0, 400.0, [code_column(c) for c in window(state, 10, 0, 8)])
    strip(img, 1200, 1500, 20.0, 500.0, [code_column(c) for c in window(state, 20, 3, 10)])
    return img


# name -> (generator, the trace counters the frame is there for)
FRAMES = {
    "carry": (carry_frame, ("a9.carry_first_of_frame", "a9.carry_inside_marker", "a9.carry_first_of_marker")),
    "codes": (codes_frame, ("a9.id_minus_2", "a10.minus_2_in_code", "a10.accepted_with_gap_2",
                            "a10.short_marker", "a10.rejected_by_coverage_tie", "a10.accepted_at_exact_coverage", "a10.accepted_inverse")),
    "angles": (angles_frame, ("a8.direction_0_low", "a8.direction_1_mid", "a8.direction_0_high", "a9.swapped", "a10.accepted_inverse")),
    "pairs": (pairs_frame, ("a5.only_clause_1_fails", "a5.only_clause_2_fails", "a5.only_clause_3_fails", "a5.only_clause_4_fails",
                            "a5.only_clause_5_fails", "a5.first_match_wins", "a8.father_chain")),
    "fan": (fan_frame, ("a8.joined_by_180_clause_only", "a8.180_clause_between_T_and_2T")),
    "many": (many_frame, ("a8.features_65",)),
    "borders": (borders_frame, ("a7.out_of_bounds", "a7.negative_truncated_to_0", "a7.sample_unused", "a7.axis_aligned_edge_at_half_pixel")),
    "long_edges": (long_edges_frame, ("a7.long_edge",)),
}


def strip_frames_tagged(state):
    for name, (make, tags) in FRAMES.items():
        yield name, make(np.asarray(state)), tags
