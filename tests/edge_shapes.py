"""Deterministic frames of the topologies where a boundary walk (stage a4, `corner_detector.cpp:171-402`) goes wrong.

Shapes are drawn as half-res masks (x, y in the half image) and stamped into a 1920x1080 frame as 2x2 blocks: dark 30 on 200.
The exact 2x cubic decimation maps such a block pattern back onto the same half-res mask, and shapes at most a few pixels thick
keep a bright pixel in every 3x3-tile neighbourhood, so the threshold keeps the mask as drawn (`tests/test_edge_extraction_cpu.py`
checks the candidates each frame yields).  The outer 5 half-res pixels are background whatever is drawn there.
No binary fixtures: everything here is computed."""
import math

import numpy as np

ROWS, COLS = 1080, 1920
HR, HC = ROWS // 2, COLS // 2
AREA_LIMIT = math.floor(0.01 * HC * HR + 0.5)  # round(0.01 * cols * rows) of the half image: 5184
DARK, BRIGHT = 30, 200


def _canvas():
    return np.zeros((HR, HC), bool)


_TAGS = []  # (topology, x0, y0, x1, y1) of every shape the frame being made has drawn, clipped at the canvas edge


def _stamp(canvas, mask, x, y, tag=None):
    """OR a mask into the canvas with its top-left at (x, y), clipped at the canvas edge; `tag` names the topology it is for."""
    h, w = mask.shape
    x0, y0 = max(x, 0), max(y, 0)
    x1, y1 = min(x + w, HC), min(y + h, HR)
    if x1 > x0 and y1 > y0:
        canvas[y0:y1, x0:x1] |= mask[y0 - y:y1 - y, x0 - x:x1 - x]
        if tag:
            _TAGS.append((tag, x0, y0, x1 - 1, y1 - 1))


def _to_frame(canvas):
    img = np.where(canvas, DARK, BRIGHT).astype(np.uint8)
    return np.ascontiguousarray(np.kron(img, np.ones((2, 2), np.uint8)))


def _poly(pts, pad=2):
    """A convex polygon (half-res coordinates) rasterised at pixel centres; returns (mask, x0, y0)."""
    pts = np.asarray(pts, np.float64)
    x0, y0 = int(math.floor(pts[:, 0].min())) - pad, int(math.floor(pts[:, 1].min())) - pad
    x1, y1 = int(math.ceil(pts[:, 0].max())) + pad, int(math.ceil(pts[:, 1].max())) + pad
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
    inside = np.ones(xx.shape, bool)
    n = len(pts)
    area2 = sum(pts[i, 0] * pts[(i + 1) % n, 1] - pts[(i + 1) % n, 0] * pts[i, 1] for i in range(n))
    sign = 1.0 if area2 > 0 else -1.0
    for i in range(n):
        a, b = pts[i], pts[(i + 1) % n]
        inside &= sign * ((b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0])) >= 0
    return inside, x0, y0


def _rect_pts(cx, cy, w, h, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [(cx + c * dx - s * dy, cy + s * dx + c * dy) for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


def _outline(mask, t):
    """The pixels of a filled mask within t pixels (chessboard) of its outside: a band the threshold keeps whole."""
    m = np.pad(mask, t)
    inner = np.ones_like(m)
    for dy in range(-t, t + 1):
        for dx in range(-t, t + 1):
            inner &= np.roll(np.roll(m, dy, 0), dx, 1)
    return (m & ~inner)[t:-t, t:-t]


def _letter(kind):
    """U, C and E masks 24 px high, strokes 4 px, the concavity facing +x (right)."""
    m = np.zeros((24, 20), bool)
    m[:4, :] = m[-4:, :] = True
    m[:, :4] = True
    if kind == "U":  # open to the right, square inner corner
        pass
    elif kind == "C":  # the arms bend in: a narrower mouth
        m[4:7, 16:20] = m[17:20, 16:20] = True
    elif kind == "E":
        m[10:14, :14] = True
    return m


def _frame_letters():
    c = _canvas()
    x = 20
    for kind in ("U", "C", "E"):
        for k in range(4):  # the concavity faces right, up, left, down: the four scan directions
            _stamp(c, np.rot90(_letter(kind), k), x, 30 + 60 * (k % 2), "%s open %s" % (kind, ("right", "up", "left", "down")[k]))
            x += 40 if k % 2 else 0
        x += 40
    # rings: square, rotated square, circle; the inner boundary must not be walked
    sq = np.zeros((34, 34), bool)
    sq[:4, :] = sq[-4:, :] = sq[:, :4] = sq[:, -4:] = True
    _stamp(c, sq, 40, 200, "ring")
    m, x0, y0 = _poly(_rect_pts(140, 220, 36, 30, 30))
    _stamp(c, _outline(m, 3), x0, y0, "ring")
    yy, xx = np.mgrid[0:41, 0:41]
    d = np.hypot(xx - 20, yy - 20)
    _stamp(c, (d <= 20) & (d > 16), 220, 200, "ring")
    _stamp(c, (d <= 20) & (d > 14.5), 300, 200, "ring")  # a thicker ring: a different inner topology
    # pinch points: two blocks joined by one diagonal pixel; a blob with a one-pixel diagonal arm; a bow-tie
    a = np.zeros((21, 21), bool)
    a[:10, :10] = True
    a[11:, 11:] = True
    a[10, 10] = True
    _stamp(c, _outline(a, 2) | np.eye(21, dtype=bool), 400, 200, "pinch")
    b = np.zeros((30, 30), bool)
    b[:12, :12] = True
    b[np.arange(12, 30), np.arange(12, 30)] = True
    _stamp(c, b, 460, 200, "diagonal arm")
    b2 = np.zeros((30, 30), bool)
    b2[18:, 18:] = True
    b2[np.arange(0, 18), np.arange(0, 18)] = True
    _stamp(c, b2, 520, 200, "diagonal arm")
    tie = np.zeros((21, 25), bool)
    for y in range(21):
        w = abs(y - 10) + 1
        tie[y, :w] = tie[y, 25 - w:] = True
    _stamp(c, tie, 580, 200, "pinch")
    arm = np.zeros((26, 26), bool)
    arm[10:26, 10:26] = True
    arm = _outline(arm, 3)
    arm[np.arange(0, 10), np.arange(0, 10)] = True
    arm[np.arange(0, 10), 25 - np.arange(0, 10)] = True
    _stamp(c, arm, 640, 200, "diagonal arm")
    # shapes symmetric about their centroid: the nearest-point sort has ties
    for i, (w, h) in enumerate(((12, 12), (13, 13), (12, 8), (9, 15), (16, 5))):
        _stamp(c, np.ones((h, w), bool), 40 + 40 * i, 330, "symmetric")
    plus = np.zeros((21, 21), bool)
    plus[8:13, :] = plus[:, 8:13] = True
    _stamp(c, plus, 260, 330, "symmetric")
    m, x0, y0 = _poly([(320, 330), (332, 342), (320, 354), (308, 342)], pad=1)  # diamond
    _stamp(c, m, x0, y0, "symmetric")
    m, x0, y0 = _poly([(370, 330), (384, 337), (370, 344), (356, 337)], pad=1)
    _stamp(c, m, x0, y0, "symmetric")
    # triangles, pentagons, discs
    for i, deg in enumerate((0, 17, 40, 90, 133, 200)):
        pts = [(430 + 70 * i % 490 + 12 * math.cos(math.radians(deg + 120 * k)), 440 + 12 * math.sin(math.radians(deg + 120 * k))) for k in range(3)]
        m, x0, y0 = _poly(pts)
        _stamp(c, _outline(m, 3), x0, y0, "triangle")
    for i, r in enumerate((10, 14)):
        pts = [(60 + 50 * i + r * math.cos(2 * math.pi * k / 5 + 0.3), 440 + r * math.sin(2 * math.pi * k / 5 + 0.3)) for k in range(5)]
        m, x0, y0 = _poly(pts)
        _stamp(c, _outline(m, 3), x0, y0, "pentagon")
    for i, r in enumerate((4.5, 6, 9, 13)):
        yy, xx = np.mgrid[-15:16, -15:16]
        _stamp(c, _outline(np.hypot(xx, yy) <= r, 3), 170 + 40 * i, 425, "disc")
    # tiny triangles: the loop runs out of points (isFailed) with few points left
    for i in range(4):
        t = np.tril(np.ones((8 + i, 8 + i), bool))
        _stamp(c, t, 700 + 30 * i, 330, "small triangle")
    return c


def _frame_rotations():
    c = _canvas()
    x = 40
    for deg in (0, 1, 44.9, 45, 89):
        for j, (w, h) in enumerate(((30, 18), (44, 24), (22, 22))):
            m, x0, y0 = _poly(_rect_pts(x, 60 + 80 * j, w, h, deg))
            _stamp(c, _outline(m, 3), x0, y0, "rect %g" % deg)
            m, x0, y0 = _poly(_rect_pts(x + 0.5, 300 + 70 * j, w * 0.5, h * 0.5, deg))  # small solid ones, half-pixel centre
            _stamp(c, m, x0, y0, "rect %g" % deg)
        x += 80
    # bars wider than 128 half-res px, across mask words and labelling tiles
    for j, (w, h, deg) in enumerate(((200, 4, 0), (300, 5, 0), (150, 3, 0), (180, 4, 1), (240, 4, 12))):
        m, x0, y0 = _poly(_rect_pts(620, 60 + 50 * j, w, h, deg))
        _stamp(c, m, x0, y0, "bar")
    return c


def _frame_seams_and_edges():
    c = _canvas()
    # boxes whose half-res x_min is 0, 31, 32, 319, 320 (mask words / labelling tiles); x = 0 lies in the background band
    for i, x in enumerate((0, 31, 32, 319, 320)):
        box = np.zeros((16, 14), bool)
        box[:3, :] = box[-3:, :] = box[:, :3] = box[:, -3:] = True
        _stamp(c, box, x, 40 + 40 * i, "seam x=%d" % x)
        _stamp(c, np.ones((6, 12), bool), x, 250 + 30 * i, "seam x=%d" % x)
    # components across each frame edge and each frame corner
    edge = np.zeros((30, 30), bool)
    edge[:, :] = True
    edge = _outline(edge, 3)
    for tag, x, y in (("edge top", 400, -10), ("edge bottom", 400, HR - 20), ("edge left", -12, 150), ("edge right", HC - 18, 150),
                      ("corner top-left", -10, -10), ("corner top-right", HC - 20, -10), ("corner bottom-left", -10, HR - 20),
                      ("corner bottom-right", HC - 20, HR - 20), ("edge top", 600, -2), ("edge left", -2, 420), ("edge right", HC - 28, 420),
                      ("edge bottom", 600, HR - 28)):
        _stamp(c, edge, x, y, tag)
    return c


def _frame_area_limits():
    """Components of 29 and 30 pixels and of AREA_LIMIT and AREA_LIMIT + 1 (outlines of t = 4 whose sides sum to 656)."""
    c = _canvas()
    _stamp(c, np.ones((2, 15), bool), 40, 20, "area 30")           # a candidate
    b = np.ones((2, 15), bool)
    b[1, 14] = False
    _stamp(c, b, 80, 20, "area 29")                                # not a candidate
    _stamp(c, np.ones((5, 6), bool), 120, 20, "area 30")
    t = np.ones((5, 6), bool)
    t[4, 5] = False
    _stamp(c, t, 140, 20, "area 29")
    w, h, th = 400, 256, 4
    ring = np.zeros((h, w), bool)
    ring[:th, :] = ring[-th:, :] = ring[:, :th] = ring[:, -th:] = True
    assert ring.sum() == AREA_LIMIT
    _stamp(c, ring, 20, 60, "area limit")                         # exactly the limit: a candidate
    ring2 = np.zeros((h, w + 1), bool)
    ring2[:, :w] = ring
    ring2[100, w] = True                                # one pixel more: not a candidate
    _stamp(c, ring2, 470, 60, "area limit + 1")                   # not a candidate
    return c


def _frame_pinch_field(seed):
    """Rows of small shapes with one-pixel necks and diagonal steps, the walk's early stops, at many offsets."""
    c = _canvas()
    rng = np.random.RandomState(7 + seed)
    for k in range(120):
        x, y = 20 + (k % 15) * 60, 20 + (k // 15) * 62
        m = np.zeros((24, 24), bool)
        a, b = rng.randint(6, 11, 2)
        m[:a, :b] = True
        m[24 - a:, 24 - b:] = True
        n = rng.randint(0, 3)
        m[np.arange(a - 1, 24 - a + 1), np.linspace(b - 1, 24 - b, 24 - 2 * a + 2).round().astype(int)] = True
        if n == 1:
            m[:a, 24 - b:] = True
        elif n == 2:
            m = m | m[:, ::-1]
        if rng.rand() < 0.5:
            m = _outline(m, 2) | m & (rng.rand(24, 24) < 0.1)
        _stamp(c, np.rot90(m, k % 4), x, y, "pinch field")
    return c


FRAMES = ["letters", "rotations", "seams_and_edges", "area_limits"] + ["pinch_field_%d" % k for k in range(10)]


ABSENT = ("area 29", "area limit + 1")  # tags whose shapes must not become candidates


def shape_frames():
    """[(name, 1080 x 1920 uint8 frame)] in a fixed order."""
    return [(name, frame) for name, frame, _ in shape_frames_tagged()]


def shape_frames_tagged():
    """[(name, frame, [(topology, x0, y0, x1, y1) half-res box of each shape drawn for it])] in a fixed order."""
    makers = {"letters": _frame_letters, "rotations": _frame_rotations, "seams_and_edges": _frame_seams_and_edges,
              "area_limits": _frame_area_limits}
    makers.update({"pinch_field_%d" % k: (lambda k=k: _frame_pinch_field(k)) for k in range(10)})
    out = []
    for name in FRAMES:
        del _TAGS[:]
        out.append((name, _to_frame(makers[name]()), list(_TAGS)))
    return out


def uhd_frame(frames):
    """Four 1080p shape frames tiled into one 3840 x 2160 frame."""
    out = np.empty((2 * ROWS, 2 * COLS), np.uint8)
    for i in range(4):
        out[(i // 2) * ROWS:(i // 2 + 1) * ROWS, (i % 2) * COLS:(i % 2 + 1) * COLS] = frames[i % len(frames)]
    return out
