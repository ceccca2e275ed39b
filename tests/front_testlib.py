"""An independent statement of the front of the chain, from a frame's bytes to the labelled half image and the candidate list:
a0 `cvtColor(BGR2GRAY)` (main.cpp:36,54), a1 `resize` to half size (CylinderTag.cpp:79) with `convertTo(CV_32F, 1/255)` (:80),
a2 `adaptiveThreshold` (corner_detector.cpp:28-79), a3 `connectedComponentsWithStats` and the area filter (:81-106).

Plain numpy / scipy, written from those lines and SURVEY App. A.1-A.4 / B1.  It imports nothing from `oracle/`, from
`cylindertag_amd/csrc` or from the testkit, and shares no table with them.  Everything here is integer- or bit-exact: whoever
compares with it compares for equality.  A `Trace` records what the coverage conditions of `tests/front_shapes.py` ask about."""
import math

import numpy as np
from scipy import ndimage as ndi

f32 = np.float32


class Trace:
    """What one `front()` call met."""

    def __init__(self):
        self.tiles = np.zeros((0, 5), np.int64)  # per interior threshold tile: tile row, tile column, mn, mx, bound (pixel u is foreground iff u < bound)
        self.vertical_ties = 0       # body pixels whose float vertical sum lies exactly on .5
        self.saturated_low = 0       # pixels the resize clips at 0 / at 255
        self.saturated_high = 0
        self.tail_columns_differing = 0   # tail columns that hold a pixel where body and tail rounding differ
        self.tail_pixels_differing = 0
        self.raster_first_outside_first_block = 0  # components whose first pixel in raster order is not in their first 2x2 block in block-raster order
        self.components = 0


# ------------------------------------------------------------------------------------------- a0
def bgr2gray(bgr):
    """OpenCV's 8-bit BGR2GRAY: 14-bit fixed point, B 1868, G 9617, R 4899 (they sum to 2^14), rounded."""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


# ------------------------------------------------------------------------------------------- a1
def _cubic_weights(x):
    """The four cubic weights (A = -0.75) of a float fractional position, evaluated in float as interpolateCubic does."""
    A, one = f32(-0.75), f32(1)
    x = x.astype(np.float32)
    c0 = ((A * (x + one) - f32(5) * A) * (x + one) + f32(8) * A) * (x + one) - f32(4) * A
    c1 = ((A + f32(2)) * x - (A + f32(3))) * x * x + one
    c2 = ((A + f32(2)) * (one - x) - (A + f32(3))) * (one - x) * (one - x) + one
    c3 = one - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], 1)


def resize_taps(n_src, n_dst):
    """Per output index: the source index of tap 1 (`floor(fx)`) and the four `short` weights (x 2048, cvRound: half to even)."""
    scale = n_src / n_dst                                      # double
    d = np.arange(n_dst, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)          # rounded to float
    sx = np.floor(fx).astype(np.int64)
    frac = fx - sx.astype(np.float32)
    w = np.clip(np.rint(_cubic_weights(frac) * f32(2048)), -32768, 32767).astype(np.int64)
    return sx, w


def resize_half(gray, simd_lanes=8, trace=None):
    """`resize(img, Size(cols / 2, rows / 2), INTER_CUBIC)` of an 8-bit image of any size >= 4 x 4 (A.1): integer horizontal pass; the
    vector body of the vertical pass (columns below `dcols & ~(simd_lanes - 1)`) in float, summed from tap 3 down to tap 0 and rounded
    half to even; the row tail in fixed point, `(v + 2^21) >> 22`; both saturated."""
    h, w = gray.shape
    dh, dw = h // 2, w // 2
    sx, a = resize_taps(w, dw)
    sy, b = resize_taps(h, dh)
    src = gray.astype(np.int64)
    H = np.zeros((h, dw), np.int64)
    for j in range(4):
        H += src[:, np.clip(sx - 1 + j, 0, w - 1)] * a[:, j][None, :]
    S = [H[np.clip(sy - 1 + k, 0, h - 1)] for k in range(4)]
    scale = f32(1) / f32(2048.0 * 2048.0)
    bf = [(b[:, k].astype(np.float32) * scale)[:, None] for k in range(4)]
    t = S[3].astype(np.float32) * bf[3]
    t = S[2].astype(np.float32) * bf[2] + t
    t = S[1].astype(np.float32) * bf[1] + t
    t = S[0].astype(np.float32) * bf[0] + t
    body_raw = np.rint(t).astype(np.int64)
    v = S[0] * b[:, 0][:, None] + S[1] * b[:, 1][:, None] + S[2] * b[:, 2][:, None] + S[3] * b[:, 3][:, None]
    tail_raw = (v + (1 << 21)) >> 22
    e = dw & ~(simd_lanes - 1)
    raw = body_raw.copy()
    raw[:, e:] = tail_raw[:, e:]
    if trace is not None:
        trace.vertical_ties += int((np.abs(t[:, :e] - np.floor(t[:, :e])) == f32(0.5)).sum())
        trace.saturated_low += int((raw < 0).sum())
        trace.saturated_high += int((raw > 255).sum())
        differ = np.clip(body_raw[:, e:], 0, 255) != np.clip(tail_raw[:, e:], 0, 255)
        trace.tail_columns_differing += int(differ.any(0).sum())
        trace.tail_pixels_differing += int(differ.sum())
    return np.clip(raw, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------- a2
def to_float(half):
    """`convertTo(CV_32F, 1.0 / 255)` (A.2): float(u) * float(1 / 255), one rounding."""
    return half.astype(np.float32) * f32(1.0 / 255)


def threshold_of_extrema(mn, mx, dark_cap=0.3):
    """:71 for a tile whose 3 x 3 neighbourhood has the 8-bit extrema mn, mx: the float threshold `min(cap, (max + min) / 2)`."""
    k = f32(1.0 / 255)
    s = (np.asarray(mx, np.float32) * k + np.asarray(mn, np.float32) * k) / f32(2)
    return np.minimum(f32(dark_cap), s)


def bound_of_extrema(mn, mx, dark_cap=0.3):
    """The same as an integer: the number of 8-bit values u whose float is below the threshold, so u is foreground iff u < bound."""
    thr = np.asarray(threshold_of_extrema(mn, mx, dark_cap), np.float32)
    u = to_float(np.arange(256, dtype=np.uint8))
    return (u[(None,) * thr.ndim] < thr[..., None]).sum(-1)


def adaptive_threshold(half, tw, dark_cap=0.3, trace=None):
    """corner_detector.cpp:28-79 on the float half image.  Tiles of tw x tw with ragged last ones (:44); the extrema of every tile;
    for the interior tiles only the minimum of the minima and the maximum of the maxima over 3 x 3 tiles (:54-67), zero elsewhere
    (B1); a pixel is 255 iff `f < min(cap, (max + min) / 2)` of its tile (:71).  Fewer than 3 tiles in a direction leave no
    interior tile: all background."""
    h, w = half.shape
    f = to_float(half)
    tr, tc = -(-h // tw), -(-w // tw)
    pad = np.full((tr * tw, tc * tw), np.nan, np.float32)
    pad[:h, :w] = f
    blk = pad.reshape(tr, tw, tc, tw)
    mn, mx = np.nanmin(blk, (1, 3)), np.nanmax(blk, (1, 3))
    thr = np.zeros((tr, tc), np.float32)
    if tr >= 3 and tc >= 3:
        mnf = ndi.minimum_filter(mn, 3)[1:-1, 1:-1]
        mxf = ndi.maximum_filter(mx, 3)[1:-1, 1:-1]
        thr[1:-1, 1:-1] = np.minimum(f32(dark_cap), (mxf + mnf) / f32(2))
        if trace is not None:
            # the extrema are floats of 8-bit values: u -> float(u) * k is strictly increasing, so the 8-bit extrema are those of the bytes
            padu = np.full((tr * tw, tc * tw), -1, np.int64)
            padu[:h, :w] = half
            bu = padu.reshape(tr, tw, tc, tw)
            mxu = bu.max((1, 3))
            bu = np.where(bu < 0, 256, bu)
            mnu = bu.min((1, 3))
            a = ndi.minimum_filter(mnu, 3)[1:-1, 1:-1]
            b = ndi.maximum_filter(mxu, 3)[1:-1, 1:-1]
            u = to_float(np.arange(256, dtype=np.uint8))
            bound = np.searchsorted(u, thr[1:-1, 1:-1].ravel(), "left")  # number of u with float(u) < thr
            ti, tj = np.mgrid[1:tr - 1, 1:tc - 1]
            trace.tiles = np.stack([ti.ravel(), tj.ravel(), a.ravel(), b.ravel(), bound], 1).astype(np.int64)
    T = np.repeat(np.repeat(thr, tw, 0), tw, 1)[:h, :w]
    return np.where(f < T, 255, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------- a3
def label(binary, trace=None, connectivity=8):
    """`connectedComponentsWithStats(src, 8, CV_32S, CCL_BBDT)` (A.4): the 8-connected partition, numbered by ascending key
    `min over the component's pixels of (y // 2) * ceil(W / 2) + x // 2`: the block-raster index of its first 2 x 2 block.  (The pixels
    of one block are 8-connected to each other, so no two components share a key.)
    Returns (labels int32, areas [n + 1] with the background first, boxes [n + 1, 4] as x_min, y_min, x_max, y_max)."""
    structure = np.ones((3, 3)) if connectivity == 8 else None
    lab, n = ndi.label(binary > 0, structure=structure)
    rows, cols = binary.shape
    if n == 0:
        return np.zeros((rows, cols), np.int32), np.array([binary.size], np.int64), np.array([[0, 0, cols - 1, rows - 1]], np.int64)
    bcols = (cols + 1) // 2
    ys, xs = np.nonzero(lab)
    ids = lab[ys, xs]
    key = (ys // 2) * bcols + xs // 2
    first = np.full(n + 1, np.iinfo(np.int64).max)
    np.minimum.at(first, ids, key)
    assert len(np.unique(first[1:])) == n
    order = np.argsort(first[1:], kind="stable")
    remap = np.zeros(n + 1, np.int32)
    remap[order + 1] = np.arange(1, n + 1)
    out = remap[lab]
    ids = remap[ids]
    areas = np.bincount(out.ravel(), minlength=n + 1).astype(np.int64)
    boxes = np.zeros((n + 1, 4), np.int64)
    boxes[:, 0], boxes[:, 1] = cols, rows
    np.minimum.at(boxes[:, 0], ids, xs)
    np.minimum.at(boxes[:, 1], ids, ys)
    np.maximum.at(boxes[:, 2], ids, xs)
    np.maximum.at(boxes[:, 3], ids, ys)
    boxes[0] = (0, 0, cols - 1, rows - 1)
    if trace is not None:
        trace.components += n
        raster_first = np.full(n + 1, np.iinfo(np.int64).max)
        np.minimum.at(raster_first, ids, ys * cols + xs)
        ry, rx = raster_first[1:] // cols, raster_first[1:] % cols
        trace.raster_first_outside_first_block += int(((ry // 2) * bcols + rx // 2 != np.sort(first[1:])).sum())
    return out, areas, boxes


def area_limit(rows, cols, area_max_fraction=0.01):
    """`round(0.01 * src.cols * src.rows)` (:88): a double product, rounded half away from zero."""
    return math.floor(area_max_fraction * cols * rows + 0.5)


def candidates(labels, areas=None, boxes=None, area_min=30, area_max_fraction=0.01):
    """:86-106: the components that are neither below `area_min` nor above the limit, in label order.
    Returns int64 [n, 6]: label, area, x_min, y_min, x_max, y_max."""
    rows, cols = labels.shape
    if areas is None:
        _, areas, boxes = label(labels > 0)
    limit = area_limit(rows, cols, area_max_fraction)
    keep = [i for i in range(1, len(areas)) if not (areas[i] < area_min or areas[i] > limit)]
    return np.array([[i, areas[i], *boxes[i]] for i in keep], np.int64).reshape(-1, 6)


# ------------------------------------------------------------------------------------------- the chain
def front(frame, tw=5, dark_cap=0.3, area_min=30, area_max_fraction=0.01, simd_lanes=8, trace=None):
    """A gray (rows, cols) or BGR (rows, cols, 3) frame -> dict(gray, half, binary, labels, areas, boxes, candidates, trace)."""
    trace = trace if trace is not None else Trace()
    gray = bgr2gray(frame) if frame.ndim == 3 else frame
    half = resize_half(gray, simd_lanes, trace)
    binary = adaptive_threshold(half, tw, dark_cap, trace)
    labels, areas, boxes = label(binary, trace)
    cand = candidates(labels, areas, boxes, area_min, area_max_fraction)
    return dict(gray=gray, half=half, binary=binary, labels=labels, areas=areas, boxes=boxes, candidates=cand, trace=trace)


def same_partition(labels, other):
    """Whether two label images (0 = background in `labels`, any non-zero numbering in `other`) describe the same components."""
    if ((labels != 0) != (other != 0)).any():
        return False
    a, b = labels.ravel().astype(np.int64), other.ravel().astype(np.int64) & 0xffffffff
    pairs = np.unique((a << 32) | b)  # every (label, other label) that shares a pixel: a bijection iff the partitions are equal
    return len(np.unique(pairs >> 32)) == len(pairs) == len(np.unique(pairs & 0xffffffff))
