"""Deterministic frames for the edges of stages a0-a3 (BGR2GRAY, resize, adaptiveThreshold, labelling and the area filter), drawn in
Python from fixed seeds.  Each frame carries tags that say what it is for; `tests/test_front_stages_cpu.py` asserts from the trace of
`tests/front_testlib.py` that each tag is reached.

Most frames are drawn as a half-size design and doubled: a 2 x 2 block of equal pixels decimates to its value wherever its
neighbours are equal too, and a step between two values rings by 3/32 of the step on the pixel at either side (the cubic taps
[-3, 19, 19, -3] / 32), nowhere else.  Dark ink (20) on bright ground (200) in lines of one or two half-size pixels therefore
gives exactly the drawn mask wherever a frame is not hollowed out by the threshold (regions wider than three tiles).

Every frame here is checked up to the candidate list (half image, mask, label image, areas, candidates), which no limit of the
chain touches; what the stages behind a3 make of these frames is not asserted.  No frame fills a batch workspace's component pool
except those tagged "dense" and the noise frames of `resize_frames`, which go alone."""
import math

import numpy as np

import front_testlib as ft

ROWS, COLS = 1080, 1920
INK, GROUND = 20, 200
TILE_W, TILE_H = 320, 30          # the labelling tiles of the device, in half-size pixels
CAPS = (0.3, 0.2, 0.45, 0.12)     # dark_cap: the reference's and the three of test_non_default_params
AREA_PARAMS = ((30, 0.01), (60, 0.002), (12, 0.03))  # (area_min, area_max_fraction): the reference's and those of test_non_default_params
WINDOWS = (1, 2, 3, 4, 6, 7, 8, 16, 31, 32)


def double(design):
    return np.ascontiguousarray(np.kron(design, np.ones((2, 2), np.uint8)))


# ------------------------------------------------------------------------------------------- threshold knife edges
def pair_table(dark_cap):
    """Every (mn, mx), mn <= mx, with mn + mx below twice the cap's own bound (154 for 0.3: 6006 pairs): the pairs whose mean term can
    decide.  The cap's bound comes from the statement alone."""
    dim = 2 * int(ft.bound_of_extrema(255, 255, dark_cap))
    return [(mn, mx) for mn in range(dim) for mx in range(mn, dim) if mn + mx < dim]


def _decimated_corner(p, base):
    """The half-size value at the corner of a doubled patch of value p on ground `base` (both directions ring), None on a rounding tie:
    v = -192 * 2048 * base + 2240 * (2240 p - 192 base), over 2^22."""
    v = 1225 * p - 201 * base  # v / 2^12
    if v % 1024 == 512:
        return None
    return min(255, max(0, (v + 512) >> 10))


def _patch_for(target, around, lo, hi, sign):
    """(base, p): a tile ground `base` in [lo, hi] within 3 of `around` and a patch value p (below it for sign -1, above for +1) whose
    decimated corner is exactly `target`."""
    for off in (0, -1, 1, -2, 2, -3, 3):
        base = around + off
        if not lo <= base <= hi:
            continue
        if base == target:
            return base, base
        guess = (target * 1024 + 201 * base) / 1225.0
        for p in (int(round(guess)), int(math.floor(guess)), int(math.ceil(guess))):
            if 0 <= p <= 255 and (p - base) * sign > 0 and _decimated_corner(p, base) == target:
                return base, p
    return None


CELL = 20  # half-size pixels: three threshold tiles of 5 and a guard tile


def knife_frames(dark_cap=0.3, extra=()):
    """1080p frames of cells, one (mn, mx) pair each (window 5).  A cell is 3 x 3 threshold tiles on the tile grid and a guard tile to
    the right and below.  Its centre tile holds rows at the pair's bound and rows one below it; tile (0, 0) holds a dark patch whose
    decimated corner is mn and tile (2, 2) a bright one whose corner is mx; everything else, the guard included, sits at the bound
    (or within 3 of it, so that the patch lands on its value), which lies between the two.  The centre tile's 3 x 3 neighbourhood is
    its own cell, so the tile sees (mn, mx) and has pixels on both sides of its bound.
    `extra`: (mn, mx, bright) cells beyond the pair table; `bright` makes the centre tile hold no pixel below the bound."""
    cells = [(a, b, False) for a, b in pair_table(dark_cap)] + list(extra)
    per_row, per_col = (COLS // 2 // 5 - 2) // 4, (ROWS // 2 // 5 - 2) // 4
    frames = []
    for k0 in range(0, len(cells), per_row * per_col):
        chunk = cells[k0:k0 + per_row * per_col]
        first_bound = int(ft.bound_of_extrema(chunk[0][0], chunk[0][1], dark_cap))
        D = np.full((ROWS // 2, COLS // 2), max(first_bound, 1), np.uint8)
        for k, (mn, mx, bright) in enumerate(chunk):
            T = int(ft.bound_of_extrema(mn, mx, dark_cap))
            T = min(max(T, mn), mx)
            cy, cx = divmod(k, per_row)
            y0, x0 = 5 + CELL * cy, 5 + CELL * cx
            D[max(y0 - 2, 0):y0 + 18, max(x0 - 2, 0):x0 + 18] = T
            lo = _patch_for(mn, T, mn, mx, -1)
            hi = _patch_for(mx, T, mn, mx, +1)
            if lo is not None:
                D[y0:y0 + 5, x0:x0 + 5] = lo[0]
                D[y0 + 1:y0 + 4, x0 + 1:x0 + 4] = lo[1]
            if hi is not None:
                D[y0 + 10:y0 + 15, x0 + 10:x0 + 15] = hi[0]
                D[y0 + 11:y0 + 14, x0 + 11:x0 + 14] = hi[1]
            if bright:
                D[y0 + 7:y0 + 10, x0 + 5:x0 + 10] = min(T + 1, mx)
            elif T - 1 >= mn:
                D[y0 + 7:y0 + 10, x0 + 5:x0 + 10] = T - 1
        frames.append(double(D))
    return frames


def cap_edge_cells(dark_cap):
    """Cells around the cap: mn + mx at thr_dim - 1, thr_dim, thr_dim + 1 (153 / 154 / 155 for 0.3), and tiles without a pixel below
    the cap's bound beside dark neighbours."""
    cap_bound = int(ft.bound_of_extrema(255, 255, dark_cap))
    dim = 2 * cap_bound
    out = []
    for s in (dim - 1, dim, dim + 1):
        for mn in range(0, cap_bound, 3):
            out.append((mn, s - mn, False))
    for mn in range(0, cap_bound, 5):
        for mx in (cap_bound + 3, cap_bound + 40, 250):
            out.append((mn, mx, True))
    return out


# ------------------------------------------------------------------------------------------- textures
def blob_texture(rows, cols, seed, scale=6.0, level=0.35):
    """Smooth dark blobs on bright ground with sensor noise: a few hundred components of all sizes."""
    from scipy import ndimage as ndi
    rng = np.random.RandomState(seed)
    field = ndi.gaussian_filter(rng.rand(rows, cols), scale)
    cut = np.quantile(field, level)
    img = np.where(field < cut, 30.0, 190.0) + rng.normal(0, 6, (rows, cols))
    return np.clip(ndi.gaussian_filter(img, 0.8), 0, 255).astype(np.uint8)


def window_frames():
    """(name, frame, window): every other window on a frame whose half size is no multiple of it, and frames with exactly 2, 3 and 4
    tiles in a direction (fewer than 3: all background)."""
    out = []
    for i, tw in enumerate(WINDOWS):
        hr, hc = 7 * max(tw, 9) + tw // 2 + 1, 11 * max(tw, 9) + (tw + 1) // 2
        hr, hc = hr + (hr % tw == 0), hc + (hc % tw == 0)
        out.append(("window %d ragged %dx%d" % (tw, 2 * hc, 2 * hr), blob_texture(2 * hr, 2 * hc, 100 + i, 3.0), tw))
    for tw in (1, 2, 3, 5, 7, 32):
        for tiles in (2, 3, 4):
            n = tiles * tw - (tw // 2 if tw > 1 else 0)  # exactly `tiles` tiles, the last one ragged
            if 2 * n < 4:
                continue
            wide = 12 * max(tw, 4) + 1
            out.append(("window %d, %d tile rows" % (tw, tiles), blob_texture(2 * n, 2 * wide, 200 + tw * 8 + tiles, 1.5), tw))
            out.append(("window %d, %d tile columns" % (tw, tiles), blob_texture(2 * wide, 2 * n + 1, 300 + tw * 8 + tiles, 1.5), tw))
    return out


# ------------------------------------------------------------------------------------------- resize
def noise(rows, cols, seed):
    return np.random.RandomState(seed).randint(0, 256, (rows, cols)).astype(np.uint8)


def black_white(rows, cols, seed):
    return np.random.RandomState(seed).choice([0, 255], (rows, cols)).astype(np.uint8)


def tie_columns(rows, cols):
    """Columns alternating 16 / 17: at an exact 2x every pixel of the vector body lies on a rounding tie."""
    img = np.zeros((rows, cols), np.uint8)
    img[:, 0::2], img[:, 1::2] = 16, 17
    return img


ODD_SIZES = ((4, 4), (5, 7), (9, 9), (75, 97), (74, 97), (75, 96), (545, 851), (1079, 1919), (1081, 1920), (1080, 1921))


def resize_frames():
    """(name, frame, tags)"""
    out = []
    for k, (r, c) in enumerate(ODD_SIZES):
        out.append(("noise %dx%d" % (c, r), noise(r, c, 400 + k), ("odd",) if (r | c) & 1 else ()))
        out.append(("black and white %dx%d" % (c, r), black_white(r, c, 500 + k), ("saturation",) if r * c >= 64 else ()))
    out.append(("black and white 1920x1080", black_white(ROWS, COLS, 520), ("saturation",)))
    out.append(("ties 1706x64", tie_columns(64, 2 * 853), ("vertical_ties", "tail_differs")))        # hcols = 853: 5 tail columns
    out.append(("ties 1707x65", tie_columns(65, 1707), ("odd",)))
    out.append(("ties 1080p crop 1900", tie_columns(200, 1900), ("vertical_ties", "tail_differs")))  # hcols = 950: 6 tail columns
    return out


LANE16_WIDTHS = (2 * 488, 2 * 953 + 1, 2 * 604, 1114)  # hcols % 16 >= 8: eight columns change hands between the two lane variants


# ------------------------------------------------------------------------------------------- labelling
def _snake(D, y0, x0, area, width):
    """A serpentine of one-pixel lines, exactly `area` pixels: runs of `width` on every other row, joined at alternating ends."""
    left, y, right_side = area, y0, True
    while left > 0:
        n = min(width, left)
        if right_side:
            D[y, x0:x0 + n] = INK
        else:
            D[y, x0 + width - n:x0 + width] = INK
        left -= n
        if left > 0:  # the joint, under the end the run stopped at
            D[y + 1, x0 + width - 1 if right_side else x0] = INK
            left -= 1
        y += 2
        right_side = not right_side
    return y


def _spiral(D, y0, x0, size):
    """A square spiral of one-pixel lines, two pixels apart."""
    y, x, dy, dx, n = y0, x0, 0, 1, size
    D[y, x] = INK
    while n > 0:
        for _ in range(3 if n == size else 2):
            for _ in range(n):
                y, x = y + dy, x + dx
                D[y, x] = INK
            dy, dx = dx, -dy  # right, down, left, up
        n -= 2


def labelling_design(seed=0):
    """The half-size design (540 x 960) of the labelling frame: spirals, combs, nested rings, diagonal chains through the corners of the
    320 x 30 label tiles, components that begin on an odd row left of a component beginning on the even row above, and a field of
    one-pixel-apart dots."""
    rng = np.random.RandomState(700 + seed)
    D = np.full((ROWS // 2, COLS // 2), GROUND, np.uint8)
    for k in range(6):  # spirals across the tile seams
        _spiral(D, 12 + 3 * k, 20 + 150 * k + 7 * seed, 61 + 8 * (k % 3))
    for k in range(8):  # combs: a spine with teeth down (many unions along the spine) and up
        y, x = 120 + (k % 2) * 47, 30 + 115 * k
        D[y, x:x + 90] = INK
        for t in range(0, 90, 2):
            if k % 2:
                D[y - 20 - (t % 7):y, x + t] = INK
            D[y:y + 25 + (t % 5), x + t] = INK
    for k in range(7):  # nested rings, two pixels apart, not touching
        cy, cx = 250, 60 + 130 * k
        for r in range(3, 40, 2 + (k % 2)):
            D[cy - r, cx - r:cx + r + 1] = D[cy + r, cx - r:cx + r + 1] = INK
            D[cy - r:cy + r + 1, cx - r] = D[cy - r:cy + r + 1, cx + r] = INK
            D[cy - r, cx] = GROUND  # each ring opened at the top: a C, so that the rings stay single components with long equivalence chains
    for k in range(30):  # diagonal one-pixel chains through tile corners (x = 320, 640; y = 30 k): 8-connected only
        cx, cy = (320, 640)[k % 2], 30 * (10 + k % 7)
        for t in range(-17, 18):
            yy, xx = cy + t, cx + (t if k % 3 else -t) + (k // 14)
            D[yy, xx] = INK
    y = 330
    for k in range(40):  # B on an even row, A on the odd row below it and to its left, in the same block row: A's block comes first
        x = 15 + 23 * k
        yy = y + 2 * (k % 5) * 6
        D[yy + 1, x:x + 1] = INK                     # A: begins on the odd row
        D[yy + 1:yy + 8, x] = INK
        D[yy, x + 6:x + 12] = INK                    # B: begins on the even row above, further right: first in raster order
        # a component whose own first raster pixel is right of its first block: a hook that starts high on the right and reaches left one row lower
        D[yy + 20, x + 8:x + 14] = INK
        D[yy + 21, x + 2:x + 9] = INK
    yy, xx = np.mgrid[440:520, 40:900]
    D[440:520, 40:900][((yy + xx) % 2 == 0) & (rng.rand(80, 860) < 0.9)] = INK  # a thinned checkerboard: large diagonal-only components
    return D


def area_design(hrows, hcols, area_min=30, area_max_fraction=0.01):
    """Serpentines of exactly area_min - 1, area_min, limit and limit + 1 pixels (and a few around them)."""
    D = np.full((hrows, hcols), GROUND, np.uint8)
    limit = ft.area_limit(hrows, hcols, area_max_fraction)
    x = 8
    wanted = [area_min - 1, area_min, area_min + 1, limit - 1, limit, limit + 1, limit + 2]
    for a in wanted:
        width = max(6, min(hcols // 9, int(math.sqrt(2 * a)) + 2))
        end = _snake(D, 8, x, a, width)
        assert end < hrows - 6 and x + width < hcols - 6, (hrows, hcols, a)
        x += width + 3
    return D, wanted


AREA_SIZES = ((540, 960), (101, 250), (135, 482))  # 0.01 * 250 * 101 = 252.5: the limit rounds half away from zero, to 253


def checkerboard(rows=400, cols=640):
    D = np.full((rows // 2, cols // 2), GROUND, np.uint8)
    yy, xx = np.mgrid[0:rows // 2, 0:cols // 2]
    D[(yy + xx) % 2 == 0] = INK
    return double(D)


def dark_noise(rows=ROWS, cols=COLS, seed=3):
    """Dark sensor noise: with window 1 well over 1500 components at 1080p."""
    return np.clip(np.random.RandomState(seed).normal(40, 25, (rows, cols)), 0, 255).astype(np.uint8)


def labelling_frames():
    """(name, frame, window, (area_min, area_max_fraction), tags)"""
    out = [("labelling shapes %d" % s, double(labelling_design(s)), 5, AREA_PARAMS[0], ("first_block", "chains")) for s in range(2)]
    for hr, hc in AREA_SIZES:
        for amin, frac in AREA_PARAMS:
            if ft.area_limit(hr, hc, frac) + 2 > hr * hc // 5 or ft.area_limit(hr, hc, frac) <= amin + 1:
                continue
            D, wanted = area_design(hr, hc, amin, frac)
            out.append(("areas %dx%d min %d fraction %g" % (hc, hr, amin, frac), double(D), 5, (amin, frac), ("areas",)))
    out.append(("checkerboard", checkerboard(), 5, AREA_PARAMS[0], ("checkerboard",)))
    out.append(("dark noise window 1", dark_noise(), 1, AREA_PARAMS[0], ("many_components", "dense")))
    return out


# ------------------------------------------------------------------------------------------- slot reuse
def slot_reuse_batches(slots=8):
    """Batches of `slots` frames that land on the same workspace slots call after call: textured, nearly empty, textured again shifted by
    one label tile and by odd amounts, empty, ... so that labels left behind a tile the next frame skips would show."""
    textured = double(labelling_design(5))
    empty = np.full((ROWS, COLS), GROUND, np.uint8)
    empty[500:520, 900:960] = INK
    shifts = [(0, 0), (60, 640), (2, 2), (34, 326)]
    batches = []
    for b, (dy, dx) in enumerate(shifts):
        tex = np.roll(np.roll(textured, dy, 0), dx, 1)
        tex[:12], tex[-12:], tex[:, :12], tex[:, -12:] = GROUND, GROUND, GROUND, GROUND
        batches.append(np.stack([tex if (s + b) % 2 == 0 else empty for s in range(slots)]))
        batches.append(np.stack([empty if (s + b) % 2 == 0 else tex for s in range(slots)]))
    return batches


# ------------------------------------------------------------------------------------------- BGR
def colourise(gray, seed):
    """A BGR frame with unequal channels around a gray scene."""
    rng = np.random.RandomState(seed)
    h, w = gray.shape
    yy, xx = np.mgrid[0:h, 0:w]
    g16 = gray.astype(np.int32)
    b = np.clip(g16 + 25 * np.sin(xx / 97.0) + rng.randint(-6, 7, gray.shape), 0, 255)
    g = np.clip(g16 - 10 * np.cos(yy / 61.0) + rng.randint(-3, 4, gray.shape), 0, 255)
    r = np.clip(g16 + 18 * np.sin((xx + yy) / 143.0) + rng.randint(-6, 7, gray.shape), 0, 255)
    return np.stack([b, g, r], 2).astype(np.uint8)


def primaries(rows=64, cols=256):
    """Rows of pure blue, green, red, white, all 256 grays, and random colours."""
    img = np.random.RandomState(9).randint(0, 256, (rows, cols, 3)).astype(np.uint8)
    img[0:4], img[4:8], img[8:12] = (255, 0, 0), (0, 255, 0), (0, 0, 255)
    img[12:16] = 255
    img[16:20] = np.arange(cols, dtype=np.uint8)[None, :, None] if cols == 256 else 0
    return img
