"""An independent Python statement of stage a4, `corner_detector::edgeExtraction` (reference `corner_detector.cpp:125-463`):
ray-cast boundary, oriented walk, rotation to the point nearest the centroid, the extended Ramer-Douglas-Peucker loop with
`expand_line`, four Welsch line fits, their intersections and the quad judgment.

It is written from the reference text and from OpenCV 4.5.3's published `fitLine` (`linefit.cpp`: `fitLine2D_wods`, `fitLine2D`,
`calcDist2D`, `weightWelsch`; `cv::RNG`'s multiply-with-carry), not from the oracle, which it is compared with.  Its input per
candidate is the component's pixel set (from the oracle's labels: the labelling is pinned by scipy in `test_oracle_cpu.py`).

Two modes:
  "ref"  the reference's types: int points, float32 wherever the reference stores a float, double where it computes in double;
  "f64"  every real quantity in float64: the high-precision reference of the corners.

Every thresholded comparison on a candidate's path leaves a margin: |value - threshold| over the magnitude of the terms the value
is computed from (so a float32 rounding of those terms is about 1e-7 of it).  `Candidate.margin` is the smallest, `margin_site`
names its comparison.  A candidate whose answer differs between two statements of the same arithmetic can only be explained by a
comparison that lies that close to its threshold.

Where the reference's behaviour is undefined or unspecified this follows SURVEY App. B (B2, B7, B8, B10, B14), cited in place.
"""
import math
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
RESOLUTION_FACTOR = 12         # see fit_resolution_px
SAME_LINE_PX = 1e-4           # two Welsch lines this close over their cluster are one answer (a tenth of the 1e-3 px corner bar)
THRESHOLD_LINE = F32(1.8)     # header/corner_detector.h:90 (float members)
THRESHOLD_EXPAND = F32(1.2)
THRESHOLD_RAC = F32(0.3)      # :110
COST_LIMIT = 1.05             # corner_detector.cpp:285,288,337: a double literal against the float member `cost`
X_BIAS = (0, 1, 1, 1, 0, -1, -1, -1)  # header/corner_detector.h:86-87: neighbour order of the walk, clockwise from north
Y_BIAS = (-1, -1, 0, 1, 1, 1, 0, -1)


@dataclass
class Candidate:
    label: int
    area: int
    bbox: tuple                      # x_min, y_min, x_max, y_max
    has_quad: int = 0
    n_boundary: int = 0
    boundary: np.ndarray = None      # (n_boundary, 2) int (x, y) in walk order, before the rotation
    n_ray_cast: int = 0              # pixels the four scans mark: a walk that visits fewer stopped early
    rotated_start: int = 0           # index of the boundary point the list is rotated to
    corners: np.ndarray = field(default_factory=lambda: np.zeros((4, 2)))
    margin: float = math.inf
    margin_site: str = ""
    f32_resolution_px: float = 0.0   # how far the reference's float32 line fits can put a corner (see fit_resolution_px)
    failed_short: bool = False       # the RDP loop stopped with <= 2 points left (isFailed, :282-290)


class _Path:
    """The float arithmetic of one mode and the margin bookkeeping of one candidate."""

    def __init__(self, mode):
        assert mode in ("ref", "f64")
        self.f64 = mode == "f64"
        self.margin, self.site = math.inf, ""
        self.failed_short = False  # the RDP loop ran out of points (isFailed with <= 2 left)

    def r(self, v):
        """A value the reference stores as float: rounded to float32 in "ref" mode."""
        return float(v) if self.f64 else float(F32(v))

    def threshold(self, member, literal):
        """A float member initialised from a double literal: the member in "ref" mode, the literal in "f64" mode."""
        return float(literal) if self.f64 else float(member)

    def note(self, site, value, threshold, scale):
        m = abs(float(value) - float(threshold)) / max(float(scale), 1e-30)
        if m < self.margin:
            self.margin, self.site = m, site


# ------------------------------------------------------------------------------------------------ cv::fitLine, OpenCV 4.5.3

class _NumpyMath:
    """Elementary functions of the "ref" mode: the float exp of weightWelsch."""

    @staticmethod
    def expf(a):
        return np.exp(np.asarray(a, np.float32))


class SharedMath:
    """The float exp the project ships for both of its implementations (`ctag_math.h`'s exp32), reached through
    the oracle library's math probe.  It is a definition of expf, not a reading of the stage: weightWelsch's weights feed float32
    moment sums whose cancellation (x2 - x^2 of coordinates near 1000) turns a 1-ulp change of one weight into ~1e-5 of a line's
    direction, so "ref" mode needs the same expf as the code it is compared with to hold 1e-3 px.  "f64" mode never uses it."""

    def __init__(self, oracle):
        self.oracle = oracle

    def expf(self, a):
        a = np.asarray(a, np.float32)
        return self.oracle.math(8, a.astype(np.float64).ravel()).astype(np.float32).reshape(a.shape)


MATH = _NumpyMath()


def use_shared_math(oracle):
    """Route "ref" mode's expf through the project's shared exp32 (see SharedMath)."""
    global MATH
    MATH = SharedMath(oracle)


def _rng_subsets(n, _cache={}):
    """The 20 restarts' starting subsets of fitLine2D for n points: `RNG rng((uint64)-1)`, `uniform(0, n) = next() % n`, with
    next(): state = (uint32)state * 4164903690 + (state >> 32); min(n, 10) distinct indices per restart, in order of drawing."""
    if n in _cache:
        return _cache[n]
    state = (1 << 64) - 1
    out = np.zeros((20, n), np.float32)
    for k in range(20):
        i = 0
        while i < min(n, 10):
            state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
            j = (state & 0xFFFFFFFF) % n
            if out[k, j] < FLT_EPSILON:
                out[k, j] = 1.0
                i += 1
    _cache[n] = out
    return out


def fitline_l2_sums(sx, sy, sxx, syy, sxy, n, f64):
    """fitLine2D_wods without weights from exact integer moments: the double sums of float products of int coordinates are
    exact, so running sums give the same line as summing the points again.  Returns (vx, vy, x0, y0)."""
    w = float(n)
    x, y, x2, y2, xy = sx / w, sy / w, sxx / w, syy / w, sxy / w
    dx2, dy2, dxy = x2 - x * x, y2 - y * y, xy - x * y
    if f64:
        t = math.atan2(2 * dxy, dx2 - dy2) / 2
        return math.cos(t), math.sin(t), x, y
    t = F32(F32(math.atan2(2 * dxy, dx2 - dy2)) / F32(2))
    return float(F32(math.cos(float(t)))), float(F32(math.sin(float(t)))), float(F32(x)), float(F32(y))


def _seqsum(a):
    """A double accumulator filled left to right (np.sum would add pairwise)."""
    return np.cumsum(a, axis=-1, dtype=np.float64)[..., -1]


def _wods(px, py, w, f64):
    """fitLine2D_wods with weights, for a batch of weight rows w (m, n): `x += weights[i] * points[i].x` etc. are float
    products added into double sums.  Returns the m lines (m, 4)."""
    if f64:
        wx, wy = w * px, w * py
        sx, sy, sxx, syy, sxy = _seqsum(wx), _seqsum(wy), _seqsum(wx * px), _seqsum(wy * py), _seqsum(wx * py)
    else:
        wx, wy = w * px, w * py  # float32 arrays: float products
        sx, sy = _seqsum(wx), _seqsum(wy)
        sxx, syy, sxy = _seqsum(wx * px), _seqsum(wy * py), _seqsum(wx * py)
    sw = _seqsum(w.astype(np.float64))
    x, y, x2, y2, xy = sx / sw, sy / sw, sxx / sw, syy / sw, sxy / sw
    dx2, dy2, dxy = x2 - x * x, y2 - y * y, xy - x * y
    t = np.arctan2(2 * dxy, dx2 - dy2)
    if f64:
        t = t / 2
        return np.stack([np.cos(t), np.sin(t), x, y], 1)
    t = (t.astype(np.float32) / F32(2)).astype(np.float64)
    return np.stack([np.cos(t), np.sin(t), x, y], 1).astype(np.float32)


def fitline_welsch(pts, path, site, trace=None):
    """cv::fitLine(points, DIST_WELSCH, 0, 0.01, 0.01) = fitLine2D: 20 restarts from random subsets, each up to 30 weighted L2
    refits with Welsch weights exp(-d^2 / 2.9846^2); the restart with the smallest error sum wins (first one on equal sums), and
    an error sum below n * FLT_EPSILON ends the search.  The restarts depend on each other only through the RNG, so they run
    side by side here and are chosen between afterwards in order.
    `trace`: a dict that receives what the restarts did -- "iters" (20 ints: IRLS iterations run, i.e. error sums computed), "end" (20 of
    "converged" / "eps" / "cap": the convergence test passed, an error sum fell below n * FLT_EPSILON, 30 iterations), "unweighted" (20
    bools: a weight sum at or below FLT_EPSILON sent a refit to unit weights), "err" and "lines" (each restart's error sum and line as the
    selection sees them), "chosen" (the restart whose line is returned) and "stopped" (the selection ended on an error sum below EPS)."""
    n = len(pts)
    f64 = path.f64
    dt = np.float64 if f64 else np.float32
    px, py = pts[:, 0].astype(dt), pts[:, 1].astype(dt)
    EPS = n * FLT_EPSILON
    rdelta = adelta = 0.01 if f64 else float(F32(0.01))
    c = 1 / 2.9846 if f64 else F32(1) / F32(2.9846)
    w = _rng_subsets(n).astype(dt)
    line = _wods(px, py, w, f64)
    prev = np.zeros_like(line)
    err = np.zeros(20)
    active = np.ones(20, bool)
    iters, unweighted, end = np.zeros(20, int), np.zeros(20, bool), np.array(["cap"] * 20, dtype=object)
    for it in range(30):
        if it:
            t = line[:, 0] * prev[:, 0] + line[:, 1] * prev[:, 1]  # float products and sum, then widened
            t = np.clip(t.astype(np.float64), -1.0, 1.0)
            ang = np.abs(np.arccos(t))
            dx = np.abs(line[:, 2] - prev[:, 2]).astype(np.float64)
            dy = np.abs(line[:, 3] - prev[:, 3]).astype(np.float64)
            d = np.maximum(dx, dy)
            for k in np.nonzero(active)[0]:  # margins on the operands: the dot product t, the two centre coordinates
                path.note(site + ".welsch_angle", t[k], math.cos(adelta), 1.0)
                if ang[k] < adelta:
                    path.note(site + ".welsch_shift", d[k], rdelta, abs(float(line[k, 2])) + abs(float(line[k, 3])) + 1.0)
            end[active & (ang < adelta) & (d < rdelta)] = "converged"
            active &= ~((ang < adelta) & (d < rdelta))
            if not active.any():
                break
        # calcDist2D: float differences and products, a double sum
        xr, yr = px[None, :] - line[:, 2:3], py[None, :] - line[:, 3:4]
        dist = np.abs(line[:, 1:2] * xr + (-line[:, 0:1]) * yr)
        e = _seqsum(dist.astype(np.float64))
        err = np.where(active, e, err)
        iters += active
        end[active & (e < EPS)] = "eps"
        active &= ~(e < EPS)
        if not active.any():
            break
        # weightWelsch: w = exp(-d * d * c * c) as float, then normalised by a double sum
        ww = np.exp(-dist * dist * c * c) if f64 else MATH.expf(-dist * dist * c * c)
        sw = _seqsum(ww.astype(np.float64))
        big = np.abs(sw) > FLT_EPSILON
        unweighted |= active & ~big
        ww = np.where(big[:, None], (ww * (1.0 / np.where(big, sw, 1.0))[:, None]).astype(dt), dt(1))
        newline = _wods(px, py, ww, f64)
        prev = np.where(active[:, None], line, prev)
        line = np.where(active[:, None], newline, line)
    best, min_err = None, math.inf
    order = []
    for k in range(20):
        order.append(err[k])
        if err[k] < min_err:
            min_err, best = err[k], k
            if err[k] < EPS:
                break
    # A near-equal error sum of another restart decides nothing when that restart converged to the same line: only competitors
    # whose line lies SAME_LINE_PX or more from the chosen one somewhere along the cluster count as knife edges.  An error sum adds
    # n distances of points ~|x0| + |y0| from the origin.
    lb = line[best].astype(np.float64)
    t = (px.astype(np.float64) - lb[2]) * lb[0] + (py.astype(np.float64) - lb[3]) * lb[1]
    ends = [(lb[2] + lb[0] * u, lb[3] + lb[1] * u) for u in (t.min(), t.max())]
    rivals = []
    for k, e in enumerate(order):
        if e == min_err:
            continue
        lk = line[k].astype(np.float64)
        move = max(abs(lk[1] * (x - lk[2]) - lk[0] * (y - lk[3])) for x, y in ends)
        if move >= SAME_LINE_PX:
            rivals.append(e)
    if rivals:
        path.note(site + ".welsch_min", min(rivals), min_err, n * (abs(lb[2]) + abs(lb[3]) + 1.0))
    if trace is not None:
        trace.update(iters=iters, end=end, unweighted=unweighted, err=np.array(err, np.float64), lines=np.array(line), chosen=best,
                     stopped=bool(min_err < EPS))
    return [float(v) for v in line[best]]


# ------------------------------------------------------------------------------------------------ the stage

def ray_cast(mask):
    """The pixels the four scans of :197-232 mark on a component's mask: see boundary_walk."""
    rows, cols = mask.shape
    vis = np.zeros_like(mask, dtype=bool)
    jc = np.nonzero(mask.any(0))[0]
    vis[mask.argmax(0)[jc], jc] = True
    vis[rows - 1 - mask[::-1].argmax(0)[jc], jc] = True
    kr = np.nonzero(mask.any(1))[0]
    vis[kr, mask.argmax(1)[kr]] = True
    vis[kr, cols - 1 - mask[:, ::-1].argmax(1)[kr]] = True
    return vis


def boundary_walk(mask):
    """Ray casting (:197-232), the start point (:235-244) and the oriented walk (:246-247, :407-418) on a component's mask
    (rows x cols of its bounding box).  Returns the walk as (x, y) in box coordinates.

    The four scans stop at the first pixel that is either visited or foreground.  Visited pixels are foreground, so each scan
    leaves the first foreground pixel of its row or column visited: the set is the top and bottom pixel of every column and the
    left and right pixel of every row.  The start is the first of them in column-major order.  The walk is a
    depth-first recursion whose by-value `starter` is moved to each neighbour it takes, so that after a return the remaining
    directions are tried around the neighbour, not around the point the call began at; it stops when no direction of any
    open call finds an unvisited ray-cast pixel, which can leave some of them unwalked."""
    rows, cols = mask.shape
    vis = ray_cast(mask)
    cm = np.nonzero(vis.T.ravel())[0]
    if not len(cm):
        return np.zeros((0, 2), int)
    sx, sy = divmod(int(cm[0]), rows)
    vis = vis.tolist()
    vis[sy][sx] = False
    walk = [(sx, sy)]
    stack = [[sx, sy, 0]]  # one open call: its (moving) starter and the next direction to try
    while stack:
        fr = stack[-1]
        if fr[2] == 8:
            stack.pop()
            continue
        j = fr[2]
        fr[2] += 1
        nx, ny = fr[0] + X_BIAS[j], fr[1] + Y_BIAS[j]
        if 0 <= ny < rows and 0 <= nx < cols and vis[ny][nx]:
            walk.append((nx, ny))
            vis[ny][nx] = False
            fr[0], fr[1] = nx, ny
            stack.append([nx, ny, 0])
    return np.array(walk, int)


def _tri_cost(ep, a):
    """cost = norm(P[a] + P[a+2] - 2 P[a+1]) (indices mod n): cv::norm of an int Point is a double, stored in the float `cost`;
    it is the square root of an integer, so its float rounding never moves it across 1.05."""
    n = len(ep)
    p0, p1, p2 = ep[a], ep[(a + 1) % n], ep[(a + 2) % n]
    vx, vy = p0[0] + p2[0] - 2 * p1[0], p0[1] + p2[1] - 2 * p1[1]
    return math.sqrt(vx * vx + vy * vy)


def expand_line(ep, init, end, path):
    """:125-169.  The span init..end grows one point at a time to the left (init-1, init-2, ... wrapping from -1 to the last index)
    and to the right (end+1, ... wrapping from n to 0), alternately, each side until a point lies farther than threshold_expand
    from the L2 line of the points taken so far, which is refitted after every point.  A side that stops gives up the rest of
    that round.  The walk ends when the two cursors meet or every point is in the span; the wrap can take an index twice (B8).
    Returns the indices, largest first."""
    n = len(ep)
    f64 = path.f64
    span = list(range(init, end + 1))
    seg = ep[init:end + 1]
    sx, sy = int(seg[:, 0].sum()), int(seg[:, 1].sum())
    sxx, syy, sxy = int((seg[:, 0] ** 2).sum()), int((seg[:, 1] ** 2).sum()), int((seg[:, 0] * seg[:, 1]).sum())
    cnt = end - init + 1
    line = fitline_l2_sums(sx, sy, sxx, syy, sxy, cnt, f64)
    thr = path.threshold(THRESHOLD_EXPAND, 1.2)
    found_l = found_r = False
    left, right = init - 1, end + 1

    def dist(p, ln):
        vx, vy, x0, y0 = ln
        x, y = int(p[0]), int(p[1])
        if f64:
            t = abs(x * vy - y * vx + vx * y0 - vy * x0)
        else:  # int * float -> float, left to right
            r = path.r
            t = abs(r(r(r(r(x * vy) - r(y * vx)) + r(vx * y0)) - r(vy * x0)))
        path.note("expand", t, thr, abs(x * vy) + abs(y * vx) + abs(vx * y0) + abs(vy * x0))
        return t

    while (not found_l or not found_r) and left != right:
        if not found_l:
            if left == -1:
                left = n - 1
            if dist(ep[left], line) > thr:
                found_l = True
                continue
            p = ep[left]
            sx, sy, sxx, syy, sxy, cnt = sx + p[0], sy + p[1], sxx + p[0] * p[0], syy + p[1] * p[1], sxy + p[0] * p[1], cnt + 1
            span.append(left)
            left -= 1
            line = fitline_l2_sums(int(sx), int(sy), int(sxx), int(syy), int(sxy), cnt, f64)
            if cnt == n:
                break
        if not found_r:
            if right == n:
                right = 0
            if dist(ep[right], line) > thr:
                found_r = True
                continue
            p = ep[right]
            sx, sy, sxx, syy, sxy, cnt = sx + p[0], sy + p[1], sxx + p[0] * p[0], syy + p[1] * p[1], sxy + p[0] * p[1], cnt + 1
            span.append(right)
            right += 1
            line = fitline_l2_sums(int(sx), int(sy), int(sxx), int(syy), int(sxy), cnt, f64)
            if cnt == n:
                break
    return sorted(span, reverse=True)


def _rdp(ep, path):
    """:277-349, the extended Ramer-Douglas-Peucker loop: up to four edges, each grown by expand_line and cut out of the list.
    Returns the four point clusters (fewer when the loop fails)."""
    clusters = [[], [], [], []]
    ep = [tuple(p) for p in ep]
    cnt_boundary, init = 0, 0
    r = path.r
    thr_line = path.threshold(THRESHOLD_LINE, 1.8)
    while ep and cnt_boundary < 4:
        n = len(ep)
        if n <= 2:  # isFailed
            path.failed_short = True
            break
        cost = _tri_cost(ep, init)
        path.note("cost", cost, COST_LIMIT, COST_LIMIT)
        while cost > COST_LIMIT and init < n - 3:
            init += 1
            cost = _tri_cost(ep, init)
            path.note("cost", cost, COST_LIMIT, COST_LIMIT)
        end = min(init + n // 2, n - 1)
        failed = False
        while True:
            if end <= init + 1:
                failed = True
                break
            (xi, yi), (xe, ye) = ep[init], ep[end]
            k = 100.0 if xi == xe else r(1.0 * (ye - yi) / (xe - xi))  # a vertical chord gets slope 100 (:313-316)
            d_line = -r(r(k * xi) + r(-1 * yi))
            den = math.sqrt(k * k + 1) if path.f64 else r(math.sqrt(r(r(k * k) + 1)))
            d2l = []
            for it in range(init + 1, end):
                x, y = ep[it]
                if path.f64:
                    d = abs(k * x - y + d_line) / den
                else:
                    d = r(abs(r(r(r(k * x) + r(-1 * y)) + d_line)) / den)
                d2l.append(d)
                path.note("line", d, thr_line, (abs(k * x) + abs(y) + abs(d_line)) / den)
            dmax = max(d2l)
            if dmax > thr_line and len(d2l) > 1:
                # sort_indexes_greater is a stable sort: b[0 .. m-1] are the indices of the maximum in increasing order, and
                # `end = b[m-1]` is the last of them -- an index into dist2line, without its offset init + 1.
                others = [d for d in d2l if d != dmax]
                if others:
                    path.note("line_tie", max(others), dmax, max(dmax, 1.0) * 1e-2)
                end = max(i for i, d in enumerate(d2l) if d == dmax)
                continue
            span = expand_line(np.array(ep), init, end, path)
            for s in span:
                clusters[cnt_boundary].append(ep[s])
            # endpoint keeping (:336-339): the largest index stays in the list when the corner after it is a straight run
            cost = _tri_cost(ep, span[0])
            path.note("cost", cost, COST_LIMIT, COST_LIMIT)
            if cost < COST_LIMIT:
                span = span[1:]
            for s in span:  # largest first; an index taken twice is erased twice, and one past the end is a no-op (B8)
                if s < len(ep):
                    del ep[s]
            cnt_boundary += 1
            init = 0 if span[-1] >= len(ep) else span[-1]
            break
        if failed:
            break
    return clusters


def _quad(clusters, area_center, area, img_rows, img_cols, path):
    """:351-402: Welsch lines, their pairwise intersections near the centroid, sorted by angle, and the best 4-subset by
    quadJudgment under threshold_RAC.  Returns the corners or None."""
    f64 = path.f64
    r = path.r
    lines = []
    for j in range(4):
        if len(clusters[j]) < 2:
            return None
        lines.append(fitline_welsch(np.array(clusters[j], np.int64), path, "welsch%d" % j))
    cx, cy = area_center
    corners = []
    for j in range(3):
        for k in range(j + 1, 4):
            lj, lk = lines[j], lines[k]
            a00, a01, a10, a11 = lj[1], -lj[0], lk[1], -lk[0]
            b0 = r(r(lj[1] * lj[2]) - r(lj[0] * lj[3]))
            b1 = r(r(lk[1] * lk[2]) - r(lk[0] * lk[3]))
            det = a00 * a11 - a01 * a10  # determinant / solve of a 2x2 CV_32F: in double, times 1/det
            if det == 0:
                continue
            path.note("det", det, 0.0, abs(a00 * a11) + abs(a01 * a10))
            if f64:
                x, y = (b0 * a11 - b1 * a01) / det, (b1 * a00 - b0 * a10) / det
                dis = math.hypot(x - cx, y - cy)
                ang = math.atan2(y - cy, x - cx) * 180 / math.pi
            else:
                inv = 1.0 / det
                x, y = r((b0 * a11 - b1 * a01) * inv), r((b1 * a00 - b0 * a10) * inv)
                dx, dy = r(x - cx), r(y - cy)
                dis = r(math.sqrt(r(r(dx * dx) + r(dy * dy))))
                ang = r(r(r(np.arctan2(F32(dy), F32(dx))) * 180) / math.pi)  # atan2f * 180 in float, / CV_PI in double
            path.note("corner_dist", dis, min(img_cols, img_rows), min(img_cols, img_rows))
            if dis < img_cols and dis < img_rows:
                corners.append((ang, x, y))
    # std::sort of <= 6 elements is an insertion sort (libstdc++ below 16 elements): equal angles keep their order
    corners.sort(key=lambda c: c[0])
    for a, b in zip(corners, corners[1:]):
        path.note("angle_order", b[0], a[0], 360.0)
    # get_permutation (:420-452): every 4-subset in lexicographic order of the sorted list; a subset with a degenerate triangle
    # (|s| < 1) is skipped; the first smallest RAC below threshold_RAC wins
    best, rac_min = None, path.threshold(THRESHOLD_RAC, 0.3)
    racs = []
    n = len(corners)
    for i0 in range(n):
        for i1 in range(i0 + 1, n):
            for i2 in range(i1 + 1, n):
                for i3 in range(i2 + 1, n):
                    q = [corners[i][1:] for i in (i0, i1, i2, i3)]
                    degenerate = False
                    for a, b, cc in ((0, 1, 2), (1, 2, 3), (2, 3, 0), (0, 1, 3)):
                        s = _tri_area2(q[a], q[b], q[cc], r)
                        # three corners on one line make s ~ 0 up to float noise: measured against the threshold itself
                        path.note("triangle", abs(s), 1.0, 1.0)
                        degenerate |= abs(s) < 1
                    if degenerate:
                        continue
                    qa, scale = 0.0, 0.0
                    for i in range(4):
                        t = r(r(q[i][0] * q[(i + 1) % 4][1]) - r(q[i][1] * q[(i + 1) % 4][0]))
                        qa = r(qa + t)
                        scale += abs(q[i][0] * q[(i + 1) % 4][1]) + abs(q[i][1] * q[(i + 1) % 4][0])
                    qa = r(qa / 2)
                    rac = r(abs(r(abs(qa) - area)) / area)
                    path.note("rac", rac, path.threshold(THRESHOLD_RAC, 0.3), scale / area)
                    racs.append(rac)
                    if rac < rac_min:
                        rac_min, best = rac, q
    if best is None:
        return None
    others = [v for v in racs if v != rac_min]
    if others:
        path.note("rac_order", min(others), rac_min, 1.0)
    for x, y in best:
        path.note("inside", x, 0.0, img_cols)
        path.note("inside", y, 0.0, img_rows)
        path.note("inside", x, img_cols, img_cols)
        path.note("inside", y, img_rows, img_rows)
        if x < 0 or y < 0 or x > img_cols or y > img_rows:
            return None
    return np.array(best, np.float64)


def _tri_area2(p0, p1, p2, r):
    """Twice the signed area of a triangle as :428-431 write it (six float products, summed left to right)."""
    terms = (p0[0] * p1[1], p1[0] * p2[1], p2[0] * p0[1], -(p0[0] * p2[1]), -(p1[0] * p0[1]), -(p2[0] * p1[1]))
    s = 0.0
    for t in terms:
        s = r(s + r(t))
    return s


def fit_resolution_px(cluster):
    """How far a float32 line fit of these points may move a corner it makes.  fitLine2D_wods rounds every product w*x*x to
    float before the double sum, so each second moment carries an error of about FLT_EPSILON * (xbar^2 + ybar^2), against a
    spread of about L^2 / 12 for a cluster of extent L: the direction is good to ~12 FLT_EPSILON R^2 / L^2 radians, and a corner
    half a cluster away moves by ~6 FLT_EPSILON R^2 / L.  Two such lines meet at every corner, each off by as much: this is
    12 FLT_EPSILON R^2 / L (RESOLUTION_FACTOR).  Short clusters far from the origin (a few pixels, R ~ 1000) make it several
    hundredths of a pixel in the reference's own arithmetic."""
    p = np.asarray(cluster, np.float64)
    r2 = float(p[:, 0].mean() ** 2 + p[:, 1].mean() ** 2)
    extent = float(np.hypot(np.ptp(p[:, 0]), np.ptp(p[:, 1])))
    return RESOLUTION_FACTOR * FLT_EPSILON * r2 / max(extent, 1.0)


def extract_candidate(pixels, img_rows, img_cols, mode="ref", label=-1):
    """Stage a4 for one candidate.  pixels: (n, 2) int (x, y) of the component in the half image (img_rows x img_cols)."""
    pixels = np.asarray(pixels, np.int64)
    path = _Path(mode)
    # :184-189 the two sorts serve only the bounding box (B10)
    x_min, y_min = pixels.min(0)
    x_max, y_max = pixels.max(0)
    c = Candidate(label=label, area=len(pixels), bbox=(int(x_min), int(y_min), int(x_max), int(y_max)))
    mask = np.zeros((y_max - y_min + 1, x_max - x_min + 1), bool)
    mask[pixels[:, 1] - y_min, pixels[:, 0] - x_min] = True
    c.n_ray_cast = int(ray_cast(mask).sum())
    walk = boundary_walk(mask) + np.array([x_min, y_min])
    c.boundary, c.n_boundary = walk, len(walk)
    # :250-256 the centroid of the walked points: integer sums, a double quotient stored as float
    n = len(walk)
    sx, sy = int(walk[:, 0].sum()), int(walk[:, 1].sum())
    cx, cy = path.r(1.0 * sx / n), path.r(1.0 * sy / n)
    # :259-275 rotation to the point nearest the centroid.  sort_indexes_lesser is a std::stable_sort, so of equal distances the
    # first in walk order is b[0].
    r = path.r
    dist = []
    for x, y in walk.tolist():
        if path.f64:  # exact: n^2 times the squared distance to (sx / n, sy / n), in integers
            dist.append((n * x - sx) ** 2 + (n * y - sy) ** 2)
        else:
            dx, dy = r(x - cx), r(y - cy)
            dist.append(r(math.sqrt(r(r(dx * dx) + r(dy * dy)))))
    dmin = min(dist)
    b0 = dist.index(dmin)
    others = [d for d in dist if d != dmin]
    if others and not path.f64:
        path.note("nearest", min(others), dmin, abs(cx) + abs(cy) + 1.0)
    c.rotated_start = b0
    ep = np.concatenate([walk[b0:], walk[:b0]])
    clusters = _rdp(ep, path)
    c.f32_resolution_px = max((fit_resolution_px(cl) for cl in clusters if len(cl) >= 2), default=0.0)
    if all(clusters):
        quad = _quad(clusters, (cx, cy), c.area, img_rows, img_cols, path)
        if quad is not None:
            c.has_quad, c.corners = 1, quad
    c.margin, c.margin_site = path.margin, path.site
    c.failed_short = path.failed_short
    return c


def candidates_of_labels(labels):
    """The candidates of a labelled half image in label order (:86-106): components of 30 .. round(0.01 * cols * rows) pixels
    (`round` of a double: half away from zero).  Returns [(label, pixels (n, 2) int (x, y))]."""
    rows, cols = labels.shape
    limit = math.floor(0.01 * cols * rows + 0.5)
    flat = labels.ravel()
    order = np.argsort(flat, kind="stable")
    counts = np.bincount(flat)
    starts = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for lab in range(1, len(counts)):
        a = counts[lab]
        if a < 30 or a > limit:
            continue
        idx = order[starts[lab]:starts[lab + 1]]
        out.append((lab, np.stack([idx % cols, idx // cols], 1)))
    return out


def extract_frame(labels, mode="ref"):
    """Stage a4 for every candidate of a labelled half image."""
    rows, cols = labels.shape
    return [extract_candidate(px, rows, cols, mode, lab) for lab, px in candidates_of_labels(labels)]


def random_shapes_frame(state, seed, rows=720, cols=1152):
    """A synthetic marker frame (cropped to rows x cols) overlaid with a random population of dark shapes: rotated
    rectangles and quads of many sizes (incl. long bars wider than 128 half-res px and blobs near the 1 % area limit),
    rings, L-shapes, stacked quad pairs (feature candidates), tiny specks, some touching the frame border or a marker."""
    import testkit as tk
    rng = np.random.RandomState(1000 + seed)
    base = tk.synth_frame_host(state, 500 + seed, rows=max(1080, rows), cols=max(1920, cols))[0]  # (larger frames: a larger synthetic base)
    y0, x0 = rng.randint(0, base.shape[0] - rows + 1), rng.randint(0, base.shape[1] - cols + 1)
    img = base[y0:y0 + rows, x0:x0 + cols].astype(np.float32)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    k = float(np.sqrt(rows * cols / (1080.0 * 1920.0)))  # shape sizes follow the frame size (area limit = 1 % of it)

    def poly(pts, level):
        pts = np.asarray(pts, np.float32)
        inside = np.ones((rows, cols), bool)
        n = len(pts)
        e0, e1 = pts[1] - pts[0], pts[2] - pts[1]
        sign = np.sign(e0[0] * e1[1] - e0[1] * e1[0]) or 1.0
        for i in range(n):
            a, b = pts[i], pts[(i + 1) % n]
            inside &= sign * ((b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0])) >= 0
        img[inside] = level

    def rect(cx, cy, w, h, ang, level):
        c, s_ = np.cos(ang), np.sin(ang)
        poly([(cx + c * dx - s_ * dy, cy + s_ * dx + c * dy) for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))], level)

    for _ in range(rng.randint(25, 60)):
        kind = rng.randint(0, 7)
        cx, cy, ang = rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(0, np.pi)
        dark = rng.randint(10, 60)
        if kind == 0:
            rect(cx, cy, k * rng.uniform(16, 120), k * rng.uniform(16, 120), ang, dark)
        elif kind == 1:  # long bar
            rect(cx, cy, k * rng.uniform(200, 420), k * rng.uniform(14, 40), ang * (rng.rand() < 0.5), dark)
        elif kind == 2:  # ring
            w, h = k * rng.uniform(60, 160), k * rng.uniform(60, 160)
            rect(cx, cy, w, h, ang, dark)
            rect(cx, cy, w * 0.6, h * 0.6, ang, 200)
        elif kind == 3:  # L-shape
            w = k * rng.uniform(60, 140)
            rect(cx, cy, w, w / 4, ang, dark)
            c, s_ = np.cos(ang), np.sin(ang)
            rect(cx - c * w * 3 / 8 - s_ * w * 3 / 8, cy - s_ * w * 3 / 8 + c * w * 3 / 8, w / 4, w, ang, dark)
        elif kind == 4:  # stacked pair of narrow quads: a feature candidate
            w, h, gap = k * rng.uniform(20, 50), k * rng.uniform(60, 160), k * rng.uniform(8, 20)
            c, s_ = np.cos(ang), np.sin(ang)
            for sgn in (-1, 1):
                off = sgn * (h / 2 + gap / 2)
                rect(cx - s_ * off, cy + c * off, w, h * rng.uniform(0.5, 1.0), ang, dark)
        elif kind == 5:  # irregular convex quad
            r = k * rng.uniform(20, 90)
            angs = np.sort(rng.uniform(0, 2 * np.pi, 4))
            poly([(cx + r * np.cos(a), cy + r * np.sin(a)) for a in angs], dark)
        else:  # specks
            for _k in range(6):
                rect(cx + rng.uniform(-40, 40), cy + rng.uniform(-40, 40), rng.uniform(2, 14), rng.uniform(2, 14), ang, dark)
    return np.clip(img, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ comparison with an implementation

EXCUSE_MARGIN = 1e-5   # a candidate may miss a bar only with a comparison this close to its threshold (relative, see the module doc)
F64_EXCUSE_SHARE = 3e-3  # between "f64" and "ref" at most this share (past the issue's 0.1 %: the regular shape frames repeat a few
                         # float32 knife edges -- a float32 distance that lands on 1.8f -- in many copies)
RESOLUTION_SHARE = 0.05  # and at most this share of candidates may need the float32 fit resolution for their f64 corners
REF_TOL_PX = 1e-3      # "ref" corners against the implementation
F64_TOL_PX = 1e-2      # "f64" corners against "ref"


class Tally:
    """Candidates compared, and the ones excused by a margin, over any number of frames."""

    def __init__(self):
        self.compared, self.with_quad, self.excused_f64, self.failed, self.resolution = 0, 0, [], [], 0
        self.resolution_ratio = 0.0  # the largest (f64 - ref corner distance - F64_TOL_PX) / fit_resolution_px used

    def add(self, what, ref, f64, has_quad, n_boundary, quads):
        """ref / f64: the statement's candidates of one frame (f64 None: the two modes were compared elsewhere); has_quad,
        n_boundary, quads (n, 8): the implementation's."""
        f64 = ref if f64 is None else f64
        assert len(ref) == len(f64) == len(has_quad) == len(n_boundary) == len(quads), (what, len(ref), len(has_quad))
        for c, d, hq, nb, q in zip(ref, f64, has_quad, n_boundary, quads):
            self.compared += 1
            self.with_quad += int(hq)
            misses = []
            if c.n_boundary != nb:
                misses.append("n_boundary %d != %d" % (c.n_boundary, nb))
            if c.has_quad != hq:
                misses.append("has_quad %d != %d" % (c.has_quad, hq))
            elif hq and np.abs(c.corners.ravel() - q).max() > REF_TOL_PX:
                misses.append("ref corners off by %.2e px" % np.abs(c.corners.ravel() - q).max())
            if d.has_quad != c.has_quad:
                misses.append("f64 has_quad %d != ref %d" % (d.has_quad, c.has_quad))
            elif c.has_quad and np.abs(d.corners - c.corners).max() > F64_TOL_PX:
                off = np.abs(d.corners - c.corners).max()
                if off <= F64_TOL_PX + c.f32_resolution_px:  # within what the reference's float32 fits resolve
                    self.resolution += 1
                    self.resolution_ratio = max(self.resolution_ratio, (off - F64_TOL_PX) / c.f32_resolution_px)
                else:
                    misses.append("f64 corners off ref by %.2e px (float32 fit resolution %.1e)" % (off, c.f32_resolution_px))
            if not misses:
                continue
            margin, site = min((c.margin, c.margin_site), (d.margin, d.margin_site))
            entry = "%s label %d area %d: %s (margin %.1e at %s)" % (what, c.label, c.area, "; ".join(misses), margin, site)
            # Against the implementation nothing is excused: "ref" repeats the reference's float arithmetic, so a miss is a finding.
            # Between "f64" and "ref" a miss needs a comparison within EXCUSE_MARGIN of its threshold.
            if all(m.startswith("f64") for m in misses) and margin < EXCUSE_MARGIN:
                self.excused_f64.append(entry)
            else:
                self.failed.append(entry)

    def report(self):
        return ("%d candidates compared (%d with a quad, %d without); %d missed a bar against the implementation (none may); "
                "%d excused between f64 and ref by a margin below %.0e; %d f64 corners beyond %.0e px but within the float32 fit "
                "resolution of the reference (at most %.2f of it)%s") % (
            self.compared, self.with_quad, self.compared - self.with_quad, len(self.failed), len(self.excused_f64), EXCUSE_MARGIN,
            self.resolution, F64_TOL_PX, self.resolution_ratio, "".join("\n  excused: " + e for e in self.excused_f64))

    def check(self):
        assert not self.failed, "%d candidates missed a bar:\n%s" % (len(self.failed), "\n".join(self.failed[:40]))
        assert len(self.excused_f64) <= F64_EXCUSE_SHARE * self.compared, self.report()
        assert self.resolution <= RESOLUTION_SHARE * self.compared, self.report()
