"""An independent Python statement of stage a7, `corner_detector::edgeRefine` (reference `corner_detector.cpp:600-951`), and of
the flow of `CylinderTag::detect` behind edgeExtraction (`CylinderTag.cpp:87-128`) over the stages of `tests/marker_testlib.py`.

It is written from the reference text and SURVEY App. A.2 (`convertTo(CV_32F, 1 / 255)`) and App. D only; `oracle/ctag_oracle.cpp`,
`k_feature.hip` and `ctag_refine.h`, which it is compared with, were not read while it was written.

For each of a feature's two quads the reference runs the same edge search four times twice over (`:605-679` and `:681-755`, again
`:778-852` and `:854-928`): the two runs of an edge differ only in the weight of a sample in the line moments, (1 - alpha) for
`lines_next` and alpha for `lines_last`.  The search of an edge is stated once here, on (samples x steps) arrays, and the two
sets of moments are summed from it in sample order (`np.cumsum`: a double accumulator filled left to right).  `features_refined`
is `features` itself (`CylinderTag.cpp:102`); a quad's corners are written only after its eight lines are fitted, and the second
quad reads corners 4..7, so the aliasing changes nothing.

Two modes:
  "ref"  the reference's types: everything double except the pixel values (`float(u) * float(1.0 / 255)`), the weight
         `(g2 - g1) * (g2 - g1)` (a float product), `atan2f` / `cosf` / `sinf` on arguments narrowed to float (from MATH of
         marker_testlib: see its use_shared_math) and the stored corner;
  "f64"  pixel values u / 255, the weight, the trigonometry (libm) and the corner in float64.
The truncations `int x1 = x0 + (n + 1) * nx` act on doubles computed from the same float corners in both modes.

Margins: the distance of every truncated argument from an integer (relative to 1 px), `fabs(det) > 0.001` and `g1 < g2` never
being a rounding question (pixel values are exact multiples), per feature in `Trace.item_margin`.  An edge without a usable
sample has N == 0: its moments are 0 / 0 = NaN, the NaN passes through atan2f / cosf / sinf into `det`, `fabs(NaN) > 0.001` is
false and the old corner is kept (`:773-775`).
"""
import math

import numpy as np

import marker_testlib as mt

F32 = np.float32
# What a7's float32 steps resolve.  A line's normal angle passes through float three times: atan2f's result (an ulp of 2 theta <= pi,
# halved: 2^-23 rad), the narrowing of .5 * that for cosf / sinf (exact: a halved float), and the two float results (half an ulp of
# a value <= 1 each, 2^-25, at right angles to the direction they move it in: at most 2^-24 rad together) -- with the last-ulp
# error libm allows atan2f / cosf / sinf themselves, 3 * 2^-23 rad per line.  A corner is the meeting point of two such lines, each
# turned about its own centroid (Ex, Ey): it moves by (lever_next + lever_last) * DIRECTION_RESOLUTION / |det|, det being the
# sine of the angle between the lines.  The pixel values and the weight product are float too, but they enter as relative 1e-7
# changes of weights inside a window of +-range px: below 1e-5 px.  An ordinary corner (levers of 100 px, det near 1) gets 7e-5 px;
# near-parallel lines that throw a corner thousands of pixels away get whole millipixels.
DIRECTION_RESOLUTION = 3 * 2.0 ** -23


def _edge_moments(img, A, B, subpix, f64, tr, item):
    """The search of :618-665 for m edges from corners A to B ((m, 2) doubles) with the same nsamples; returns the two line
    fits (Ex, Ey, nx, ny) with weights (1 - alpha) and alpha, each (m, 4)."""
    rows, cols = img.shape
    nx = B[:, 1] - A[:, 1]
    ny = -B[:, 0] + A[:, 0]
    mag = np.sqrt(nx * nx + ny * ny)
    with np.errstate(all="ignore"):
        nx, ny = nx / mag, ny / mag
        ns = np.maximum(128.0, mag / 8)
    ns = np.where(np.isfinite(ns), ns, 128.0).astype(np.int64)  # :615, truncation
    assert (ns == ns[0]).all()
    ns = int(ns[0])
    alpha = (15.0 + np.arange(ns)) / (ns + 30)  # :619
    x0 = alpha[None, :] * A[:, 0:1] + (1 - alpha[None, :]) * B[:, 0:1]
    y0 = alpha[None, :] * A[:, 1:2] + (1 - alpha[None, :]) * B[:, 1:2]
    n = np.arange(-subpix * 4, subpix * 4 + 1) * 0.25  # :627: -range, -range + 0.25 ... range, exact in binary
    with np.errstate(all="ignore"):
        ax1 = x0[:, :, None] + (n + 1.0)[None, None, :] * nx[:, None, None]
        ay1 = y0[:, :, None] + (n + 1.0)[None, None, :] * ny[:, None, None]
        ax2 = x0[:, :, None] + (n - 1.0)[None, None, :] * nx[:, None, None]
        ay2 = y0[:, :, None] + (n - 1.0)[None, None, :] * ny[:, None, None]
        args = np.stack([ax1, ay1, ax2, ay2])
        finite = np.isfinite(args).all(0)
        ints = np.trunc(np.where(np.isfinite(args), args, -1.0)).astype(np.int64)  # double -> int: toward zero
    x1, y1, x2, y2 = ints
    ok = finite & (x1 >= 0) & (x1 < cols) & (y1 >= 0) & (y1 < rows) & (x2 >= 0) & (x2 < cols) & (y2 >= 0) & (y2 < rows)  # :631-637
    if tr is not None:
        near = np.abs(args - np.rint(args))
        near = np.where(np.isfinite(near), near, 0.0).min(axis=(0, 2, 3))
        for k, v in enumerate(near):
            tr.note("a7.truncation", v, 0.0, 1.0, item[k])
        # an axis-aligned edge between corners at x.5 (or y.5): the normal is exactly (+-1, 0) or (0, +-1) and every fourth step of n has
        # a truncation argument that is an integer
        half = lambda v: np.abs(v - np.floor(v) - 0.5) == 0  # noqa: E731
        aligned = ((np.abs(nx) == 1) & (ny == 0) & half(A[:, 0]) & half(B[:, 0])) | ((np.abs(ny) == 1) & (nx == 0) & half(A[:, 1]) & half(B[:, 1]))
        tr.hit("a7.axis_aligned_edge_at_half_pixel", int(np.sum(aligned & (near == 0))))
        tr.hit("a7.out_of_bounds", int(np.sum(~ok)))
        tr.hit("a7.negative_truncated_to_0", int(np.sum((args > -1) & (args < 0) & finite[None])))
    cl = lambda v, hi: np.clip(v, 0, hi - 1)  # noqa: E731
    u1 = img[cl(y1, rows), cl(x1, cols)]
    u2 = img[cl(y2, rows), cl(x2, cols)]
    ok &= ~(u1 < u2)  # :642 g1 < g2: continue
    if f64:
        d = u2.astype(np.float64) / 255 - u1.astype(np.float64) / 255
        w = d * d
    else:
        s = F32(1.0 / 255)
        d = u2.astype(np.float32) * s - u1.astype(np.float32) * s
        w = (d * d).astype(np.float64)  # a float product, widened
    w = np.where(ok, w, 0.0)  # a skipped step adds nothing; x + 0.0 == x
    Mn = np.cumsum(w * n[None, None, :], axis=2)[:, :, -1]
    Mc = np.cumsum(w, axis=2)[:, :, -1]
    used = Mc != 0  # :651
    with np.errstate(all="ignore"):
        n0 = Mn / Mc
        bx = x0 + n0 * nx[:, None]
        by = y0 + n0 * ny[:, None]
    bx, by = np.where(used, bx, 0.0), np.where(used, by, 0.0)
    if tr is not None:
        tr.hit("a7.sample_unused", int(np.sum(~used)))
        tr.hit("a7.edge_without_sample", int(np.sum(~used.any(1))))
    out = []
    for wt in (1 - alpha, alpha):
        wt = np.where(used, wt[None, :], 0.0)
        seq = lambda a: np.cumsum(a, axis=1)[:, -1]  # noqa: E731
        Mx, My = seq(bx * wt), seq(by * wt)
        Mxx, Mxy, Myy, N = seq(bx * bx * wt), seq(bx * by * wt), seq(by * by * wt), seq(wt)
        with np.errstate(all="ignore"):
            Ex, Ey = Mx / N, My / N
            Cxx, Cxy, Cyy = Mxx / N - Ex * Ex, Mxy / N - Ex * Ey, Myy / N - Ey * Ey
            if f64:
                th = 0.5 * np.arctan2(-2 * Cxy, Cyy - Cxx)
                lx, ly = np.cos(th), np.sin(th)
            else:
                th = 0.5 * mt.MATH.atan2f((-2 * Cxy).astype(np.float32), (Cyy - Cxx).astype(np.float32)).astype(np.float64)  # :672
                lx = mt.MATH.cosf(th.astype(np.float32)).astype(np.float64)
                ly = mt.MATH.sinf(th.astype(np.float32)).astype(np.float64)
        out.append(np.stack([Ex, Ey, lx, ly], 1))
    return out


def refine_features(gray, features1, subpix_dist, mode, trace=None):
    """a7: (nf, 19) features in full-size coordinates -> the same with refined corners (centre and angle stay as they are)."""
    f64 = mode == "f64"
    tr = trace
    dt = np.float64 if f64 else np.float32
    f = np.array(features1, dt).reshape(-1, 19)
    nf = len(f)
    if nf == 0:
        return f
    img = np.ascontiguousarray(gray, np.uint8)
    C = f[:, :16].astype(np.float64).reshape(nf, 2, 4, 2)  # feature, quad, corner, xy
    A = C.reshape(nf * 2, 4, 2)
    Bn = np.roll(A, -1, 1)
    A, Bn = A.reshape(-1, 2), Bn.reshape(-1, 2)  # edge e of quad q: row q * 4 + e, from corner e to corner (e + 1) & 3
    item = np.repeat(np.arange(nf), 8)
    mag = np.hypot(*(Bn - A).T)
    with np.errstate(all="ignore"):
        ns = np.where(np.isfinite(mag), np.maximum(128.0, mag / 8), 128.0).astype(np.int64)
    nxt, lst = np.zeros((len(A), 4)), np.zeros((len(A), 4))
    for v in np.unique(ns):
        sel = np.nonzero(ns == v)[0]
        if v > 128 and tr is not None:
            tr.hit("a7.long_edge", len(sel))
        for lo in range(0, len(sel), 64):  # (64 x 128 x 81 doubles at most in one array)
            s = sel[lo:lo + 64]
            a, b = _edge_moments(img, A[s], Bn[s], int(subpix_dist), f64, tr, item[s])
            nxt[s], lst[s] = a, b
    nxt, lst = nxt.reshape(nf * 2, 4, 4), lst.reshape(nf * 2, 4, 4)
    out = C.reshape(nf * 2, 4, 2).copy()
    for it in range(4):  # :757-776
        k = (it + 1) & 3
        A00, A01 = nxt[:, it, 3], -lst[:, k, 3]
        A10, A11 = -nxt[:, it, 2], lst[:, k, 2]
        B0, B1 = -nxt[:, it, 0] + lst[:, k, 0], -nxt[:, it, 1] + lst[:, k, 1]
        with np.errstate(all="ignore"):
            det = A00 * A11 - A10 * A01
            W00, W01 = A11 / det, -A01 / det
            L0 = W00 * B0 + W01 * B1
            x, y = nxt[:, it, 0] + L0 * A00, nxt[:, it, 1] + L0 * A10
            good = np.abs(det) > 0.001  # false for NaN
        if tr is not None:
            with np.errstate(all="ignore"):
                res = (np.hypot(x - nxt[:, it, 0], y - nxt[:, it, 1]) + np.hypot(x - lst[:, k, 0], y - lst[:, k, 1])) * DIRECTION_RESOLUTION / np.abs(det) \
                    + 2.0 ** -24 * np.maximum(np.abs(x), np.abs(y))  # and the stored corner is a float: half an ulp of its coordinate
            for q in np.nonzero(good)[0]:
                tr.resolution[q // 2] = max(tr.resolution.get(q // 2, 0.0), float(res[q]))
            for q in range(nf * 2):
                if math.isnan(det[q]):
                    tr.hit("a7.nan_determinant")
                else:
                    tr.note("a7.determinant", abs(det[q]), 0.001, 1.0, q // 2)
            tr.hit("a7.corner_kept", int(np.sum(~good)))
        out[:, k, 0] = np.where(good, x, out[:, k, 0])
        out[:, k, 1] = np.where(good, y, out[:, k, 1])
    f[:, :16] = out.reshape(nf, 16).astype(dt)
    return f


def back_half(quads, gray, state, feature_size, mode, subpix=True, subpix_dist=5, params=None):
    """CylinderTag::detect from its first early return on (CylinderTag.cpp:87-128): quads -> the result record, and the stages
    on the way {features0, features1, features2, premarkers, result, traces}."""
    T = {k: mt.Trace() for k in ("a5", "a7", "a8", "a10")}
    out = {"traces": T}
    if len(quads) == 0:  # :87-90
        out["result"] = out["premarkers"] = mt._empty_result(mode, mt.NO_CORNER)
        return out
    if len(quads) > mt.MAX_QUADS:
        out["result"] = out["premarkers"] = mt._empty_result(mode, mt.ERR_LIMIT, mt.FLAG_QUAD_OVERFLOW)
        return out
    f0, pairs = mt.recover_features(quads, mode, params, T["a5"])
    out["features0"], out["pairs"] = f0, pairs
    if len(f0) < feature_size:  # :93-96
        out["result"] = out["premarkers"] = mt._empty_result(mode, mt.NO_FEATURE)
        return out
    f1 = mt.obtain_corners(f0, mode)
    f2 = refine_features(gray, f1, subpix_dist, mode, T["a7"]) if subpix else f1.copy()
    out["features1"], out["features2"] = f1, f2
    pre = mt.organize_markers(f2, mode, params, T["a8"])
    out["premarkers"] = pre
    out["result"] = mt.decode_markers(pre, state, feature_size, mode, T["a10"])
    return out
