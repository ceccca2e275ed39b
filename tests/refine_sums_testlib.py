"""What `k_edge_refine_sums` (cylindertag_amd/csrc/k_feature.hip) must leave in a quad's block, stated in numpy from the reference text
(`corner_detector.cpp:609-615` the edge's normal and sample count, `:619-621` the sample's point on the edge, `:651-664` / `:734-739` the
point moved along the normal and the twelve running sums), and the quads tests/test_refine_sums_gpu.py feeds it.

The kernel's input is the search's result per sample, n0 = Mn / Mcount (NaN: the reference's `continue` at Mcount == 0), and the quad's
four corners.  A sum is a double accumulator filled in sample order 0..127; a sample without an edge point is SKIPPED here, as the
reference skips it -- the kernel adds +0.0 instead, and the bytes must still be equal.  Every rounding is the reference's: the float
subtraction of two corner coordinates widened to double, `alpha * a + (1 - alpha) * b` with the float corners widened first,
`bestx * bestx * w` as `(bestx * bestx) * w`.

A quad with an edge of more than 128 samples (longer than 1032 px) is not this kernel's: it leaves the block alone and writes 0.0 at
[48].  A frame whose status is not OK is left alone altogether."""
import numpy as np

SAMPLES = 128
MOMENTS = ("Mx", "My", "Mxx", "Mxy", "Myy", "N")


def edge_geometry(corners):
    """corners float32 [nq, 4, 2] -> (nx, ny, nsamples) per edge [nq, 4]: edge e runs from corner e to corner (e + 1) & 3 (:606-615)."""
    a = np.asarray(corners, np.float32)
    b = np.roll(a, -1, axis=1)
    nx = (b[:, :, 1] - a[:, :, 1]).astype(np.float64)   # Point2f - Point2f: a float difference, then double
    ny = (-b[:, :, 0] + a[:, :, 0]).astype(np.float64)
    mag = np.sqrt(nx * nx + ny * ny)
    with np.errstate(all="ignore"):
        ns = np.where(mag / 8 > 128.0, mag / 8, 128.0).astype(np.int64)  # max(128.0, mag / 8), truncated
        return nx / mag, ny / mag, ns


def expected_blocks(nfeat, status, corners, n0, ok_status=0):
    """The first 49 doubles of every quad's block after the kernel: nfeat, status per frame; corners float32 [sum nfeat, 16];
    n0 float64 [sum 2 nfeat, 4, 128] -> float64 [sum 2 nfeat, 49]."""
    n0 = np.asarray(n0, np.float64).reshape(-1, 4, SAMPLES)
    nq = len(n0)
    quads = np.asarray(corners, np.float32).reshape(nq, 4, 2)
    a = quads.astype(np.float64)
    b = np.roll(a, -1, axis=1)
    nx, ny, ns = edge_geometry(quads)
    acc = np.zeros((nq, 4, 2, 6))  # quad, edge, weighting (towards the next corner, towards the last), moment
    for s in range(SAMPLES):
        alpha = (15.0 + s) / (SAMPLES + 30)  # :619 at nsamples == 128
        x0 = alpha * a[:, :, 0] + (1 - alpha) * b[:, :, 0]
        y0 = alpha * a[:, :, 1] + (1 - alpha) * b[:, :, 1]
        n = n0[:, :, s]
        used = ~np.isnan(n)
        with np.errstate(all="ignore"):
            bestx = x0 + n * nx
            besty = y0 + n * ny
            for p, w in enumerate((1 - alpha, alpha)):
                terms = (bestx * w, besty * w, bestx * bestx * w, bestx * besty * w, besty * besty * w, np.full_like(bestx, w))
                for m, t in enumerate(terms):
                    acc[:, :, p, m] = np.where(used, acc[:, :, p, m] + t, acc[:, :, p, m])
    out = n0.reshape(nq, 4 * SAMPLES)[:, :49].copy()  # what the kernel does not write stays
    frame_of_quad = np.repeat(np.arange(len(nfeat)), 2 * np.asarray(nfeat))
    live = np.asarray(status)[frame_of_quad] == ok_status
    short = (ns <= SAMPLES).all(axis=1)
    out[live & short, :48] = acc.reshape(nq, 48)[live & short]
    out[live & short, 48] = 1.0
    out[live & ~short, 48] = 0.0
    return out


# ---- the quads of the GPU test -------------------------------------------------------------------------------------------------------
KINDS = ("plain", "first_nan", "last_nan", "edge_nan", "all_nan", "long", "scattered_nan", "plain")


def kind_of(frame, q):
    """Quads q and q + 12 -- the two slots of a wave at 12 blocks per frame -- are four kinds apart: a long quad has a "first_nan" partner and is
    one's partner, in either slot."""
    return KINDS[(q * 5 + frame) % len(KINDS)]


def make_call(quads_per_frame, dead, seed):
    """One call of the probe: quads_per_frame[f] quads in frame f; dead: {frame: status} frames the kernel must leave alone (they keep their
    features).  -> nfeat, status, corners [sum nfeat, 16], n0 [sum quads, 4, 128], kinds [sum quads]"""
    rng = np.random.default_rng(seed)
    nfeat = np.array([q // 2 for q in quads_per_frame], np.int32)
    assert all(q % 2 == 0 for q in quads_per_frame)
    status = np.array([dead.get(f, 0) for f in range(len(nfeat))], np.int32)
    corners, n0, kinds = [], [], []
    for f, nq in enumerate(quads_per_frame):
        for q in range(nq):
            kind = kind_of(f, q)
            c = rng.uniform((100, 100), (1800, 1000))
            half = rng.uniform(20, 110, 2)
            quad = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]]) * half + c + rng.uniform(-8, 8, (4, 2))
            if kind == "long":
                quad = np.array([[10.25, 10.5], [1200.75, 14.5], [1198.5, 100.25], [12.5, 98.75]]) + rng.uniform(0, 3, (4, 2))
            block = rng.uniform(-5, 5, (4, SAMPLES))
            e = int(rng.integers(4))
            if kind == "first_nan":
                block[e, 0] = np.nan
            elif kind == "last_nan":
                block[e, SAMPLES - 1] = np.nan
            elif kind == "edge_nan":
                block[e, :] = np.nan
            elif kind == "all_nan":
                block[:] = np.nan
            elif kind == "scattered_nan":
                block[rng.random((4, SAMPLES)) < 0.1] = np.nan
            corners.append(quad.astype(np.float32))
            n0.append(block)
            kinds.append(kind)
    corners = np.array(corners, np.float32).reshape(-1, 16) if corners else np.zeros((0, 16), np.float32)
    n0 = np.array(n0, np.float64).reshape(-1, 4, SAMPLES)
    return nfeat, status, corners, n0, kinds


# Quads per frame (2 nfeat: always even).  With 12 blocks per frame and two quads per wave: 2 and 4 -- blocks with a lone quad; 22 -- ten pairs and two
# lone quads, a partner in some blocks and none in others; 24 -- every block one pair; 26 -- a pair, then an odd leftover; 46 -- two turns of the loop, the
# second a lone quad in two blocks; 48 -- two full turns; 50 -- two turns and a leftover.  They are the even neighbours of 3, 23, 25, 47 and 49.
# Between them a frame without features and frames whose status is not OK (1: CTAG_NO_FEATURE), which keep their features and n0.
CALLS = {
    "up to one pair": dict(quads=(2, 6, 4, 0, 22, 24, 10, 26, 24), dead={1: 1, 6: 1}, seed=11),
    "two turns": dict(quads=(48, 0, 46, 8, 50, 26, 2), dead={3: 1}, seed=12),
}
