"""Seed models for the model reconstruction (Detector.fit_model): the ideal cylinder a printed strip of a dictionary makes when it
is wrapped round a tube of known nominal radius.  The strip geometry is the one the synthetic 3-D scenes print
(testkit/ctag_synth.h: model_corners): strip height L, bars L / 15 wide at a pitch of L / 10, the two gap centres of a bar from its
code's cross ratios."""
import numpy as np

MAX_COLS = 20  # CTAG_MAX_CODE_POS
CROSS_RATIOS = (1.47, 1.54, 1.61, 1.68, 1.68, 1.61, 1.54, 1.47)  # ID_cr_correspond, mirrored for ids 4 .. 7


def gap_centre(code_id, strip_height):
    """Distance of a gap's centre from the strip's edge for id 0 .. 7: a root of p^2 - L p - k L^2 = 0, k = 0.11 - 0.2 cr."""
    k = 0.11 - 0.2 * CROSS_RATIOS[code_id]
    disc = np.sqrt(1.0 + 4.0 * k)
    return 0.5 * strip_height * (1.0 + disc) if code_id >= 4 else 0.5 * strip_height * (1.0 - disc)


def default_radius(row, n_cols, strip_height=60.0):
    """The radius the synthetic scenes give dictionary row `row` (testkit/ctag_synth.h: row_radius_mm)."""
    return n_cols * 0.1 * strip_height * (0.45 + 0.08 * ((row * 7 + 3) % 11))


def cylinder_model(state, strip_height, radius_per_row):
    """Corner lists of the ideal cylinders: float32 [rows, cols * 8, 3] in the object frame (x along the strip, bent round the axis
    y, z out of the strip's middle), corner order as detect() emits it.  state: the dictionary [rows, cols] (codes 0 .. 63);
    radius_per_row: one radius for all rows or one per row, in the unit of strip_height.  Ready for Model(ids=range(rows), ...)."""
    state = np.asarray(state, np.int64)
    rows, dcols = state.shape
    n = min(dcols, MAX_COLS)
    L = float(strip_height)
    radius = np.broadcast_to(np.asarray(radius_per_row, np.float64), (rows,))
    W, cw, pitch = n * 0.1 * L, L / 15.0, 1.5 * L / 15.0
    out = np.zeros((rows, n * 8, 3), np.float32)
    for row in range(rows):
        r = float(radius[row])
        for c in range(n):
            code = int(state[row, c])
            gl, gr = gap_centre(code // 8, L), gap_centre(code % 8, L)
            u0 = c * pitch
            u1 = u0 + cw
            uv = ((u0, 0.0), (u1, 0.0), (u1, gr - 0.1 * L), (u0, gl - 0.1 * L), (u1, L), (u0, L), (u0, gl + 0.1 * L), (u1, gr + 0.1 * L))
            for k, (u, v) in enumerate(uv):
                th = (u - 0.5 * W) / r
                out[row, c * 8 + k] = (r * np.sin(th), v - 0.5 * L, r - r * np.cos(th))
    return out
