"""`k_edge_refine_sums` alone, through the test kit's probe (`ctag_testkit_refine_sums`: the kernel with the plan's grid, 12 blocks of one
wave per frame) on caller-made corners and search results: the first 49 doubles of every quad's block must equal, byte for byte, the
running sums tests/refine_sums_testlib.py forms in numpy sample by sample with the reference's expressions.

The kernel works on two quads of a block at a time (q and q + 12).  The frames hold 2, 4, 22, 24, 26, 46, 48 and 50 quads -- a quad count
is twice a feature count, so these stand for 2, 3, 23, 24, 25, 26, 47 and 49: a lone quad, a partner in some blocks and not in others, an odd
leftover after a pair, two turns of a block's loop -- with a frame without features and frames whose status is not OK between them.  The
quads: no NaN; the first / the last / every sample of one edge NaN; all NaN (every sum +0.0, flag 1.0); NaNs scattered; an edge of more
than 1032 px (not this kernel's: flag 0.0, the block otherwise untouched) as either quad of a pair whose other quad is an ordinary one.

The expectation needs no GPU; the first test holds it to the independent statement of edgeRefine (tests/refine_testlib.py) on one quad of a
drawn frame, and every GPU test asks for that check first."""
import numpy as np
import pytest

import cylindertag_amd as ca
import refine_sums_testlib as rs
import refine_testlib as rt
import strip_shapes as ss
import testkit as tk
from cylindertag_amd import capi

PER_FRAME = 12  # ChunkPlan::refine_sums_gx


def _search_n0(img, quad, subpix):
    """n0 = Mn / Mcount per (edge, sample) of one quad with the statement's own search in its "f64" mode (refine_testlib._edge_moments, :618-655);
    NaN where a sample has no edge point."""
    rows, cols = img.shape
    a = quad.astype(np.float64)
    b = np.roll(a, -1, axis=0)
    nx, ny, ns = rs.edge_geometry(quad[None])
    nx, ny = nx[0], ny[0]
    assert (ns == 128).all()
    alpha = (15.0 + np.arange(128)) / 158
    x0 = alpha[None, :] * a[:, 0:1] + (1 - alpha[None, :]) * b[:, 0:1]
    y0 = alpha[None, :] * a[:, 1:2] + (1 - alpha[None, :]) * b[:, 1:2]
    n = np.arange(-subpix * 4, subpix * 4 + 1) * 0.25
    args = np.stack([x0[:, :, None] + (n + 1.0) * nx[:, None, None], y0[:, :, None] + (n + 1.0) * ny[:, None, None],
                     x0[:, :, None] + (n - 1.0) * nx[:, None, None], y0[:, :, None] + (n - 1.0) * ny[:, None, None]])
    x1, y1, x2, y2 = np.trunc(args).astype(np.int64)
    ok = (x1 >= 0) & (x1 < cols) & (y1 >= 0) & (y1 < rows) & (x2 >= 0) & (x2 < cols) & (y2 >= 0) & (y2 < rows)
    u1 = img[np.clip(y1, 0, rows - 1), np.clip(x1, 0, cols - 1)]
    u2 = img[np.clip(y2, 0, rows - 1), np.clip(x2, 0, cols - 1)]
    ok &= ~(u1 < u2)
    d = u2.astype(np.float64) / 255 - u1.astype(np.float64) / 255
    w = np.where(ok, d * d, 0.0)
    Mn = np.cumsum(w * n[None, None, :], axis=2)[:, :, -1]
    Mc = np.cumsum(w, axis=2)[:, :, -1]
    with np.errstate(all="ignore"):
        return np.where(Mc != 0, Mn / Mc, np.nan)


def check_expectation_against_the_statement():
    """One quad around a dark square on a light ground, corners at quarter pixels (their differences are exact in float and in double, the one
    place where the statement's types differ from the reference's): the lines of the expectation's sums equal the statement's in every bit."""
    img = np.full((240, 320), 215, np.uint8)
    img[60:170, 80:250] = 25
    img[60:170, 120:124] = 215  # a gap in the upper and lower edge: samples whose search finds no edge point ...
    img[100:110, :] = 215       # ... and in the left and right one
    quad = np.array([[79.25, 58.75], [251.5, 61.25], [248.75, 171.5], [81.5, 168.25]], np.float32)
    subpix = 3
    n0 = _search_n0(img, quad, subpix)
    assert 8 < np.isnan(n0).sum() < 200 and not np.isnan(n0).all(axis=1).any()
    sums = rs.expected_blocks([1], [0], np.concatenate([quad.reshape(-1), quad.reshape(-1)]), np.stack([n0, n0]))
    assert sums[0].tobytes() == sums[1].tobytes() and sums[0, 48] == 1.0
    A = quad.astype(np.float64)
    want_next, want_last = rt._edge_moments(img, A, np.roll(A, -1, axis=0), subpix, True, None, None)
    for p, want in enumerate((want_next, want_last)):
        Mx, My, Mxx, Mxy, Myy, N = sums[0, :48].reshape(4, 2, 6)[:, p, :].T
        Ex, Ey = Mx / N, My / N
        Cxx, Cxy, Cyy = Mxx / N - Ex * Ex, Mxy / N - Ex * Ey, Myy / N - Ey * Ey
        th = 0.5 * np.arctan2(-2 * Cxy, Cyy - Cxx)
        got = np.stack([Ex, Ey, np.cos(th), np.sin(th)], 1)
        assert got.tobytes() == want.tobytes(), (p, got, want)


def test_the_expectation_agrees_with_the_statement_on_one_quad():
    check_expectation_against_the_statement()


@pytest.fixture(scope="module")
def probe(dictionary):
    """A detector whose last chunk was nine blank frames with the corner refinement on: the workspace the probe writes into."""
    check_expectation_against_the_statement()
    state, fs = dictionary
    det = tk.Detector(state, fs, device=0)
    det.set_option(capi.OPT_STREAMS, 1)  # one chunk per call
    assert tk.chunk_plan(rows=ss.ROWS, cols=ss.COLS, nframes=9)["refine"].startswith("split")
    assert tk.chunk_plan(rows=ss.ROWS, cols=ss.COLS, nframes=9)["refine_sums_gx"] == PER_FRAME
    det.detect_batch(np.full((9, ss.ROWS, ss.COLS), 255, np.uint8))
    yield det
    det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rs.CALLS))
def test_sums_equal_the_running_sums_byte_for_byte(probe, name):
    call = rs.CALLS[name]
    nfeat, status, corners, n0, kinds = rs.make_call(call["quads"], call["dead"], call["seed"])
    assert len(nfeat) <= 9
    want = rs.expected_blocks(nfeat, status, corners, n0)
    got = probe.refine_sums(nfeat, status, corners, n0)
    frame = np.repeat(np.arange(len(nfeat)), 2 * nfeat)
    q_in_frame = np.concatenate([np.arange(2 * k) for k in nfeat])
    live = status[frame] == 0
    # what the call covers: every kind of quad in a live frame; a long quad in either slot of a pair with an ordinary partner
    assert set(np.array(kinds)[live]) == set(rs.KINDS)
    slots = set()
    for f, q, k in zip(frame[live], q_in_frame[live], np.array(kinds)[live]):
        nq, first = 2 * nfeat[f], q % (2 * PER_FRAME) < PER_FRAME
        partner = q + PER_FRAME if first else q - PER_FRAME
        if k == "long" and 0 <= partner < nq and rs.kind_of(f, partner) != "long":
            slots.add(0 if first else 1)
    assert slots == {0, 1}
    flat = n0.reshape(len(n0), -1)[:, :49]
    assert want[~live].tobytes() == flat[~live].tobytes()  # (the expectation leaves the frames that are not OK alone)
    allnan = np.array(kinds) == "all_nan"
    assert (np.signbit(want[live & allnan, :48]) == 0).all() and (want[live & allnan, :48] == 0).all() and (want[live & allnan, 48] == 1).all()
    bad = [(int(f), int(q), k) for f, q, k, g, w in zip(frame, q_in_frame, kinds, got, want) if g.tobytes() != w.tobytes()]
    print("\n%s: %d quads in %d frames, %d differ" % (name, len(got), len(nfeat), len(bad)))
    assert not bad, "quads (frame, quad, kind) whose 49 doubles differ from the running sums: %s" % bad[:20]


@pytest.mark.gpu
def test_the_probe_refuses_what_does_not_fit(probe):
    nfeat, status, corners, n0, _ = rs.make_call((2,) * 10, {}, 1)
    with pytest.raises(ca.CtagError):  # more frames than the last chunk had
        probe.refine_sums(nfeat, status, corners, n0)
    with pytest.raises(ca.CtagError):  # so few frames that the plan runs edgeRefine as one kernel
        probe.refine_sums(nfeat[:2], status[:2], corners[:2], n0[:4])
