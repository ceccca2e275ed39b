"""k_welsch's two forms of the Welsch weight (cylindertag_amd/csrc/k_quad.hip: welsch_weight): a wave whose active lanes all have an argument with
`exp32_k_is_zero` takes the bare polynomial `exp32_nonpos_k0`, any other wave trip the general `exp32_nonpos`.  Clusters built so that a trip's side is
known, through the test kit's probe of the stage (`Detector.welsch_fit`) on the workspace of 32 blank 1080p frames, against `oracle.fitline`: all 16 bytes
of every line, nothing excluded.
  (a) clean straight segments, twelve of one size per frame (one block of k_welsch), sizes at and around the weight cache (16) and in each staging mode
      (float pairs up to 128, packed words up to 240, global memory above): every point lies within a pixel of every restart's line, every trip is fast at all
      three sites (first pass cached and uncached, second pass recomputed);
  (b) the frames of (a) with ONE point of ONE edge moved off its segment by 1 .. 60 px, once at an index below 16 and once above: at that trip the wave is
      mixed -- the other lanes have k = 0, the restarts of that edge k = -1 .. -25 or, for 30 and 60 px, an argument below the flush at -87;
  (c) two frames in which EVERY edge carries such a point at the same index: a trip in which no lane has k = 0.
The last test holds math probe 17 (`exp32_nonpos_k0` on the device) against the host's `exp32_nonpos` on arguments where the predicate holds."""
import numpy as np
import pytest

import testkit as tk
import welsch_shapes as ws
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

SIZES = (11, 16, 17, 40, 128, 129, 241)
MOVES = (1, 2, 3, 5, 12, 30, 60)
EDGES = 12  # = kWE: one block of k_welsch per frame
MARGIN = 80  # room for the moved point inside the frame


def clean_segment(rng, n):
    """n points of a straight segment in a random direction, rounded to the grid in walk order -> (points, unit normal)."""
    half = min(max(n * rng.uniform(0.8, 1.4), 4.0), 900.0) / 2
    ang = rng.uniform(0, 2 * np.pi)
    cx, cy = rng.uniform(half + MARGIN, 1920 - 1 - MARGIN - half), rng.uniform(half + MARGIN, 1080 - 1 - MARGIN - half)
    t = np.linspace(-half, half, n)
    p = np.rint(np.stack([cx + t * np.cos(ang), cy + t * np.sin(ang)], 1)).astype(np.int32)
    return p, np.array([-np.sin(ang), np.cos(ang)])


def moved(seg, at, d):
    p, normal = seg
    q = p.copy()
    q[at] += np.rint(d * normal).astype(np.int32)
    return q


def _clean_frames():
    rng = np.random.default_rng(20241019)
    return {n: [clean_segment(rng, n) for _ in range(EDGES)] for n in SIZES}


CLEAN = _clean_frames()


def _batch(frames):
    calls = [dict(frames=list(range(i, min(i + 32, len(frames)))), latency=0, gx=0, gs=0, tail=False) for i in range(0, len(frames), 32)]
    return dict(size=ws.HD, frames=frames, calls=calls)


def batch_clean():
    return _batch([("%d clean edges of %d points" % (EDGES, n), [p for p, _ in CLEAN[n]]) for n in SIZES])


def batch_one_moved():
    frames = []
    for n in SIZES:
        for i, d in enumerate(MOVES):
            for at in (3 + i, 16 + (5 * i + 1) % (n - 16) if n > 16 else None):  # below the weight cache's 16 points / beyond them
                if at is None:
                    continue
                e = (5 * i + (at >= 16)) % EDGES
                frames.append(("%d points, point %d of edge %d moved by %d px" % (n, at, e, d),
                               [moved(s, at, d) if j == e else s[0] for j, s in enumerate(CLEAN[n])]))
    return _batch(frames)


def batch_all_moved():
    return _batch([("every edge of %d points, point %d moved by %d px" % (n, at, d), [moved(s, at, d) for s in CLEAN[n]])
                   for n, at, d in ((40, 7, 3), (129, 100, 30))])


def test_the_clusters_are_what_they_claim_to_be():
    assert ws.K["kWCap"] == 16 and ws.K["kWE"] == EDGES and ws.K["kWPts"] == 128 and ws.K["kWPtsU"] == 240
    for n in SIZES:
        for p, normal in CLEAN[n]:
            assert len(p) == n and np.ptp(p @ normal) < 1.4143  # rounding alone: a line has every point within 0.7072 px, far inside k = 0 (1.757 px)
            for d in MOVES:  # the moved point's distance from the segment: d, bar the rounding of the move
                assert abs(np.rint(d * normal) @ normal) > d - 0.7072
            assert p.min() >= MARGIN and p[:, 0].max() < 1920 - MARGIN and p[:, 1].max() < 1080 - MARGIN
    b = batch_one_moved()
    assert len(b["frames"]) == len(MOVES) * (2 * len(SIZES) - 2)  # (11 and 16 points: no index beyond the cache)


@pytest.fixture(scope="module")
def hd(dictionary):
    """A detector whose last chunk was 32 blank 1080p frames."""
    state, fs = dictionary
    det = tk.Detector(state, fs, device=0)
    det.set_option(capi.OPT_STREAMS, 1)  # one chunk per call: the probe works on the workspace of the last chunk
    det.detect_batch(np.full((32,) + ws.HD, 255, np.uint8))
    yield det
    det.close()


ORACLE_LINES = {}  # cluster bytes -> the oracle's line, shared by the tests (the clean edges recur in every frame of (b))


def _check(det, oracle, batch, at_least):
    compared, bad = ws.probe_mismatches(det, batch, lambda c: oracle.fitline(c, True), None, ORACLE_LINES)
    assert not bad, "%d of %d lines differ from the oracle:\n%s" % (len(bad), compared, "\n".join(bad[:12]))
    assert compared >= at_least
    return compared


def test_clean_segments_every_trip_fast(hd, oracle):
    _check(hd, oracle, batch_clean(), EDGES * len(SIZES))


def test_one_moved_point_mixes_one_trip(hd, oracle):
    _check(hd, oracle, batch_one_moved(), EDGES * len(MOVES) * (2 * len(SIZES) - 2))


def test_every_edge_moved_at_the_same_index(hd, oracle):
    _check(hd, oracle, batch_all_moved(), 2 * EDGES)


def test_probe_17_on_the_device_equals_the_hosts_exp32_nonpos(hd, oracle):
    log2e = np.float32(1.44269502162933349609375)
    rng = np.random.default_rng(17)
    x = np.concatenate([-rng.uniform(0, 0.3465, 3000), -np.exp(rng.uniform(-100, -1.1, 1000))]).astype(np.float32)
    lo, hi = 0xBD800000, 0xBF000000  # the last float (by bit pattern) with x * log2e >= -0.5, by bisection
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if np.array([mid], np.uint32).view(np.float32)[0] * log2e >= np.float32(-0.5) else (lo, mid)
    edge = np.arange(lo - 63, lo + 1, dtype=np.uint32).view(np.float32)
    x = np.concatenate([x, edge, np.array([0.0, -0.0, -1e-45, -1e-38, -1.1754944e-38], np.float32)])
    assert (x * log2e >= np.float32(-0.5)).all() and (x <= 0).all() and np.rint(edge[-1] * log2e) == 0 and len(x) > 4000
    arg = x.astype(np.float64)
    want = oracle.math(tk.MATH_EXP32_NONPOS, arg, np.zeros_like(arg))
    got = hd.math(tk.MATH_EXP32_NONPOS_K0, arg)
    assert got.tobytes() == want.tobytes()
    assert hd.math(tk.MATH_EXP32_NONPOS, arg).tobytes() == want.tobytes()
