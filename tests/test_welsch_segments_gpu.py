"""k_welsch's point loops as wave-uniform segments (cylindertag_amd/csrc/k_quad.hip: welsch_stops, welsch_walk): the lanes of a wave hold restarts of
edges of different lengths, a loop runs as segments between consecutive lengths -- unrolled by four with a single-step remainder -- and the lanes of an
edge leave at the segment boundary that is their length.  The weight cache's first 16 points are one more boundary.  Frames of twelve edges (one block;
in rank order the waves hold edges 0-3, 3-6, 6-9, 9-11) built from test_welsch_smallarg_gpu's clean segments so that the boundaries fall where the
loops can go wrong, through the same probe on the workspace of 32 blank 1080p frames, against `oracle.fitline`: all 16 bytes of every line.
  one step down     lengths 40, 39, .. 29: every segment after a wave's first is ONE point long
  around the cache  21, 20, .. 10 and 18, 17, 16, 16, 15, ..: the cached / uncached split falls differently for the lanes of one wave
  remainders        four frames of lengths m + 28, m + 8 and m, m = 12 .. 15: first segments [0, m) and [16, m + 8) of 0, 1, 2, 3 mod 4 trips, and [16, m + 28)
  equal lengths     twelve of 17, twelve of 40: one segment
  many lengths      twelve distinct lengths 17 .. 128, clean and rough (restarts of many edges share a wave after the regroup: more lengths than the
                    loops keep stops for), and 63 short edges of the nine lengths 2 .. 10 beside them (a lane each: nine lengths in one wave)
  other modes       the descending frame under a 200-point edge (packed words) and under a 300-point edge (global memory)
  slow trips        the descending frame with one point of one edge moved by 3, 12 and 60 px at an index beyond the cache -- inside the wave's first
                    segment, and in a one-point tail segment: a trip that is not fast inside the unrolled body and in a remainder, in both passes"""
import numpy as np
import pytest

import test_welsch_smallarg_gpu as sm
import testkit as tk
import welsch_shapes as ws
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

EDGES = sm.EDGES
DESCENDING = tuple(range(40, 28, -1))
AROUND_CACHE = (tuple(range(21, 9, -1)), (18, 17, 16, 16, 15, 14, 14, 13, 12, 12, 11, 11))
MANY = (17, 27, 37, 47, 57, 67, 78, 88, 98, 108, 118, 128)
MOVES = (3, 12, 60)
MOVED_AT = ((0, 20), (0, 39), (5, 34))  # (edge in rank order, point): inside wave 0's first uncached segment [16, 37); alone in [39, 40); edge 5 with edges 3, 4 in [34, 35)


def _frames():
    rng = np.random.default_rng(20241020)
    seg = lambda n: sm.clean_segment(rng, n)
    frames = [("one step down", [seg(n)[0] for n in DESCENDING])]
    frames += [("around the cache %d" % i, [seg(n)[0] for n in lens]) for i, lens in enumerate(AROUND_CACHE)]
    frames += [("remainders m = %d" % m, [seg(n)[0] for n in (m + 28,) * 4 + (m + 8,) * 4 + (m,) * 4]) for m in (12, 13, 14, 15)]
    frames += [("twelve of %d" % n, [seg(n)[0] for _ in range(EDGES)]) for n in (17, 40)]
    frames.append(("many lengths, clean", [seg(n)[0] for n in MANY]))
    frames.append(("many lengths, rough", [ws.segment(rng, n) for n in MANY]))
    frames.append(("nine short lengths in a wave", [seg(n)[0] for n in DESCENDING] + [seg(n)[0] for n in range(2, 11) for _ in range(7)]))
    for leader in (200, 300):
        frames.append(("descending under a %d-point edge" % leader, [seg(leader)[0]] + [seg(n)[0] for n in DESCENDING[:-1]]))
    base = [seg(n) for n in DESCENDING]
    for d in MOVES:
        for e, at in MOVED_AT:
            frames.append(("descending, point %d of edge %d moved by %d px" % (at, e, d), [sm.moved(s, at, d) if j == e else s[0] for j, s in enumerate(base)]))
    return frames, base


FRAMES, BASE = _frames()


def test_the_frames_are_what_they_claim_to_be():
    assert ws.K["kWCap"] == 16 and ws.K["kWE"] == EDGES and ws.K["kWShort"] == 10 and ws.K["kWPts"] == 128 and ws.K["kWPtsU"] == 240
    assert len(FRAMES) == 1 + 2 + 4 + 2 + 3 + 2 + 9 <= 32  # one call
    lens = {name: sorted((len(c) for c in f), reverse=True) for name, f in FRAMES}
    assert lens["one step down"] == list(DESCENDING) and all(a - b == 1 for a, b in zip(DESCENDING, DESCENDING[1:]))
    assert [min(n, 16) for n in lens["around the cache 0"]].count(16) == 6 and lens["around the cache 1"].count(16) == 2
    for m in (12, 13, 14, 15):
        assert lens["remainders m = %d" % m][3::4] == [m + 28, m + 8, m] and m % 4 == (m + 8 - 16) % 4 == m - 12
    assert len(set(lens["many lengths, clean"])) == 12 and lens["many lengths, clean"][0] == ws.K["kWPts"] and lens["many lengths, rough"] == lens["many lengths, clean"]
    short = [n for n in lens["nine short lengths in a wave"] if n <= ws.K["kWShort"]]
    assert len(set(short[:64])) == 9 and len(short) == 63  # the first wave of short edges holds all nine lengths
    assert lens["descending under a 200-point edge"][0] == 200 > ws.K["kWPts"] and lens["descending under a 300-point edge"][0] == 300 > ws.K["kWPtsU"]
    for e, at in MOVED_AT:  # beyond the cache, on the edge; the tail points are the last of their edge
        assert 16 <= at < DESCENDING[e]
    assert DESCENDING[0] - 1 == 39 and DESCENDING[5] - 1 == 34 and 20 < DESCENDING[3]
    for p, normal in BASE:
        assert np.ptp(p @ normal) < 1.4143
        for d in MOVES:
            assert abs(np.rint(d * normal) @ normal) > d - 0.7072 > 1.76  # off the line by more than the distance at which a weight's k is 0
    for _, f in FRAMES:
        for c in f:
            assert c.min() >= 0 and c[:, 0].max() < 1920 and c[:, 1].max() < 1080


@pytest.fixture(scope="module")
def hd(dictionary):
    """A detector whose last chunk was 32 blank 1080p frames."""
    state, fs = dictionary
    det = tk.Detector(state, fs, device=0)
    det.set_option(capi.OPT_STREAMS, 1)  # one chunk per call: the probe works on the workspace of the last chunk
    det.detect_batch(np.full((32,) + ws.HD, 255, np.uint8))
    yield det
    det.close()


def test_every_line_of_every_frame(hd, oracle):
    batch = sm._batch(FRAMES)
    compared, bad = ws.probe_mismatches(hd, batch, lambda c: oracle.fitline(c, True), None, sm.ORACLE_LINES)
    assert not bad, "%d of %d lines differ from the oracle:\n%s" % (len(bad), compared, "\n".join(bad[:12]))
    assert compared == sum(len(f) for _, f in FRAMES)
