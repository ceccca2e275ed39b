"""The Welsch line fits (`k_line_sort` + `k_welsch`, `k_welsch_lat`; cylindertag_amd/csrc/k_quad.hip) driven directly through the test kit's probe
(`ctag_testkit_welsch_fit`: the launcher the detection chain itself ends its quad stage with) on the clusters of tests/welsch_shapes.py: every size
tier, staging mode, pick source, block and grid loop, sort form and data-dependent branch, each in the batch form and -- where it applies -- the
few-frame form.  Every line must equal the oracle's `ctago_fitline_welsch` in all 16 bytes; nothing is excluded.  What the clusters cover is asserted
without a GPU by tests/test_welsch_statement_cpu.py, which also holds the oracle to the independent Python statement on the same clusters.
The last test feeds the stage with the kernels' own previous stage: the clusters real frames produce, read back through CTAG_DBG_LINE_POINTS."""
import numpy as np
import pytest

import cylindertag_amd as ca
import edge_shapes as es
import testkit as tk
import welsch_shapes as ws
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu


def _blank(n, size):
    return np.full((n,) + tuple(size), 255, np.uint8)


def _detector(dictionary):
    state, fs = dictionary
    det = tk.Detector(state, fs, device=0)
    det.set_option(capi.OPT_STREAMS, 1)  # one chunk per call: the probe works on the workspace of the last chunk
    return det


@pytest.fixture(scope="module")
def hd(dictionary):
    """A detector whose last chunk was 32 blank 1080p frames."""
    det = _detector(dictionary)
    det.detect_batch(_blank(32, ws.HD))
    yield det
    det.close()


@pytest.fixture(scope="module")
def fit(oracle):
    return lambda c: oracle.fitline(c, True)


ORACLE_LINES = {}  # cluster bytes -> the oracle's line (the one reference of this module)


def _check(det, batch, fit, calls=None, at_least=1):
    compared, bad = ws.probe_mismatches(det, batch, fit, calls, ORACLE_LINES)
    assert not bad, "%d of %d lines differ from the oracle:\n%s" % (len(bad), compared, "\n".join(bad[:12]))
    assert compared >= at_least
    return compared


@pytest.mark.parametrize("form", ["batch", "few-frame"])
def test_size_edges(hd, fit, form):
    b = ws.size_edges()
    calls = [c for c in b["calls"] if not c["tail"] and c["latency"] == (form == "few-frame")]
    print("size_edges, %s form: %d lines in %d calls" % (form, _check(hd, b, fit, calls, at_least=1000), len(calls)))


def test_size_edges_at_the_end_of_the_pool(dictionary, fit):
    """A workspace of ONE frame: the frame's last cluster ends at the last element of the pool's allocation proper, and the point the fit requests past an
    edge's last is the allocation's pad."""
    det = _detector(dictionary)
    try:
        det.detect_batch(_blank(1, ws.HD))
        b = ws.size_edges()
        calls = [c for c in b["calls"] if c["tail"]]
        assert len(calls) == len(ws.SIZES)
        _check(det, b, fit, calls, at_least=4 * len(ws.SIZES))
        with pytest.raises(ca.CtagError):  # (and it IS a workspace of one frame)
            det.welsch_fit([b["frames"][0][1]] * 2)
    finally:
        det.close()


def test_block_mix(hd, fit):
    print("block_mix: %d lines" % _check(hd, ws.block_mix(), fit, at_least=20000))


def test_branch_batch(hd, fit):
    print("branch_batch: %d lines" % _check(hd, ws.branch_batch(), fit, at_least=200))


def test_sort_forms(dictionary, fit):
    """3840 x 2160: line_cap 32 512, the only batch workspace that holds more edges than k_line_sort ranks in LDS."""
    det = _detector(dictionary)
    try:
        det.detect_batch(_blank(4, ws.UHD))
        print("sort_forms: %d lines" % _check(det, ws.sort_forms(), fit, at_least=44000))
        with pytest.raises(ca.CtagError):  # more edges than line_cap
            det.welsch_fit([[ws.collinear(2, 1, 1, 1, 0)] * 32513])
    finally:
        det.close()


def test_sort_forms_full_1080p_workspace(hd, fit):
    _check(hd, ws.sort_forms_hd(), fit, at_least=8192)
    with pytest.raises(ca.CtagError):  # line_cap is 8192 there
        hd.welsch_fit([[ws.collinear(2, 1, 1, 1, 0)] * 8193])


def test_a_smaller_call_after_a_larger_one(hd, fit):
    """line_sorted, line_long and welsch_rs of the larger call stay in the workspace; the smaller one must not read them."""
    big, small = ws.block_mix(), ws.branch_batch()
    for latency in (0, 1):
        large = [c for c in big["calls"] if c["latency"] == latency][-1]
        _check(hd, big, fit, [large])
        first = dict(small["calls"][0], frames=small["calls"][0]["frames"][:2], latency=latency)
        _check(hd, small, fit, [first])
        one = dict(frames=[0], latency=latency, gx=0, gs=0, tail=False)
        _check(hd, ws.size_edges(), fit, [one])


def test_the_same_call_twice_gives_the_same_bytes(hd):
    b = ws.block_mix()
    for call in (b["calls"][1], [c for c in b["calls"] if c["latency"]][0]):
        frames = [b["frames"][i][1] for i in call["frames"]]
        a = hd.welsch_fit(frames, call["latency"], call["gx"], call["gs"])
        again = hd.welsch_fit(frames, call["latency"], call["gx"], call["gs"])
        assert a.tobytes() == again.tobytes() and np.isfinite(a).all()


def test_argument_rejections(hd):
    ok = [ws.collinear(5, 10, 10, 1, 0)]
    assert hd.welsch_fit([ok]).shape == (1, 4)
    for frames, kw in (([ok] * 33, {}),                                   # more frames than the last chunk had
                       ([ok] * 5, dict(latency=1)),                       # the few-frame form is for at most kLatencyFrames
                       ([[ok[0][:1]]], {}),                               # an edge of one point
                       ([[np.array([[0, 0], [65536, 3]])]], {}),          # a coordinate outside 16 bits
                       ([[np.array([[0, -1], [6, 3]])]], {}),
                       ([[ws.collinear(2, 1, 1, 1, 0)] * 8193], {}),      # more edges than line_cap
                       ([[np.zeros((262145, 2), np.int32)]], {}),         # more points than cl_cap
                       ([[np.zeros((200000, 2), np.int32)] * 2], {}),
                       ([ok], dict(welsch_gx=-1))):
        with pytest.raises(ca.CtagError) as e:
            hd.welsch_fit(frames, **kw)
        assert e.value.status == -1  # CTAG_ERR_ARG
    assert hd.welsch_fit([ok] * 4, latency=1).shape == (4, 4) and hd.welsch_fit([[np.zeros((262144, 2), np.int32)]]).shape == (1, 4)


def _tier(n):
    for hi, name in ((ws.K["kWShort"], "<= 10: a lane each"), (ws.K["kWCap"], "11-16: every weight cached"), (ws.K["kWPts"], "17-128: float pairs"),
                     (ws.K["kWPtsU"], "129-240: packed words"), (ws.K["kPickN"] - 1, "241-255: global memory, byte picks"),
                     (ws.K["kLatPoints"], "256-512: 16-bit picks"), (ws.K["kPickN2"] - 1, "513-4095: beyond the few-frame kernel")):
        if n <= hi:
            return name
    return ">= 4096: replayed RNG"


def test_real_frames_fits_equal_the_oracle_on_their_own_clusters(detector, oracle, test_bmp):
    """The stage behind the kernels' own boundary stage: every CTAG_DBG_LINE_FITS line of test.bmp alone, of a 64-frame batch of shape frames and of one
    3840 x 2160 frame is the oracle's fit of that frame's CTAG_DBG_LINE_POINTS cluster.  The histogram says which tiers such frames reach; nothing is
    asserted on it -- it is the gap the direct tests above close."""
    shapes = [f for _, f in es.shape_frames()]
    cache, hist, compared = {}, {}, 0

    def check(frame, what):
        nonlocal compared
        n = detector.debug(frame, tk.DBG_LINES)
        pts = detector.debug(frame, tk.DBG_LINE_POINTS)
        fits = detector.debug(frame, tk.DBG_LINE_FITS)
        assert len(fits) == len(n) and len(pts) == n.sum() and (n >= 2).all(), what
        blocks = ws.kernel_blocks([np.zeros((k, 2)) for k in n])
        for blk in blocks:
            top = n[blk[0]]
            mode = "float pairs" if top <= ws.K["kWPts"] else "packed words" if top <= ws.K["kWPtsU"] else "global memory"
            hist["block of %2d staged as %s" % (len(blk), mode)] = hist.get("block of %2d staged as %s" % (len(blk), mode), 0) + 1
        at = 0
        for j, k in enumerate(n):
            c = np.ascontiguousarray(pts[at:at + k])
            at += k
            key = c.tobytes()
            if key not in cache:
                cache[key] = oracle.fitline(c, True)
            hist[_tier(k)] = hist.get(_tier(k), 0) + 1
            compared += 1
            assert fits[j].tobytes() == cache[key].tobytes(), "%s, cluster %d of %d points: %s, want %s" % (what, j, k, fits[j], cache[key])

    detector.detect(test_bmp)
    check(0, "test.bmp")
    idx = [k % len(shapes) for k in range(64)]
    detector.detect_batch(np.stack([shapes[i] for i in idx]))
    for f in range(64):
        check(f, "batch frame %d" % f)
    detector.detect(es.uhd_frame(shapes[:4]))
    check(0, "uhd frame")
    print("\nWelsch fits of real frames: %d lines equal the oracle's; tiers reached:\n%s" % (compared, "\n".join("  %-50s %d" % kv for kv in sorted(hist.items()))))
    assert compared >= 1000
