"""GPU tests of the second packed boundary kernel's own packs (-m gpu): k_repack ranks the packed components by the boundary length the first kernel
traced and packs them by need2(n_boundary) = two lists of n words -- not by the capacity of their boxes, which is what the first kernel holds in LDS.

Every case runs batches of 8 frames (few-frame calls have no packs) twice: as they are (the label-scan branch of launch_quad_edges) and with the fused
sweep forced (CTAG_OPT_FUSED_SWEEP = 2: the mask branch).  Every frame's DBG_CAND_QUADS and record must be the oracle's byte for byte, and the pack lists read
back through DBG_PACKS must hold, per frame:
  * every packed component with a traced boundary, in exactly one pack; no other component in any (frames here whose flags are 0: the first kernel gives
    up on a component only for want of pool space, which raises CTAG_FLAG_POOL_OVERFLOW);
  * at most 8 components per pack, their need2 summing to at most 2560 words (a wave's LDS at four waves per SIMD);
  * descending n_boundary along the order.
Shapes are drawn as half-size masks and stamped as 2 x 2 blocks, dark 30 on 200 (tests/edge_shapes.py: the threshold keeps shapes up to two tiles thick as
drawn).  The reference keeps components of 30 pixels .. 1 % of the half-size frame (768 at 640 x 480), so the smallest blob here is 5 x 6, not 3 x 3, and
the largest box that still packs is a one-pixel L of 300 x 175 (pack_need 2556)."""
import numpy as np
import pytest

import testkit as tk
from cylindertag_amd import capi
from clutter import blob_field, chevron_texture
from test_gpu_parity import assert_same_record

pytestmark = pytest.mark.gpu

HR, HC = 240, 320          # half-size frame of 640 x 480
PACK_WORDS, PACK_MAX = 2560, 8


def need2(n):
    return 2 * ((np.asarray(n) + 1) & ~1)


def pack_need(w, h):
    return ((w + 1) & ~1) + 2 * h + 2 * (np.minimum(2 * (w + h), w * h) + 1) + 4


def _frame(canvas):
    return np.ascontiguousarray(np.kron(np.where(canvas, 30, 200).astype(np.uint8), np.ones((2, 2), np.uint8)))


def _rect(c, x, y, w, h):
    c[y:y + h, x:x + w] = True


def _ell(c, x, y, w, h, t=1):
    """An L: a vertical stroke of h pixels and a horizontal one of w along its foot, t thick."""
    c[y:y + h, x:x + t] = True
    c[y + h - t:y + h, x:x + w] = True


def _diag(c, x, y, n, t=2, flip=False):
    """A diagonal of n steps, t pixels wide per row, in an n x (n + t - 1) box."""
    for k in range(n):
        xx = x + (n - 1 - k if flip else k)
        c[y + k, xx:xx + t] = True


class Packs:
    """DBG_PACKS of one frame."""

    def __init__(self, a):
        a = np.asarray(a, np.int64)
        self.nc, self.np1, self.nbig, self.np2, self.nel = (int(v) for v in a[:5])
        o = 5
        self.packs1, o = a[o:o + self.np1], o + self.np1
        self.packs2, o = a[o:o + self.np2], o + self.np2
        self.order1, o = a[o:o + self.nc], o + self.nc
        self.order2, o = a[o:o + self.nel], o + self.nel
        self.nb = a[o:o + self.nc]
        assert o + self.nc == len(a)

    def members(self, packs, order):
        return [order[int(p) & 0xFFFFFF:(int(p) & 0xFFFFFF) + (int(p) >> 24)] for p in packs]


def check_packs(p, what):
    packed = p.order1[:p.nc - p.nbig]
    assert len(set(packed.tolist())) == len(packed), what
    eligible = sorted(int(c) for c in packed if p.nb[c] > 0)
    at = 0
    for pw, m in zip(p.packs2, p.members(p.packs2, p.order2)):
        assert (int(pw) & 0xFFFFFF) == at and 1 <= len(m) <= PACK_MAX, (what, at, len(m))  # consecutive entries of the order
        assert int(need2(p.nb[m]).sum()) <= PACK_WORDS, (what, p.nb[m])
        at += len(m)
    assert at == p.nel == len(eligible), (what, at, p.nel, len(eligible))
    assert sorted(p.order2.tolist()) == eligible, what  # each once, no other
    nb2 = p.nb[p.order2]
    assert (nb2[:-1] >= nb2[1:]).all(), (what, nb2)
    # the packs are the greedy ones over that order: a pack closes when it holds 8 components or the next one's words do not fit
    sizes, cnt, words = [], 0, 0
    for n in need2(nb2).tolist():
        if cnt and (cnt == PACK_MAX or words + n > PACK_WORDS):
            sizes.append(cnt)
            cnt = words = 0
        cnt, words = cnt + 1, words + n
    assert [len(m) for m in p.members(p.packs2, p.order2)] == sizes + ([cnt] if cnt else []), what
    # the first kernel's own packs, for comparison: by capacity
    for m in p.members(p.packs1, p.order1):
        assert 1 <= len(m) <= PACK_MAX, what


def _run(det, oracle, dictionary, frames, what, probe=None):
    """The batch through both branches; returns the Packs of every probed frame of the label-scan pass (probe: frame indices, default all)."""
    state, fs = dictionary
    frames = np.ascontiguousarray(frames)
    want = [oracle.detect(f, state, fs) for f in frames]
    out = None
    for fused in (1, 2):
        det.set_option(capi.OPT_FUSED_SWEEP, fused)
        try:
            got = det.detect_batch(frames)
            packs = {}
            for f in (range(len(frames)) if probe is None else probe):
                o = want[f]
                tag = "%s, %s branch, frame %d" % (what, "mask" if fused == 2 else "label-scan", f)
                assert det.debug(f, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes(), tag + ": candidate quads"
                assert_same_record(got[f], o["result"], tag)
                assert got[f]["flags"] == 0, tag
                p = Packs(det.debug(f, tk.DBG_PACKS))
                assert p.nc == len(o["candidates"]) and (p.nb == o["candidates"][:, 7]).all(), tag + ": n_boundary"
                check_packs(p, tag)
                packs[f] = p
        finally:
            det.set_option(capi.OPT_FUSED_SWEEP, 1)
        out = out or packs
    return out, want


def _count_frames():
    """Frames of 0, 1, 8, 9 and more than 20 packable components, 5 x 6 blobs to the largest box that packs."""
    frames = []
    for k, n in enumerate((0, 1, 8, 9)):
        c = np.zeros((HR, HC), bool)
        for i in range(n):
            _rect(c, 12 + 34 * i, 14 + 9 * k, 6 + 2 * (i % 3), 5 + (i % 2))
        frames.append(c)
    c = np.zeros((HR, HC), bool)   # 24 components: the largest L, long thin bars, diagonals, blobs
    _ell(c, 10, 30, 300, 175)
    for i in range(5):
        _rect(c, 20, 40 + 14 * i, 160 + 20 * i, 3)
    for i in range(6):
        _diag(c, 30 + 45 * i, 120, 40, flip=i % 2 == 1)
    for i in range(12):
        _rect(c, 24 + 22 * i, 182, 6 + i % 4, 5 + i % 3)
    frames.append(c)
    c = np.zeros((HR, HC), bool)   # 20 bars of 90 x 3: capacity-sized packs of 5, length-sized packs of 6 and 7
    for i in range(20):
        _rect(c, 10 + 100 * (i % 3), 10 + 10 * (i // 3), 90, 3)
    frames.append(c)
    c = np.zeros((HR, HC), bool)   # 9 Ls in 60 x 60 boxes and 16 blobs
    for i in range(9):
        _ell(c, 10 + 62 * (i % 5), 10 + 70 * (i // 5), 60, 60, t=2)
    for i in range(16):
        _rect(c, 12 + 19 * i, 160 + 8 * (i % 2), 7, 6)
    frames.append(c)
    frames.append(frames[4][::-1].copy())
    return [_frame(c) for c in frames]


def test_counts_and_sizes(detector, oracle, dictionary):
    packs, want = _run(detector, oracle, dictionary, np.stack(_count_frames()), "counts")
    for f, n in enumerate((0, 1, 8, 9)):
        assert len(want[f]["candidates"]) == n and packs[f].nel == n and packs[f].np2 == (n + 7) // 8, (f, n)
    c = want[4]["candidates"]
    w, h = c[:, 4] - c[:, 2] + 1, c[:, 5] - c[:, 3] + 1
    assert len(c) == 24 and pack_need(w, h).max() == 2556 and packs[4].nbig == 0  # the largest box that packs is there, and packed
    for f in (4, 5, 6):  # capacity-sized and length-sized packs differ in count, hence in membership
        assert len(want[f]["candidates"]) >= 20 and packs[f].np2 < packs[f].np1, (f, packs[f].np1, packs[f].np2)
    assert packs[5].np1 == 4 and packs[5].np2 == 3  # 20 bars of 90 x 3: pack_need 474 -> 5 a pack; need2(182) = 364 -> 7 a pack


def _fit_frame(widths):
    """Filled rectangles 10 rows high: the boundary of a w x 10 rectangle is its 2 (w + 10) - 4 border pixels."""
    c = np.zeros((HR, HC), bool)
    for i, w in enumerate(widths):
        _rect(c, 10 + 150 * (i % 2), 10 + 20 * (i // 2), w, 10)
    return _frame(c)


def test_exact_fit(detector, oracle, dictionary):
    """Eight boundaries of 160 points: need2 sums to exactly 2560 words, one pack.  One boundary of 162 among them: 2564, a pack of 7 and a pack of 1."""
    exact, over = _fit_frame([72] * 8), _fit_frame([73] + [72] * 7)
    frames = np.stack([exact, over] * 4)
    packs, want = _run(detector, oracle, dictionary, frames, "exact fit")
    for f in range(8):
        nb = np.sort(want[f]["candidates"][:, 7])[::-1]
        assert nb.tolist() == ([160] * 8 if f % 2 == 0 else [162] + [160] * 7), (f, nb)  # what the oracle's walk gives, as assumed
        sizes = [len(m) for m in packs[f].members(packs[f].packs2, packs[f].order2)]
        assert int(need2(nb).sum()) == (2560 if f % 2 == 0 else 2564)
        assert sizes == ([8] if f % 2 == 0 else [7, 1]), (f, sizes)


def test_boundary_far_below_capacity(detector, oracle, dictionary):
    """Thin diagonals and Ls in 60 x 60 boxes (capacity 241 points, boundaries of about half that or less) beside bars three pixels high, whose boundary
    is within a few points of their capacity."""
    frames = []
    for k in range(8):
        c = np.zeros((HR, HC), bool)
        for i in range(5):
            _diag(c, 8 + 62 * i, 8, 58 - (i + k) % 3, t=1 + (i + k) % 2, flip=(i + k) % 2 == 0)
            _ell(c, 8 + 62 * i, 74, 60 - (k % 4), 60 - i, t=1 + i % 2)
        for i in range(9):
            _rect(c, 10 + (k % 5), 142 + 9 * i, 60 + 22 * i, 3)
        frames.append(_frame(c))
    packs, want = _run(detector, oracle, dictionary, np.stack(frames), "thin shapes")
    for f in range(8):
        c = want[f]["candidates"]
        w, h = c[:, 4] - c[:, 2] + 1, c[:, 5] - c[:, 3] + 1
        cap = np.minimum(2 * (w + h), w * h) + 1
        assert len(c) == 19 and (2 * c[:, 7] < cap).sum() >= 5 and (c[:, 7] + 8 >= cap).sum() >= 9, (f, c[:, 7], cap)
        assert packs[f].np2 < packs[f].np1, (f, packs[f].np1, packs[f].np2)


def test_components_the_first_kernel_gave_up_on(detector, oracle, dictionary):
    """A chevron texture exhausts the batch workspace's cluster pool: the first kernel gives up on the components it has no slot for (they enter no pack),
    the frame is flagged and run again alone, and its record is the oracle's.  A blob field of more than kLdsCand = 2048 candidates that still fits
    the 1920 x 1200 batch workspace (2304 candidates) takes k_pack's and k_repack's counting-sort path; a denser one overflows the candidate pool."""
    state, fs = dictionary
    frames = np.stack([tk.synth_frame_host(state, 700 + f, rows=1200, cols=1920)[0] for f in range(8)])
    frames[1] = chevron_texture(frames[1])[0]
    frames[3] = blob_field(frames[3])[0]
    frames[6], n_blobs = blob_field(np.full((1200, 1920), 200, np.uint8), pitch_x=34, pitch_y=29)
    want, _ = oracle.detect_many(frames, state, fs)
    o6 = oracle.detect(frames[6], state, fs)
    assert 2048 < len(o6["candidates"]) <= 2304, (n_blobs, len(o6["candidates"]))
    for fused in (1, 2):
        detector.set_option(capi.OPT_FUSED_SWEEP, fused)
        try:
            before = detector.counters()["reruns"]
            got = detector.detect_batch(frames)
            assert detector.counters()["reruns"] == before + 2  # the texture and the dense field; not the 2048+ field
            for f in range(8):
                assert_same_record(got[f], want[f], "give-up batch, fused %d, frame %d" % (fused, f))
            # the 2048+ field in a batch without reruns (they replace what the probes look at)
            few = np.stack([frames[6], frames[0], frames[6], frames[2], frames[6], frames[4], frames[5], frames[7]])
            got = detector.detect_batch(few)
            for f in (0, 2, 4):
                assert detector.debug(f, tk.DBG_CAND_QUADS).tobytes() == o6["candidate_quads"].tobytes(), (fused, f)
                assert_same_record(got[f], o6["result"], "2048+ field, fused %d, frame %d" % (fused, f))
                p = Packs(detector.debug(f, tk.DBG_PACKS))
                assert p.nc == len(o6["candidates"]) > 2048 and p.nbig == 0 and (p.nb == o6["candidates"][:, 7]).all()
                check_packs(p, "2048+ field, fused %d, frame %d" % (fused, f))
        finally:
            detector.set_option(capi.OPT_FUSED_SWEEP, 1)


def test_reference_shapes_at_1920x1200(detector, oracle, dictionary, test_bmp):
    """The reference's own frame (and the frame shifted by three columns), repeated to a batch of 8: its shapes in the small configuration."""
    frames = np.stack([np.roll(test_bmp, 3 * (k % 2), axis=1) for k in range(8)])
    packs, want = _run(detector, oracle, dictionary, frames, "test.bmp", probe=(0, 1, 7))
    assert packs[0].nel > 8 and packs[0].np2 <= packs[0].np1
