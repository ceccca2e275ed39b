"""GPU tests of the first packed boundary kernel's own packs behind a silhouette scan (-m gpu): k_prepack counts the distinct silhouette pixels of every
packed component that has a cluster-pool slot (ntotal: where the kernel's traversal stops, hence all its boundary list and stack can hold), ranks the
components by that count and packs them by need1(w, h, ntotal) = (w + 2) + (h + 2) + ntotal + (ntotal + 1), rounded up to an even word -- not by the capacity
of their boxes (pack_need), which is what k_pack knows before anything was scanned.

Every case runs batches of 8 frames of 640 x 480 (few-frame calls have no packs) twice: as they are (the label-scan branch of launch_quad_edges) and with the
fused sweep forced (CTAG_OPT_FUSED_SWEEP = 2: the mask branch).  Every frame's DBG_CAND_QUADS and record must be the oracle's byte for byte, its flags 0, its
n_boundary the oracle's.  The mask branch must have built the lists; the label-scan branch where testkit.chunk_plan says the silhouettes come from a kernel of
their own ("prescan": at this frame size it is not -- the small configuration scans inside the kernel there unless a developer knob says otherwise -- so that pass
checks the records and that DBG_PACKS1 says no lists were built).  Where they were built, DBG_PACKS1 must hold, per frame:
  * every packed component (flags are 0: each has a slot) in exactly one pack, no other component in any;
  * at most 8 components per pack, their need1 summing to at most 2560 words (a wave's LDS at four waves per SIMD);
  * descending ntotal along the order; the packs being the greedy ones over that order;
  * ntotal = the number of distinct first / last pixels per row and per column of the shape as drawn (numpy, from the drawn mask), -1 for a component in no pack.
Shapes are drawn as half-size masks and stamped as 2 x 2 blocks, dark 30 on 200 (tests/edge_shapes.py: the threshold keeps shapes a few pixels thick as drawn);
each shape is drawn into a mask of its own, so the count is of that shape alone, and a candidate is matched to its shape by its box."""
import numpy as np
import pytest

import testkit as tk
from cylindertag_amd import capi
from test_gpu_parity import assert_same_record

pytestmark = pytest.mark.gpu

HR, HC = 240, 320          # half-size frame of 640 x 480
PACK_WORDS, PACK_MAX = 2560, 8


def need1(w, h, nt):
    return (np.asarray(w) + np.asarray(h) + 2 * np.asarray(nt) + 6) & ~1


def pack_need(w, h):
    return ((w + 1) & ~1) + 2 * h + 2 * (np.minimum(2 * (w + h), w * h) + 1) + 4


def silhouette_count(mask):
    """Distinct pixels among the first and last of every row and of every column of a shape."""
    pts = set()
    for y in np.flatnonzero(mask.any(axis=1)):
        xs = np.flatnonzero(mask[y])
        pts.update(((int(xs[0]), int(y)), (int(xs[-1]), int(y))))
    for x in np.flatnonzero(mask.any(axis=0)):
        ys = np.flatnonzero(mask[:, x])
        pts.update(((int(x), int(ys[0])), (int(x), int(ys[-1]))))
    return len(pts)


class Scene:
    """One half-size frame: every shape in a mask of its own."""

    def __init__(self):
        self.shapes = []

    def _new(self):
        self.shapes.append(np.zeros((HR, HC), bool))
        return self.shapes[-1]

    def rect(self, x, y, w, h, cut=()):
        """A filled rectangle; cut: corners (0 .. 3: top left, top right, bottom left, bottom right) left out, a pixel each."""
        m = self._new()
        m[y:y + h, x:x + w] = True
        for k in cut:
            m[y + (h - 1) * (k >> 1), x + (w - 1) * (k & 1)] = False

    def ell(self, x, y, w, h, t=1):
        """An L: a vertical stroke of h pixels and a horizontal one of w along its foot, t thick."""
        m = self._new()
        m[y:y + h, x:x + t] = True
        m[y + h - t:y + h, x:x + w] = True

    def diag(self, x, y, n, t=2, flip=False):
        """A diagonal of n steps, t pixels wide per row, in an (n + t - 1) x n box."""
        m = self._new()
        for k in range(n):
            xx = x + (n - 1 - k if flip else k)
            m[y + k, xx:xx + t] = True

    def stairs(self, x, y, steps, run, rise, t=2):
        """A staircase going down to the right: treads `run` long and t thick, risers `rise` high and t thick.  The pixels of a riser between two treads are
        their rows' first and last and head no column list: the count's second term."""
        m = self._new()
        for k in range(steps):
            m[y + k * rise:y + k * rise + t, x + k * run:x + (k + 1) * run + t] = True
            m[y + k * rise:y + (k + 1) * rise + t, x + (k + 1) * run:x + (k + 1) * run + t] = True

    def comb(self, x, y, teeth, pitch, length, t=2):
        """A comb: a spine along the top and teeth hanging from it, the last ones shorter and shorter."""
        m = self._new()
        m[y:y + t, x:x + (teeth - 1) * pitch + t] = True
        for k in range(teeth):
            m[y:y + max(length - 3 * k, t + 1), x + k * pitch:x + k * pitch + t] = True

    def canvas(self):
        c = np.zeros((HR, HC), bool)
        for m in self.shapes:
            assert not (c & m).any()
            c |= m
        return c

    def frame(self):
        return np.ascontiguousarray(np.kron(np.where(self.canvas(), 30, 200).astype(np.uint8), np.ones((2, 2), np.uint8)))

    def by_box(self):
        """{(x_min, y_min, x_max, y_max): silhouette_count} of the shapes."""
        out = {}
        for m in self.shapes:
            ys, xs = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
            box = (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))
            assert box not in out
            out[box] = silhouette_count(m)
        return out


class Packs1:
    """DBG_PACKS1 of one frame."""

    def __init__(self, a):
        a = np.asarray(a, np.int64)
        self.nc, self.built, self.np, self.nel = (int(v) for v in a[:4])
        if not self.built:
            assert len(a) == 4 and self.np == 0 and self.nel == 0
            return
        o = 4
        self.packs, o = a[o:o + self.np], o + self.np
        self.order, o = a[o:o + self.nel], o + self.nel
        self.ntotal = a[o:o + self.nc]
        assert o + self.nc == len(a)

    def members(self):
        return [self.order[int(p) & 0xFFFFFF:(int(p) & 0xFFFFFF) + (int(p) >> 24)] for p in self.packs]


def check_packs1(p, kpack, cands, counts, what):
    """p: Packs1; kpack: (order, nbig) of k_pack (DBG_PACKS); cands: the oracle's candidates; counts: Scene.by_box() or None (shapes not drawn here)."""
    order1, nbig = kpack
    packed = sorted(int(c) for c in order1[:p.nc - nbig])
    assert len(set(packed)) == len(packed), what
    w, h = cands[:, 4] - cands[:, 2] + 1, cands[:, 5] - cands[:, 3] + 1
    at = 0
    for pw, m in zip(p.packs, p.members()):
        assert (int(pw) & 0xFFFFFF) == at and 1 <= len(m) <= PACK_MAX, (what, at, len(m))  # consecutive entries of the order
        assert int(need1(w[m], h[m], p.ntotal[m]).sum()) <= PACK_WORDS, (what, p.ntotal[m])
        at += len(m)
    assert at == p.nel == len(packed), (what, at, p.nel, len(packed))
    assert sorted(p.order.tolist()) == packed, what  # each once, no other
    nt = p.ntotal[p.order]
    assert (nt >= 1).all() and (nt[:-1] >= nt[1:]).all(), (what, nt)
    assert (need1(w[p.order], h[p.order], nt) <= pack_need(w[p.order], h[p.order])).all(), what
    rest = np.setdiff1d(np.arange(p.nc), p.order)
    assert (p.ntotal[rest] == -1).all(), (what, p.ntotal[rest])
    # the packs are the greedy ones over that order: a pack closes when it holds 8 components or the next one's words do not fit
    sizes, cnt, words = [], 0, 0
    for n in need1(w[p.order], h[p.order], nt).tolist():
        if cnt and (cnt == PACK_MAX or words + n > PACK_WORDS):
            sizes.append(cnt)
            cnt = words = 0
        cnt, words = cnt + 1, words + n
    assert [len(m) for m in p.members()] == sizes + ([cnt] if cnt else []), what
    if counts is not None:
        for c in p.order.tolist():
            box = tuple(int(v) for v in cands[c, 2:6])
            assert box in counts, (what, box)  # the component is the shape as drawn
            assert int(p.ntotal[c]) == counts[box], (what, box, int(p.ntotal[c]), counts[box])


def _run(det, oracle, dictionary, scenes, what, frames=None):
    """The batch through both branches; returns ({frame: Packs1} of the mask pass, the oracle's outputs, {frame: Packs1} of the label-scan pass).  scenes: a Scene per frame (or None with `frames`)."""
    state, fs = dictionary
    frames = np.ascontiguousarray(np.stack([s.frame() for s in scenes]) if frames is None else frames)
    want = [oracle.detect(f, state, fs) for f in frames]
    counts = [s.by_box() if s is not None else None for s in scenes]
    out = {}
    for fused in (1, 2):
        det.set_option(capi.OPT_FUSED_SWEEP, fused)
        try:
            got = det.detect_batch(frames)
            must = fused == 2 or bool(tk.chunk_plan(frames.shape[1], frames.shape[2], len(frames), fuse_mode=fused)["prescan"])
            packs = {}
            for f in range(len(frames)):
                o = want[f]
                tag = "%s, %s branch, frame %d" % (what, "mask" if fused == 2 else "label-scan", f)
                assert det.debug(f, tk.DBG_CAND_QUADS).tobytes() == o["candidate_quads"].tobytes(), tag + ": candidate quads"
                assert_same_record(got[f], o["result"], tag)
                assert got[f]["flags"] == 0, tag
                a = np.asarray(det.debug(f, tk.DBG_PACKS), np.int64)  # nc, np1, nbig, np2, nel | packs1 | packs2 | order1 | order2 | n_boundary
                nc, np1, nbig, np2, nel = (int(v) for v in a[:5])
                assert nc == len(o["candidates"]) and (a[5 + np1 + np2 + nc + nel:] == o["candidates"][:, 7]).all(), tag + ": n_boundary"
                p = Packs1(det.debug(f, tk.DBG_PACKS1))
                assert p.nc == nc and (p.built or not must), (tag, p.built)  # (a developer knob may send the label-scan branch through a scan kernel as well)
                if p.built:
                    check_packs1(p, (a[5 + np1 + np2:5 + np1 + np2 + nc], nbig), o["candidates"], counts[f], tag)
                packs[f] = p
        finally:
            det.set_option(capi.OPT_FUSED_SWEEP, 1)
        out[fused] = packs
    return out[2], want, out[1]


def _count_scenes():
    """Frames of 0, 1, 8, 9 and more than 20 packable components, 5 x 6 blobs to the largest box that packs."""
    scenes = []
    for k, n in enumerate((0, 1, 8, 9)):
        s = Scene()
        for i in range(n):
            s.rect(12 + 34 * i, 14 + 9 * k, 6 + 2 * (i % 3), 5 + (i % 2))
        scenes.append(s)
    s = Scene()   # 24 components: the largest L (alone in the longest pack: its need1 leaves room for the bars), long thin bars, diagonals, blobs
    s.ell(10, 30, 300, 175)
    for i in range(5):
        s.rect(20, 40 + 14 * i, 160 + 20 * i, 3)
    for i in range(6):
        s.diag(30 + 45 * i, 120, 40, flip=i % 2 == 1)
    for i in range(12):
        s.rect(24 + 22 * i, 182, 6 + i % 4, 5 + i % 3)
    scenes.append(s)
    s = Scene()   # the largest L alone
    s.ell(10, 30, 300, 175)
    scenes.append(s)
    s = Scene()   # 20 solid bars of 90 x 3: ntotal = 2 (w + h) - 4 = 182, one short of capacity
    for i in range(20):
        s.rect(10 + 100 * (i % 3), 10 + 10 * (i // 3), 90, 3)
    scenes.append(s)
    s = Scene()   # a 5 x 6 blob next to shapes at capacity (solid bars) and Ls far below it
    s.rect(8, 8, 5, 6)
    for i in range(7):
        s.rect(20, 20 + 12 * i, 120 + 20 * i, 3)   # (up to 240 x 3: the reference drops components of more than 768 pixels here)
    for i in range(4):
        s.ell(10 + 70 * i, 120, 60, 60, t=2)
    scenes.append(s)
    return scenes


def test_counts_and_sizes(detector, oracle, dictionary):
    scenes = _count_scenes()
    packs, want, other = _run(detector, oracle, dictionary, scenes, "counts")
    for f, n in enumerate((0, 1, 8, 9)):
        assert len(want[f]["candidates"]) == n and packs[f].nel == n and packs[f].np == (n + 7) // 8, (f, n)
    for f in (4, 5):
        c = want[f]["candidates"]
        w, h = c[:, 4] - c[:, 2] + 1, c[:, 5] - c[:, 3] + 1
        big = int(np.argmax(pack_need(w, h)))
        assert len(c) == (24 if f == 4 else 1) and pack_need(w, h).max() == 2556  # the largest box that packs is there
        # The mask kernel holds a component's own pixels as h rows of (w + 31) / 32 + 1 words, 512 at most: the L is a whole-wave component behind it and in
        # no pack.  Behind the scan kernel it is packed: w + h - 1 distinct silhouette pixels, need1 = 3 (w + h) + 4 words where its box reserved 2556
        assert packs[f].nel == len(c) - 1 and packs[f].ntotal[big] == -1
        if other[f].built:
            assert other[f].nel == len(c) and other[f].ntotal[big] == 300 + 175 - 1 and need1(300, 175, 474) == 1428
    c = want[6]["candidates"]
    assert len(c) == 20 and (packs[6].ntotal == 182).all() and (c[:, 7] == 182).all()
    # 20 bars of 90 x 3: pack_need 474 -> 5 a pack; need1 = (93 + 364 + 6) & ~1 = 462 -> 5 a pack as well: at capacity nothing is gained
    assert [len(m) for m in packs[6].members()] == [5, 5, 5, 5]
    assert len(want[7]["candidates"]) == 12 and packs[7].ntotal.min() == 2 * (5 + 6) - 4


def _fit_scene(widths):
    """Rectangles 10 rows high without their four corner pixels: w + h = s, ntotal = 2 s - 8, need1 = (5 s - 10) & ~1."""
    s = Scene()
    for i, w in enumerate(widths):
        s.rect(10 + 150 * (i % 2), 10 + 20 * (i // 2), w, 10, cut=(0, 1, 2, 3))
    return s


def test_exact_fit(detector, oracle, dictionary):
    """Eight shapes of w + h = 66 and 124 silhouette pixels: need1 = 66 + 4 + 124 + 125 = 319 -> 320 words each, exactly 2560: one pack.  One of them a pixel
    longer (w + h = 67, 126 pixels: 324 words): 2564, a pack of 7 and a pack of 1.  (w + h even: the stack's extra word is not lost in the rounding, so a
    build that laid out a word less per component would pack the second frame into one pack.)"""
    exact, over = _fit_scene([56] * 8), _fit_scene([57] + [56] * 7)
    packs, want, other = _run(detector, oracle, dictionary, [exact, over] * 4, "exact fit")
    for f in range(8):
        nt = np.sort(packs[f].ntotal)[::-1]
        assert nt.tolist() == ([124] * 8 if f % 2 == 0 else [126] + [124] * 7), (f, nt)
        c = want[f]["candidates"]
        assert int(need1(c[:, 4] - c[:, 2] + 1, c[:, 5] - c[:, 3] + 1, packs[f].ntotal).sum()) == (2560 if f % 2 == 0 else 2564)
        assert [len(m) for m in packs[f].members()] == ([8] if f % 2 == 0 else [7, 1]), f


def test_silhouette_far_below_capacity(detector, oracle, dictionary):
    """Thin diagonals in 60 x 60 boxes (capacity 241 points, a silhouette of half that), staircases and combs -- whose risers and teeth are row ends that head
    no column list, the count's second term -- beside bars three pixels high, within a point of their capacity."""
    scenes = []
    for k in range(8):
        s = Scene()
        for i in range(5):
            s.diag(8 + 62 * i, 8, 58 - (i + k) % 3, t=1 + (i + k) % 2, flip=(i + k) % 2 == 0)
        s.stairs(8, 74, 6 + k % 3, 7, 6, t=2)
        s.stairs(90, 74, 4, 12 + k, 9, t=1 + k % 2)
        s.comb(170, 74, 6, 9 + k % 2, 30, t=2)
        s.comb(250, 74, 4, 12, 40 - k, t=2)
        for i in range(6):
            s.rect(10 + (k % 5), 142 + 9 * i, 60 + 22 * i, 3)
        scenes.append(s)
    packs, want, other = _run(detector, oracle, dictionary, scenes, "thin shapes")
    for f in range(8):
        c = want[f]["candidates"]
        w, h = c[:, 4] - c[:, 2] + 1, c[:, 5] - c[:, 3] + 1
        cap = np.minimum(2 * (w + h), w * h) + 1
        nt = packs[f].ntotal
        assert len(c) == 15 and (2 * nt < cap).sum() >= 5 and (nt + 8 >= cap).sum() >= 6, (f, nt, cap)
        # the second term is there: these shapes have more silhouette pixels than two per column
        assert (nt > 2 * w).sum() >= 2, (f, nt, w)
        assert packs[f].np < _kpack_packs(detector, f), f


def _kpack_packs(det, f):
    """k_pack's pack count of frame f of the last batch (DBG_PACKS)."""
    return int(det.debug(f, tk.DBG_PACKS)[1])


def test_reference_shapes_at_1920x1200(detector, oracle, dictionary, test_bmp):
    """The reference's own frame (and the frame shifted by three columns), repeated to a batch of 8: its shapes in the small configuration."""
    frames = np.stack([np.roll(test_bmp, 3 * (k % 2), axis=1) for k in range(8)])
    packs, want, other = _run(detector, oracle, dictionary, [None] * 8, "test.bmp", frames=frames)
    assert packs[0].nel > 8
