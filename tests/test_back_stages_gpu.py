"""Stages a5-a10 of the HIP path (`k_features`, `k_edge_refine` / `k_edge_refine_long`, `k_markers`) against the independent
statements in `tests/marker_testlib.py` and `tests/refine_testlib.py` (-m gpu).  Each stage of the statement ("ref") is fed with the
kernels' own previous stage -- DBG_CAND_QUADS rows with has_quad -> DBG_FEATURES0 -> 1 -> 2 -> DBG_PREMARKERS (kept with
CTAG_OPT_KEEP_PREMARKERS) -> the result record -- with the bars of `test_back_stages_cpu.py`: every integer and every float of a5,
a6, a8, a9, a10 byte for byte, a7 corners within 1e-3 px, nothing excused; the byte equality with the oracle stays beside it.
The statement's answers are worked out once per distinct stage input and reused for every copy in a batch.

Through every form of the back half the default plan picks, each confirmed with `tk.chunk_plan`: refine "one" (one frame per
call, its hipGraph replay on the third identical call, and CTAG_OPT_GRAPH 0 and 1), "split_looping" (a 64-frame batch, and a
fused chunk of 1024 frames on a handle with OPT_HOST_SUBCHUNK 1024 / OPT_STREAMS 1), "split_large" (3840 x 2160, 8 frames, two of them with edges longer than
1032 px: the long-edge flag, `k_edge_refine_long`, inside a batch of ordinary frames), "none" (cornerSubPix off); at
cornerSubPixDist 0, 1, 3, 5, 8 and 9; device-resident BGR frames in the direct form; frames of more than 64 features alone and in a
batch.  The form "split" is picked only under the developer knob CTAG_REFINE_XCD (plan_chunk), never by the default plan: it is out
of scope here."""
import numpy as np
import pytest

import marker_testlib as mt
import refine_testlib as rt
import strip_shapes as ss
import cylindertag_amd as ca
import testkit as tk
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

REF_TOL_PX = 1e-3
ALL_DISTS = (0, 1, 3, 5, 8, 9)


class Checker:
    """Compares one frame of a detector's last call with the statement, stage by stage, and with the oracle's run of that frame."""

    def __init__(self, oracle, state, fs):
        mt.use_shared_math(oracle)
        self.oracle, self.state, self.fs = oracle, state, fs
        self.cache, self.oracle_runs = {}, {}
        self.features = self.markers = self.frames = 0
        self.a7_max = 0.0
        self.failed = []

    def _once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def oracle_run(self, name, img, subpix, dist):
        key = (name, subpix, dist)
        if key not in self.oracle_runs:
            self.oracle_runs[key] = self.oracle.detect(img, self.state, self.fs, subpix=subpix, subpix_dist=dist)
        return self.oracle_runs[key]

    def frame(self, det, f, record, name, img, what, subpix=True, dist=5):
        what = "%s: %s (subpix %s, dist %d)" % (what, name, subpix, dist)
        o = self.oracle_run(name, img, subpix, dist)
        self.frames += 1

        def same(stage, got, want_statement, want_oracle):
            if np.asarray(got).tobytes() != np.asarray(want_statement).tobytes():
                self.failed.append("%s %s differs from the statement" % (what, stage))
            if np.asarray(got).tobytes() != np.asarray(want_oracle).tobytes():
                self.failed.append("%s %s differs from the oracle" % (what, stage))

        cand = det.debug(f, tk.DBG_CANDIDATES)
        quads = det.debug(f, tk.DBG_CAND_QUADS)[cand[:, 5] == 1]
        assert quads.tobytes() == o["quads"].tobytes(), what
        if record["status"] != o["status"]:
            self.failed.append("%s status %d, the oracle's %d" % (what, record["status"], o["status"]))
            return
        if o["status"] == mt.NO_CORNER:
            assert len(quads) == 0
            return
        k0 = det.debug(f, tk.DBG_FEATURES0)
        same("a5", k0, self._once(("a5", quads.tobytes()), lambda: mt.recover_features(quads, "ref")[0]), o["features"][0])
        assert (len(k0) < self.fs) == (record["status"] == mt.NO_FEATURE), what
        if record["status"] != mt.OK:
            return
        k1, k2 = det.debug(f, tk.DBG_FEATURES1), det.debug(f, tk.DBG_FEATURES2)
        same("a6", k1, self._once(("a6", k0.tobytes()), lambda: mt.obtain_corners(k0, "ref")), o["features"][1])
        if subpix:
            want = self._once(("a7", name, k1.tobytes(), dist), lambda: rt.refine_features(img, k1, dist, "ref"))
            d = np.abs(k2.astype(np.float64) - want)
            self.a7_max = max(self.a7_max, float(d.max()))
            if d[:, :16].max() > REF_TOL_PX or d[:, 16:].max() != 0:
                self.failed.append("%s a7: corners %.2e px off the statement's" % (what, d.max()))
            if k2.tobytes() != o["features"][2].tobytes():
                self.failed.append("%s a7 differs from the oracle" % what)
        else:
            assert k2.tobytes() == k1.tobytes(), what
        pre = det.debug(f, tk.DBG_PREMARKERS)
        same("a8 + a9", pre, self._once(("a8", k2.tobytes()), lambda: mt.organize_markers(k2, "ref")), o["premarkers"])
        same("a10", record, self._once(("a10", pre.tobytes()), lambda: mt.decode_markers(pre, self.state, self.fs, "ref")), o["result"])
        self.features += len(k0)
        self.markers += int(pre["n_markers"])

    def report(self):
        return "%d frames, %d features, %d markers before decoding; largest a7 corner difference to the statement %.2e px; %d misses" % (
            self.frames, self.features, self.markers, self.a7_max, len(self.failed))

    def check(self):
        assert not self.failed, "%d misses:\n%s" % (len(self.failed), "\n".join(self.failed[:40]))


def _plan(want, **args):
    plan = tk.chunk_plan(**args)
    assert {k: plan[k] for k in want} == want, (args, plan)
    return "%s: %s" % (", ".join("%s=%s" % kv for kv in args.items()), ", ".join("%s=%s" % kv for kv in want.items()))


@pytest.fixture(scope="module")
def strips(dictionary):
    state, _ = dictionary
    return {name: img for name, img, _ in ss.strip_frames_tagged(state)}


@pytest.fixture()
def keeping(detector):
    detector.set_option(capi.OPT_KEEP_PREMARKERS, 1)
    yield detector
    detector.set_option(capi.OPT_KEEP_PREMARKERS, 0)


def _uhd(strips, names):
    """Strip frames side by side on a 3840 x 2160 ground."""
    out = np.full((2160, 3840), ss.GROUND, np.uint8)
    for k, n in enumerate(names):
        out[(k // 3) * ss.ROWS:(k // 3 + 1) * ss.ROWS, (k % 3) * ss.COLS:(k % 3 + 1) * ss.COLS] = strips[n]
    return out


def test_one_frame_per_call_and_graph_replay(keeping, oracle, dictionary, strips):
    det, (state, fs) = keeping, dictionary
    c = Checker(oracle, state, fs)
    forms = [_plan(dict(refine="one", latency=1), rows=ss.ROWS, cols=ss.COLS, nframes=1),
             _plan(dict(refine="one", latency=1), rows=2160, cols=3840, nframes=1),
             _plan(dict(refine="none", latency=1), rows=ss.ROWS, cols=ss.COLS, nframes=1, corner_subpix=0)]
    for name, img in strips.items():
        for dist in (ALL_DISTS if name in ("borders", "carry", "long_edges") else (5,)):
            for call in range(3):  # the third identical call replays the captured graph (CTAG_OPT_GRAPH 2: calls of up to 4 frames)
                rec = det.detect(img, subpix_dist=dist)
                if call != 1:
                    c.frame(det, 0, rec, name, img, "alone, call %d" % call, True, dist)
        for call in range(3):
            rec = det.detect(img, subpix=False)
        c.frame(det, 0, rec, name, img, "alone, cornerSubPix off, call 2", False, 5)
    # No debug view tells a replayed graph from direct launches (and a capture that fails falls back to them silently), so the replay
    # above is what the library's rule promises, not something observed.  Hence both settings that leave no choice: never a graph, and a
    # graph for every chunk (captured on the first call, replayed on the next two), one frame and a 12-frame batch.
    names = [n for n in strips if n != "long_edges"]
    batch = np.stack([strips[names[k % len(names)]] for k in range(12)])
    try:
        for mode in (0, 1):
            det.set_option(capi.OPT_GRAPH, mode)
            for call in range(3):
                for name in ("carry", "pairs", "fan"):
                    c.frame(det, 0, det.detect(strips[name]), name, strips[name], "alone, CTAG_OPT_GRAPH %d, call %d" % (mode, call))
                got = det.detect_batch(batch)
            for f in range(12):
                n = names[f % len(names)]
                c.frame(det, f, got[f], n, strips[n], "batch 12, CTAG_OPT_GRAPH %d, call 2, frame %d" % (mode, f))
    finally:
        det.set_option(capi.OPT_GRAPH, 2)
    print("\nstages a5-a10, one frame per call (plan forms: %s): %s" % ("; ".join(forms), c.report()))
    c.check()
    assert c.features >= 500


def test_batches_match_statement(keeping, oracle, dictionary, strips):
    det, (state, fs) = keeping, dictionary
    c = Checker(oracle, state, fs)
    names = [n for n in strips if n != "long_edges"]
    forms = [_plan(dict(refine="split_looping", latency=0), rows=ss.ROWS, cols=ss.COLS, nframes=64)]
    idx = [k % len(names) for k in range(64)]
    got = det.detect_batch(np.stack([strips[names[i]] for i in idx]))
    for f, i in enumerate(idx):
        c.frame(det, f, got[f], names[i], strips[names[i]], "batch 64 frame %d" % f)
    forms.append(_plan(dict(refine="split_looping", latency=0), rows=ss.ROWS, cols=ss.COLS, nframes=12))
    batch = np.stack([strips[names[k % len(names)]] for k in range(12)])
    for dist in (0, 1, 3, 8, 9):
        got = det.detect_batch(batch, subpix_dist=dist)
        for f in range(12):
            n = names[f % len(names)]
            c.frame(det, f, got[f], n, strips[n], "batch 12 frame %d" % f, True, dist)
    forms.append(_plan(dict(refine="none", latency=0), rows=ss.ROWS, cols=ss.COLS, nframes=12, corner_subpix=0))
    got = det.detect_batch(batch, subpix=False)
    for f in range(12):
        n = names[f % len(names)]
        c.frame(det, f, got[f], n, strips[n], "batch 12 frame %d" % f, False, 5)
    print("\nstages a5-a10, batches (plan forms: %s): %s" % ("; ".join(forms), c.report()))
    c.check()
    assert c.features >= 3000 and c.markers >= 300


def test_4k_batch_with_a_long_edge_frame(keeping, oracle, dictionary, strips):
    """3840 x 2160, eight frames: the large split form, and among ordinary frames two whose feature edges exceed 1032 px (the
    long-edge flag: k_edge_refine_long).  That the long form did the work is inferred from the data -- the oracle's stage 1 holds an
    edge above 1032 px, which is what sets the flag -- no probe of the library confirms which kernel ran."""
    det, (state, fs) = keeping, dictionary
    c = Checker(oracle, state, fs)
    form = _plan(dict(refine="split_large", latency=0), rows=2160, cols=3840, nframes=8)
    frames = {"uhd a": _uhd(strips, ("carry", "codes", "angles")), "uhd b": _uhd(strips, ("pairs", "borders", "angles")),
              "long_edges": strips["long_edges"]}
    order = ("uhd a", "long_edges", "uhd b", "uhd a", "uhd b", "long_edges", "uhd a", "uhd b")
    for n in ("uhd a", "uhd b"):
        o = c.oracle_run(n, frames[n], True, 5)
        assert o["status"] == 0 and len(o["features"][0]) > 40, n
    o = c.oracle_run("long_edges", frames["long_edges"], True, 5)
    q = o["features"][1][:, :16].reshape(-1, 2, 4, 2)
    assert np.linalg.norm(q - np.roll(q, -1, axis=2), axis=3).max() > 1032  # nsamples = max(128.0, mag / 8) above 128
    got = det.detect_batch(np.stack([frames[n] for n in order]))
    for f, n in enumerate(order):
        c.frame(det, f, got[f], n, frames[n], "4k batch frame %d" % f)
    print("\nstages a5-a10 at 3840x2160 (%s): %s" % (form, c.report()))
    c.check()


def test_more_than_64_features(keeping, oracle, dictionary, strips):
    """Frames of 65-96 features (both register halves of k_markers), alone and in a batch."""
    det, (state, fs) = keeping, dictionary
    c = Checker(oracle, state, fs)
    frames = [("many markers %d/%d" % (mk, idx), tk.synth_frame_host(state, idx, markers=mk)[0]) for mk in (6, 8) for idx in (5, 6, 7, 8)]
    form = _plan(dict(refine="split_looping", latency=0), rows=1080, cols=1920, nframes=8)
    for name, img in frames:
        assert len(c.oracle_run(name, img, True, 5)["features"][0]) > 64
        c.frame(det, 0, det.detect(img), name, img, "alone")
    got = det.detect_batch(np.stack([f for _, f in frames]))
    for f, (name, img) in enumerate(frames):
        c.frame(det, f, got[f], name, img, "batch 8 frame %d" % f)
    img = strips["many"]
    assert len(c.oracle_run("many", img, True, 5)["features"][0]) >= 65
    c.frame(det, 0, det.detect(img), "many", img, "alone")
    print("\nstages a5-a10, more than 64 features (%s): %s" % (form, c.report()))
    c.check()


def test_chunk_of_1024_and_device_bgr(oracle, dictionary, strips):
    """A handle of its own: one fused chunk of 1024 frames on one stream, and device-resident BGR frames in the direct form (a7 reads the
    pixels of a frame that has no gray copy)."""
    import torch
    state, fs = dictionary
    c = Checker(oracle, state, fs)
    own = tk.Detector(state, fs, device=0)
    try:
        own.set_option(capi.OPT_KEEP_PREMARKERS, 1)
        own.set_option(capi.OPT_HOST_SUBCHUNK, 1024)
        own.set_option(capi.OPT_STREAMS, 1)
        # 1280 columns (the strip frames with 128 columns of ground to their right): a size the fused sweep takes
        wide = {n + " wide": np.pad(f, ((0, 0), (0, 1280 - ss.COLS)), constant_values=ss.GROUND) for n, f in strips.items() if n != "long_edges"}
        names = list(wide)
        forms = [_plan(dict(refine="split_looping", fused=1, latency=0), rows=ss.ROWS, cols=1280, nframes=1024)]
        idx = [(k * 5) % len(names) for k in range(1024)]
        frames = np.empty((1024, ss.ROWS, 1280), np.uint8)
        for f, i in enumerate(idx):
            frames[f] = wide[names[i]]
        got = own.detect_batch(frames)
        del frames
        for f, i in enumerate(idx):
            c.frame(own, f, got[f], names[i], wide[names[i]], "fused chunk 1024 frame %d" % f)
        own.set_option(capi.OPT_FUSED_SWEEP, 2)
        forms.append(_plan(dict(bgr_direct=1, refine="split_looping"), rows=1080, cols=1920, nframes=64, channels=3, fuse_mode=2))
        synth = [("synthetic %d" % f, tk.synth_frame_host(state, f)[0]) for f in range(8)]
        idx = [(k * 3) % 8 for k in range(64)]
        dev = torch.from_numpy(np.stack([np.repeat(synth[i][1][:, :, None], 3, axis=2) for i in idx])).cuda()
        out = torch.zeros((64, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        own.detect_batch_bgr_device(dev.data_ptr(), 64, 1080, 1920, 1920 * 3, 1080 * 1920 * 3, out.data_ptr())
        own.sync()
        with pytest.raises(ca.CtagError):
            own.debug(0, tk.DBG_GRAY)  # the direct form: no gray image was written
        got = np.frombuffer(out.cpu().numpy().tobytes(), ca.RESULT_DT)
        for f, i in enumerate(idx):
            c.frame(own, f, got[f], synth[i][0], synth[i][1], "bgr direct 64 frame %d" % f)
        del dev, out
    finally:
        own.close()
    print("\nstages a5-a10, chunk of 1024 and device BGR (plan forms: %s): %s" % ("; ".join(forms), c.report()))
    c.check()
