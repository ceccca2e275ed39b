"""Stages a0-a3 of the HIP path (`k_sweep.hip`: BGR2GRAY, decimation, adaptive threshold, labelling, candidate list) against the
independent statement in `tests/front_testlib.py` alone (-m gpu), on the frames of `tests/front_shapes.py` and a few marker frames,
through every decimation and labelling form the chunk plan picks without developer aids.  Every comparison is an equality:

- `DBG_HALF` = the statement's half image (in the fused forms the testkit decimates the frame again with the stand-alone kernel: the
  product there is the mask; in the direct BGR form no gray rows exist and the view is refused: asserted);
- `DBG_MASK` = `binary > 0` where the chunk took the fused sweep;
- `DBG_LABELS`: foreground equal to `binary`, and the same partition as the statement's label image;
- `DBG_CANDIDATES[:, 0:5]` (area, box) = the statement's candidate list, in order, and the candidate count;
- `DBG_GRAY` = `bgr2gray` where a gray image exists.

`tk.chunk_plan` with each call's arguments confirms the form; the byte equality with the oracle stays beside the statement.  The
statement's answers are worked out once per distinct (frame, window, parameters).  In the chunks of 256 and 1024 frames every frame's
candidate list is compared and every 16th frame's images; everywhere else every frame's images."""
import numpy as np
import pytest

import front_shapes as fs
import front_testlib as ft
import cylindertag_amd as ca
import testkit as tk
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

ROWS, COLS = fs.ROWS, fs.COLS


class Answers:
    """The statement's and the oracle's answers, once per distinct (frame, window, parameters)."""

    def __init__(self, oracle, dictionary):
        self.oracle, (self.state, self.fsz) = oracle, dictionary
        self.cache = {}

    def of(self, name, frame, tw=5, cap=0.3, area=fs.AREA_PARAMS[0]):
        key = (name, tw, cap, area)
        if key not in self.cache:
            s = ft.front(frame, tw, cap, area[0], area[1])
            default = (cap, area) == (0.3, fs.AREA_PARAMS[0])
            if not default:
                p = ca.default_params()
                p.dark_cap, p.area_min, p.area_max_fraction = cap, area[0], area[1]
                self.oracle.set_params(p)
            try:
                o = self.oracle.detect(s["gray"], self.state, self.fsz, tw)
            finally:
                self.oracle.set_params(None)
            self.cache[key] = dict(name=name, frame=frame, tw=tw, s=s, o=o)
        return self.cache[key]


class Tally:
    def __init__(self):
        self.frames = self.images = self.pixels = self.components = self.candidates = 0
        self.forms = {}   # (dec, ccl) -> plan lines

    def plan(self, want, what, **args):
        plan = tk.chunk_plan(**args)
        assert {k: plan[k] for k in want} == want, (what, args, plan)
        line = "%s [%s] -> dec=%s ccl=%s fused=%d latency=%d bgr_direct=%d" % (
            what, ", ".join("%s=%s" % (k, hex(v) if k == "frames" else v) for k, v in args.items()), plan["dec"], plan["ccl"], plan["fused"], plan["latency"],
            plan["bgr_direct"])
        self.forms.setdefault((plan["dec"], plan["ccl"]), []).append(line)
        return plan

    def report(self):
        lines = ["%d frame copies (%d with their images: %d half-size pixels, %d components), %d candidates" % (
            self.frames, self.images, self.pixels, self.components, self.candidates)]
        for (dec, ccl), runs in sorted(self.forms.items()):
            lines.append("  dec=%s ccl=%s: %d runs, e.g. %s" % (dec, ccl, len(runs), runs[0]))
        return "\n".join(lines)


def check(det, f, a, what, tally, fused, images=True, half=True):
    s, o = a["s"], a["o"]
    what = (what, a["name"], f)
    cand = det.debug(f, tk.DBG_CANDIDATES)
    assert cand.shape[0] == len(s["candidates"]), what
    assert (cand[:, 0:5] == s["candidates"][:, 1:6]).all(), what
    assert (cand[:, 0:5] == o["candidates"][:, 1:6]).all(), what  # and byte for byte the oracle's
    tally.frames += 1
    tally.candidates += len(cand)
    if not images:
        return
    shape = s["half"].shape
    if half:
        assert (det.debug(f, tk.DBG_HALF).reshape(shape) == s["half"]).all(), what
        assert (s["half"] == o["half"]).all(), what
    elif half is not None:
        with pytest.raises(ca.CtagError):
            det.debug(f, tk.DBG_HALF)
    if fused:
        assert (det.debug(f, tk.DBG_MASK).reshape(shape) == (s["binary"] > 0)).all(), what
    else:
        with pytest.raises(ca.CtagError):
            det.debug(f, tk.DBG_MASK)  # the two-kernel form: no mask exists
    lab = det.debug(f, tk.DBG_LABELS).reshape(shape)
    assert ((lab != 0) == (s["binary"] > 0)).all(), what
    assert ft.same_partition(s["labels"], lab), what
    tally.images += 1
    tally.pixels += s["half"].size
    tally.components += len(s["areas"]) - 1


def pool_1080(state, test_bmp):
    """Distinct 1080p frames that fill no component pool: the knife-edge set of the reference's cap, labelling shapes, the area limits, the
    slot-reuse pair, marker frames."""
    import edge_testlib as et
    from sequences import avi_substitute
    out = [("knife edges %d" % k, f) for k, f in enumerate(fs.knife_frames(0.3, fs.cap_edge_cells(0.3)))]
    out += [(name, f) for name, f, tw, area, tags in fs.labelling_frames() if f.shape == (ROWS, COLS) and area == fs.AREA_PARAMS[0] and "dense" not in tags]
    batch = fs.slot_reuse_batches()[1]
    out += [("slot reuse empty", batch[0]), ("slot reuse textured", batch[1])]
    out += [("synthetic %d" % k, tk.synth_frame_host(state, k)[0]) for k in range(4)]
    out.append(("random shapes 2", et.random_shapes_frame(state, 2, ROWS, COLS)))
    out.append(("sequence 0", avi_substitute(test_bmp, 1)[0]))
    return out


@pytest.fixture(scope="module")
def answers(oracle, dictionary):
    return Answers(oracle, dictionary)


@pytest.fixture(scope="module")
def pool(answers, dictionary, test_bmp):
    return [answers.of(name, f) for name, f in pool_1080(dictionary[0], test_bmp)]


@pytest.fixture(scope="module")
def tally():
    return Tally()


def test_single_frames_match_statement(detector, answers, pool, tally, test_bmp):
    """One frame per call (the latency forms): every shape frame at its window, test.bmp at every window, host BGR frames (two-step)."""
    cases = list(pool)
    cases += [answers.of(name, f, tw) for name, f, tw in fs.window_frames()]
    cases += [answers.of(name, f) for name, f, tags in fs.resize_frames()]
    cases += [answers.of(name, f, tw) for name, f, tw, area, tags in fs.labelling_frames() if area == fs.AREA_PARAMS[0]]
    cases += [answers.of("test.bmp", test_bmp, tw) for tw in (1, 2, 3, 4, 5, 6, 7, 8, 16, 31, 32)]
    statuses = set()
    for a in cases:
        rows, cols = a["frame"].shape
        tally.plan(dict(latency=1, fused=0), "one frame", rows=rows, cols=cols, nframes=1, adaptive_thresh=a["tw"])
        r = detector.detect(a["frame"], a["tw"])
        check(detector, 0, a, "alone, window %d" % a["tw"], tally, fused=False)
        statuses.add(int(r["status"]))
        hr, hc = a["s"]["half"].shape
        if min(-(-hr // a["tw"]), -(-hc // a["tw"])) < 3:
            assert r["status"] == 1 and not a["s"]["binary"].any(), a["name"]
    assert {0, 1, 2} <= statuses
    # host BGR frames: k_bgr2gray into a gray image, then the gray chain of one frame
    tally.plan(dict(latency=1, fused=0), "host BGR, two-step", rows=1200, cols=1920, nframes=1, channels=1)
    for name, bgr, tw in (("coloured test.bmp", fs.colourise(test_bmp, 1), 5), ("primaries and grays", fs.primaries(), 3),
                          ("coloured labelling shapes", fs.colourise(fs.double(fs.labelling_design(3)), 2), 5)):
        a = answers.of(name, bgr, tw)
        detector.detect_bgr(bgr, tw)
        assert (detector.debug(0, tk.DBG_GRAY).reshape(a["s"]["gray"].shape) == a["s"]["gray"]).all(), name
        check(detector, 0, a, "host bgr", tally, fused=False)


def test_batches_match_statement(detector, answers, pool, tally):
    """Batches through the shared handle: 64 frames at 1080p, small and large windows, odd sizes, the slot-reuse sequence."""
    n = len(pool)
    tally.plan(dict(latency=0, fused=0, dec="banded", ccl="tw5"), "64 frames", rows=ROWS, cols=COLS, nframes=64)
    idx = [k % n for k in range(64)]
    detector.detect_batch(np.stack([pool[i]["frame"] for i in idx]))
    for f, i in enumerate(idx):
        check(detector, f, pool[i], "batch 64", tally, fused=False)
    # odd sizes in a batch: the general decimation
    tally.plan(dict(latency=0, fused=0, dec="general", ccl="tw5"), "64 odd frames", rows=ROWS - 1, cols=COLS - 1, nframes=64)
    odd = [answers.of(a["name"] + " cropped odd", np.ascontiguousarray(a["frame"][1:, 1:])) for a in pool[::2]]
    idx = [k % len(odd) for k in range(64)]
    detector.detect_batch(np.stack([odd[i]["frame"] for i in idx]))
    for f, i in enumerate(idx):
        check(detector, f, odd[i], "batch 64 odd", tally, fused=False)
    # the other windows in batches of 16: variants of each window's ragged frame
    frames = {tw: f for name, f, tw in fs.window_frames() if "ragged" in name}
    for tw in (1, 2, 3, 7, 32):
        rows, cols = frames[tw].shape
        tally.plan(dict(latency=0, fused=0, ccl="any"), "16 frames, window %d" % tw, rows=rows, cols=cols, nframes=16, adaptive_thresh=tw)
        variants = [answers.of("window %d variant %d" % (tw, k), np.ascontiguousarray(np.roll(frames[tw], (3 * k, 5 * k), (0, 1))), tw) for k in range(4)]
        idx = [k % 4 for k in range(16)]
        detector.detect_batch(np.stack([variants[i]["frame"] for i in idx]), tw)
        for f, i in enumerate(idx):
            check(detector, f, variants[i], "batch 16, window %d" % tw, tally, fused=False)
    # slot reuse: textured and nearly empty frames alternate on the same workspace slots, then shifted copies
    tally.plan(dict(latency=0, fused=0), "slot reuse, 8 frames a call", rows=ROWS, cols=COLS, nframes=8)
    for b, batch in enumerate(fs.slot_reuse_batches()):
        a = [answers.of("slot reuse batch %d frame %d" % (b, k), batch[k]) for k in (0, 1)]
        detector.detect_batch(batch)
        for f in range(len(batch)):
            want = a[0] if (batch[f] == batch[0]).all() else a[1]
            check(detector, f, want, "slot reuse batch %d" % b, tally, fused=False)


def _device_run(det, frames, tw=5, row_stride=None, offset=0):
    """Frames (n, rows, cols) through the device entry point at a row stride and a pointer offset; returns what keeps the memory alive."""
    import torch
    n, rows, cols = frames.shape
    stride = cols if row_stride is None else row_stride
    buf = torch.zeros(n * rows * stride + 64, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + n * rows * stride].view(n, rows, stride)
    view[:, :, :cols] = torch.from_numpy(frames).cuda()
    out = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    det.detect_batch_device(buf.data_ptr() + offset, n, rows, cols, stride, rows * stride, out.data_ptr(), tw)
    det.sync()
    return buf, out


def test_large_chunks_and_other_forms_match_statement(answers, pool, tally, dictionary, test_bmp):
    """A handle of its own (one stream, host sub-chunk 1024: the debug views hold the whole chunk): the fused chunks of 1024 frames at 1080p
    (`mask`) and 1920 x 1200 (`mask_bands`), window 7 (`wide` + `any`), `banded135`, `unaligned` rows and pointers, 3840 x 2160, device BGR in
    the direct form, and the graph replay settings."""
    import torch
    state, fsz = dictionary
    n = len(pool)
    own = tk.Detector(state, fsz, device=0)
    try:
        own.set_option(capi.OPT_HOST_SUBCHUNK, 1024)
        own.set_option(capi.OPT_STREAMS, 1)

        def chunk(cases, count, what, want, tw=5, fused=False, **plan_args):
            rows, cols = cases[0]["frame"].shape
            tally.plan(want, what, rows=rows, cols=cols, nframes=count, adaptive_thresh=tw, **plan_args)
            idx = [(k * 5) % len(cases) for k in range(count)]
            frames = np.empty((count, rows, cols), np.uint8)
            for f, i in enumerate(idx):
                frames[f] = cases[i]["frame"]
            own.detect_batch(frames, tw)
            for f, i in enumerate(idx):
                check(own, f, cases[i], what, tally, fused=fused, images=(f % 16 == 0 or f == count - 1))

        chunk(pool, 1024, "fused 1024 frames", dict(fused=1, dec="mask", ccl="mask"), fused=True)
        wuxga = [answers.of("test.bmp", test_bmp)]
        wuxga += [answers.of("test.bmp rolled %d" % k, np.ascontiguousarray(np.roll(test_bmp, (7 * k, 33 * k), (0, 1)))) for k in (1, 2)]
        wuxga += [answers.of(a["name"] + " padded to 1200 rows", np.pad(a["frame"], ((60, 60), (0, 0)), "edge")) for a in pool[:8]]
        chunk(wuxga, 1024, "fused 1024 frames of 1920x1200", dict(fused=1, dec="mask_bands", ccl="mask"), fused=True)
        seven = [answers.of(a["name"], a["frame"], 7) for a in pool]
        chunk(seven, 1024, "1024 frames, window 7", dict(fused=0, dec="wide", ccl="any"), tw=7)
        wide = [answers.of(a["name"] + " padded to 1936 columns", np.pad(a["frame"], ((0, 0), (8, 8)), "edge")) for a in pool[::2]]
        chunk(wide, 256, "256 frames of 1936x1080", dict(fused=0, dec="banded135", ccl="tw5"))

        # rows with a stride of their own, and a frame pointer off by 4: the unaligned decimation
        idx = [k % n for k in range(64)]
        frames = np.stack([pool[i]["frame"] for i in idx])
        keep = _device_run(own, frames, row_stride=COLS + 4)
        tally.plan(dict(fused=0, dec="unaligned", ccl="tw5"), "64 device frames, row stride 1924", rows=ROWS, cols=COLS, nframes=64, row_stride=COLS + 4)
        for f, i in enumerate(idx):
            check(own, f, pool[i], "row stride 1924", tally, fused=False, images=f % 4 == 0)
        keep = _device_run(own, frames[:1], offset=4)
        tally.plan(dict(fused=0, dec="unaligned", latency=1), "one device frame, pointer off by 4", rows=ROWS, cols=COLS, nframes=1,
                   frames=keep[0].data_ptr() + 4)
        check(own, 0, pool[idx[0]], "pointer off by 4", tally, fused=False)
        keep = _device_run(own, frames[:8], offset=4, row_stride=COLS + 12)
        tally.plan(dict(fused=0, dec="unaligned", latency=0), "8 device frames, pointer off by 4, row stride 1932", rows=ROWS, cols=COLS, nframes=8,
                   frames=keep[0].data_ptr() + 4, row_stride=COLS + 12)
        for f in range(8):
            check(own, f, pool[idx[f]], "pointer off by 4, stride 1932", tally, fused=False)
        del keep, frames

        # 3840 x 2160: four 1080p frames each, rolled so that texture lies across the middle columns (the seam of the two waves of a row)
        uhd = []
        for k in (0, 4):
            quad = [a["frame"] for a in pool[k:k + 4]]
            img = np.roll(np.block([[quad[0], quad[1]], [quad[2], quad[3]]]), (ROWS // 2 + 7, COLS // 2 + 13), (0, 1))
            uhd.append(answers.of("uhd %d" % k, np.ascontiguousarray(img)))
        for fuse, want in ((1, dict(fused=0, ccl="tw5")), (2, dict(fused=1, dec="mask", ccl="mask", dec_xblocks=2))):
            own.set_option(capi.OPT_FUSED_SWEEP, fuse)
            tally.plan(want, "8 frames of 3840x2160, fused sweep option %d" % fuse, rows=2 * ROWS, cols=2 * COLS, nframes=8, fuse_mode=fuse)
            own.detect_batch(np.stack([uhd[f % 2]["frame"] for f in range(8)]))
            for f in range(8):
                check(own, f, uhd[f % 2], "4k, fused sweep option %d" % fuse, tally, fused=fuse == 2, images=f < 4)

        # the knife-edge set where the fused kernel evaluates the bound itself, in a small batch (the 64 and 1024-frame runs hold it too)
        knife = [a for a in pool if a["name"].startswith("knife")]
        tally.plan(dict(fused=1, dec="mask", ccl="mask"), "knife-edge frames, fused", rows=ROWS, cols=COLS, nframes=len(knife), fuse_mode=2)
        own.detect_batch(np.stack([a["frame"] for a in knife]))
        for f, a in enumerate(knife):
            check(own, f, a, "knife edges, fused", tally, fused=True)

        # device BGR frames in the direct form: the fused sweep converts as it loads; no gray image and no gray rows exist
        coloured = [answers.of(a["name"] + " coloured", fs.colourise(a["frame"], 40 + k)) for k, a in enumerate(pool[:8])]
        tally.plan(dict(bgr_direct=1, fused=1, dec="mask", ccl="mask"), "64 device BGR frames, direct", rows=ROWS, cols=COLS, nframes=64, channels=3, fuse_mode=2)
        idx = [(k * 3) % 8 for k in range(64)]
        dev = torch.from_numpy(np.stack([coloured[i]["frame"] for i in idx])).cuda()
        out = torch.zeros((64, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        own.detect_batch_bgr_device(dev.data_ptr(), 64, ROWS, COLS, COLS * 3, ROWS * COLS * 3, out.data_ptr())
        own.sync()
        with pytest.raises(ca.CtagError):
            own.debug(0, tk.DBG_GRAY)
        for f, i in enumerate(idx):
            check(own, f, coloured[i], "bgr direct", tally, fused=True, images=f % 4 == 0, half=False)
        # ... and in the two-step form: a gray image exists
        own.set_option(capi.OPT_BGR_DIRECT, 0)
        tally.plan(dict(bgr_direct=0, fused=1), "64 device BGR frames, two-step", rows=ROWS, cols=COLS, nframes=64, channels=3, fuse_mode=2, bgr_direct=0)
        own.detect_batch_bgr_device(dev.data_ptr(), 64, ROWS, COLS, COLS * 3, ROWS * COLS * 3, out.data_ptr())
        own.sync()
        for f, i in enumerate(idx):
            if f % 8 == 0:
                assert (own.debug(f, tk.DBG_GRAY).reshape(ROWS, COLS) == coloured[i]["s"]["gray"]).all(), f
            check(own, f, coloured[i], "bgr two-step on the device", tally, fused=True, images=f % 8 == 0, half=None)  # (the mask is the product)
        own.set_option(capi.OPT_BGR_DIRECT, 1)
        own.set_option(capi.OPT_FUSED_SWEEP, 1)
        del dev, out

        # graph replay settings on a batch of 8 and on one frame, each call made three times behind the same pointers
        frames = np.stack([pool[i]["frame"] for i in range(8)])
        for setting in (0, 1, 2):
            own.set_option(capi.OPT_GRAPH, setting)
            for count in (8, 1):
                for rep in range(3):
                    keep = _device_run(own, frames[:count]) if rep == 0 else keep
                    if rep:
                        own.detect_batch_device(keep[0].data_ptr(), count, ROWS, COLS, COLS, ROWS * COLS, keep[1].data_ptr())
                        own.sync()
                    for f in range(count):
                        check(own, f, pool[f], "graph setting %d, %d frames, call %d" % (setting, count, rep), tally, fused=False, images=rep == 2)
            tally.plan(dict(fused=0, dec="banded", ccl="tw5"), "graph setting %d" % setting, rows=ROWS, cols=COLS, nframes=8)
        own.set_option(capi.OPT_GRAPH, 2)
    finally:
        own.close()


def test_non_default_caps_and_area_limits_match_statement(answers, tally, dictionary):
    """`ctag_create_ex` with the dark_cap / area limits of test_non_default_params: each cap's knife-edge set through the two-kernel form
    (K2 reads the byte table built for the cap) and the fused form (the kernel evaluates the bound), and the area-limit frames."""
    state, fsz = dictionary
    for cap, area in zip(fs.CAPS[1:], (fs.AREA_PARAMS[1], fs.AREA_PARAMS[2], fs.AREA_PARAMS[0])):
        p = ca.default_params()
        p.dark_cap, p.area_min, p.area_max_fraction = cap, area[0], area[1]
        det = tk.Detector(state, fsz, params=p)
        try:
            det.set_option(capi.OPT_STREAMS, 1)
            knife = [answers.of("knife edges cap %g %d" % (cap, k), f, 5, cap, area) for k, f in enumerate(fs.knife_frames(cap, fs.cap_edge_cells(cap)))]
            count = max(len(knife), 6)  # more than the latency forms take
            idx = [k % len(knife) for k in range(count)]
            for fuse in (1, 2):
                det.set_option(capi.OPT_FUSED_SWEEP, fuse)
                tally.plan(dict(fused=int(fuse == 2), latency=0, ccl="mask" if fuse == 2 else "tw5"), "dark_cap %g, fused sweep option %d" % (cap, fuse),
                           rows=ROWS, cols=COLS, nframes=count, fuse_mode=fuse)
                det.detect_batch(np.stack([knife[i]["frame"] for i in idx]))
                for f, i in enumerate(idx):
                    check(det, f, knife[i], "dark_cap %g, fused sweep option %d" % (cap, fuse), tally, fused=fuse == 2)
            det.set_option(capi.OPT_FUSED_SWEEP, 1)
            for name, f, tw, its_area, tags in fs.labelling_frames():
                if "areas" in tags and its_area == area:
                    a = answers.of(name, f, tw, cap, area)
                    det.detect(f, tw)
                    check(det, 0, a, "area limits %s" % (area,), tally, fused=False)
                    assert len(a["s"]["candidates"]) == 4, name  # area_min, area_min + 1, limit - 1, limit
        finally:
            det.close()


def test_summary_names_every_form(tally):
    """Last in the file: every decimation and labelling form of the plan was run, each named with the plan line that proves it."""
    print("\nstages a0-a3, kernels vs statement: " + tally.report())
    assert {dec for dec, _ in tally.forms} == set(tk.DEC_FORMS), sorted(tally.forms)
    assert {ccl for _, ccl in tally.forms} == set(tk.CCL_FORMS), sorted(tally.forms)
    assert tally.frames >= 3000 and tally.images >= 500
