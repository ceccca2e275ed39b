"""Stage a4 of the HIP path (`k_quad.hip`) against the independent statement in `tests/edge_testlib.py` (-m gpu): every candidate's
`has_quad` and `n_boundary` (DBG_CANDIDATES) and its corners (DBG_CAND_QUADS) with the "ref" bars of `test_edge_extraction_cpu.py`
(no excuses against an implementation), on the frames of `tests/edge_shapes.py`, through every boundary-stage form the chunk plan
picks: one frame (latency, a wave per component), a 64-frame batch (k_pack), a fused batch of 1024 frames (k_silhouette_mask),
3840x2160 frames (prescan) and device-resident BGR frames in the direct form (the fused sweep converting as it loads).  Host BGR
frames are converted by k_bgr2gray and then take the gray chain: they are checked too, against the gray plan they run.
`tk.chunk_plan` with the same arguments confirms the form of each run; the byte equality with the oracle stays beside it.
The statement's answers are worked out once per distinct frame and reused for every copy in a batch; its two modes ("ref" against
"f64") are compared on these frames by the CPU test.  Runs that need non-default options get a handle of their own."""
import numpy as np
import pytest

import edge_shapes as es
import edge_testlib as et
import cylindertag_amd as ca
import testkit as tk
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shape_answers(oracle, dictionary):
    """The statement's answers and the oracle's run, once per distinct frame: [(name, frame, oracle run, ref)]."""
    et.use_shared_math(oracle)
    state, fs = dictionary
    out = []
    for name, img in es.shape_frames():
        o = oracle.detect(img, state, fs)
        out.append((name, img, o, et.extract_frame(o["labels"], "ref")))
    return out


def _check_frame(det, f, answer, tally, what):
    name, _, o, ref = answer
    cand = det.debug(f, tk.DBG_CANDIDATES)
    quads = det.debug(f, tk.DBG_CAND_QUADS)
    assert cand.shape[0] == len(ref), (what, name)
    tally.add("%s %s" % (what, name), ref, None, cand[:, 5], cand[:, 6], quads)
    assert (cand[:, 0:7] == o["candidates"][:, 1:8]).all(), (what, name)  # and byte for byte the oracle's
    assert quads.tobytes() == o["candidate_quads"].tobytes(), (what, name)


def _plan(want, **args):
    plan = tk.chunk_plan(**args)
    assert {k: plan[k] for k in want} == want, (args, plan)
    return "%s: %s" % (", ".join("%s=%s" % kv for kv in args.items()), ", ".join("%s=%s" % kv for kv in want.items()))


def test_edge_extraction_forms_match_statement(detector, oracle, dictionary, shape_answers):
    tally = et.Tally()
    forms = []
    n = len(shape_answers)
    # one frame per call: the latency kernels, every component a wave of its own
    forms.append(_plan(dict(latency=1, all_wave=1, fused=0), rows=es.ROWS, cols=es.COLS, nframes=1))
    for a in shape_answers:
        detector.detect(a[1])
        _check_frame(detector, 0, a, tally, "alone")
    # a 64-frame batch: packed components (k_pack)
    forms.append(_plan(dict(latency=0, all_wave=0, fused=0, mask_scan=0), rows=es.ROWS, cols=es.COLS, nframes=64))
    idx = [k % n for k in range(64)]
    detector.detect_batch(np.stack([shape_answers[i][1] for i in idx]))
    for f, i in enumerate(idx):
        _check_frame(detector, f, shape_answers[i], tally, "batch 64 frame %d" % f)
    # host BGR frames: k_bgr2gray into the gray slab, then the gray chain of one frame
    forms.append(_plan(dict(latency=1, all_wave=1, fused=0), rows=es.ROWS, cols=es.COLS, nframes=1, channels=1))
    for a in shape_answers[:6]:
        bgr = np.ascontiguousarray(np.repeat(a[1][:, :, None], 3, axis=2))
        assert (oracle.bgr2gray(bgr) == a[1]).all()  # equal channels: the gray frame itself
        detector.detect_bgr(bgr)
        assert (detector.debug(0, tk.DBG_GRAY).reshape(a[1].shape) == a[1]).all()  # the two-step form: a gray image exists
        _check_frame(detector, 0, a, tally, "host bgr")
    state, fs = dictionary
    own = tk.Detector(state, fs, device=0)
    try:
        # one chunk of 1024 frames on one stream (host batches go up in steps of 128, and two streams split a chunk into pieces:
        # the debug views hold the last piece)
        own.set_option(capi.OPT_HOST_SUBCHUNK, 1024)
        own.set_option(capi.OPT_STREAMS, 1)
        # a fused batch of 1024 frames: silhouettes from the threshold mask (k_silhouette_mask)
        forms.append(_plan(dict(latency=0, fused=1, mask_scan=1, prescan=1), rows=es.ROWS, cols=es.COLS, nframes=1024))
        idx = [(k * 5) % n for k in range(1024)]
        frames = np.empty((1024, es.ROWS, es.COLS), np.uint8)
        for f, i in enumerate(idx):
            frames[f] = shape_answers[i][1]
        own.detect_batch(frames)
        del frames
        for f, i in enumerate(idx):
            _check_frame(own, f, shape_answers[i], tally, "fused 1024 frame %d" % f)
        # device-resident BGR frames in the direct form: the fused sweep reads the BGR bytes (CTAG_OPT_FUSED_SWEEP 2 takes it for 64)
        import torch
        own.set_option(capi.OPT_FUSED_SWEEP, 2)
        forms.append(_plan(dict(bgr_direct=1, latency=0, fused=1, mask_scan=1), rows=es.ROWS, cols=es.COLS, nframes=64, channels=3,
                           fuse_mode=2))
        idx = [(k * 3) % n for k in range(64)]
        dev = torch.from_numpy(np.stack([np.repeat(shape_answers[i][1][:, :, None], 3, axis=2) for i in idx])).cuda()
        out = torch.zeros((64, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        own.detect_batch_bgr_device(dev.data_ptr(), 64, es.ROWS, es.COLS, es.COLS * 3, es.ROWS * es.COLS * 3, out.data_ptr())
        own.sync()
        with pytest.raises(ca.CtagError):
            own.debug(0, tk.DBG_GRAY)  # the direct form: no gray image was written
        for f, i in enumerate(idx):
            _check_frame(own, f, shape_answers[i], tally, "bgr direct 64 frame %d" % f)
        del dev, out
    finally:
        own.close()
    print("\nedgeExtraction, kernels vs statement (plan forms: %s): %s" % ("; ".join(forms), tally.report()))
    tally.check()


def test_edge_extraction_at_4k_matches_statement(detector, oracle, dictionary, shape_answers):
    """3840 x 2160 frames of four shape frames each, eight to a batch: the boundary stage's prescan."""
    state, fs = dictionary
    form = _plan(dict(latency=0, prescan=1), rows=2 * es.ROWS, cols=2 * es.COLS, nframes=8)
    frames = [es.uhd_frame([a[1] for a in shape_answers[k:k + 4]]) for k in (0, 4)]
    answers = []
    for k, img in enumerate(frames):
        o = oracle.detect(img, state, fs)
        answers.append(("uhd %d" % k, img, o, et.extract_frame(o["labels"], "ref")))
    tally = et.Tally()
    detector.detect_batch(np.stack([frames[f % 2] for f in range(8)]))
    for f in range(8):
        _check_frame(detector, f, answers[f % 2], tally, "4k batch frame %d" % f)
    print("\nedgeExtraction at 3840x2160, kernels vs statement (%s): %s" % (form, tally.report()))
    tally.check()
    assert tally.compared >= 8 * 100
