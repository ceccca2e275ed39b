"""The hand-eye kernels (k_hand_eye.hip) against tests/hand_eye_statement.py, one undamped Gauss-Newton step from the start
(max_iterations = 1, lambda0 = 0): every field of every record within hand_eye_statement.BAR_STEP on every batch of
tests/hand_eye_shapes.py; statuses, flags and counts exact; a problem's bytes in any rig slot and on any run; nothing written outside the
two output arrays; the device form against the host form."""
import numpy as np
import pytest
import torch

import hand_eye_shapes as sh
import hand_eye_statement as hs
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 4096
fit = sh.device_fit


@pytest.mark.parametrize("name", sh.BATCHES)
def test_single_step_matches_statement(detector, name):
    b = sh.batch(name)
    rec, frames = fit(detector, b, max_iterations=1, lambda0=0.0)
    sh.check_against(rec, frames, sh.single_step(name), b, name, hs.BAR_STEP)


def body(rec):
    """a record's bytes without its rig field"""
    c = np.array(rec, copy=True)
    c["rig"] = 0
    return c.tobytes()


def test_a_problem_has_the_same_bytes_anywhere(detector):
    """rig 5 of `counts` (65 used frames: two chunks and a lane): on a second run, and in slot 2 beside other rigs"""
    b = sh.batch("counts")
    full, ffr = fit(detector, b)
    again, afr = fit(detector, b)
    assert full.tobytes() == again.tobytes() and ffr.tobytes() == afr.tobytes()
    c = dict(b)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov"):
        c[k] = np.array(b[k], copy=True)
        c[k][:, 2], c[k][:, 5], c[k][:, 0] = b[k][:, 5], b[k][:, 6], b[k][:, 3]
    moved, mfr = fit(detector, c)
    assert moved["status"][2] == capi.HE_OK and body(moved[2]) == body(full[5])
    assert body(mfr[:, 2]) == body(ffr[:, 5])
    # alone, in a one-rig call (another grid)
    one = dict(b, n_rigs=1, rec_rig=np.zeros((b["n_frames"], 1), np.int32), rec_frame=b["rec_frame"][:, :1])
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov"):
        one[k] = np.ascontiguousarray(b[k][:, 5:6])
    alone, _ = fit(detector, one)
    assert body(alone[0]) == body(full[5])


def test_no_byte_outside_the_two_arrays(detector):
    b = sh.batch("holes")
    P, Q, K = sh.to_records(b)
    n, nr = b["n_frames"] * b["n_rigs"], b["n_rigs"]
    dev = torch.device("cuda:0")
    dP = torch.from_numpy(P.view(np.uint8)).to(dev)
    dQ = torch.from_numpy(Q.view(np.uint8)).to(dev)
    out = torch.full((GUARD + nr * capi.HAND_EYE_DT.itemsize + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    frs = torch.full((GUARD + n * capi.HAND_EYE_FRAME_DT.itemsize + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    rigs = sh.RigSet(nr)
    torch.cuda.synchronize()
    detector.fit_hand_eye_device(rigs, dP.data_ptr(), dQ.data_ptr(), b["n_frames"], K, out.data_ptr() + GUARD, frs.data_ptr() + GUARD, opts=sh.he_opts(b))
    K[:] = 0    # the links were copied before the call returned
    detector.sync()
    o, s = out.cpu().numpy(), frs.cpu().numpy()
    assert (o[:GUARD] == 0xA5).all() and (o[-GUARD:] == 0xA5).all() and (s[:GUARD] == 0x5A).all() and (s[-GUARD:] == 0x5A).all()
    rec = o[GUARD:-GUARD].view(capi.HAND_EYE_DT)
    fr = s[GUARD:-GUARD].view(capi.HAND_EYE_FRAME_DT).reshape(b["n_frames"], nr)
    host, hfr = fit(detector, b)
    assert rec.tobytes() == host.tobytes() and fr.tobytes() == hfr.tobytes()   # device form against host form, byte for byte
    # frames_dev == NULL: the problem records are what they were, and the frame array is not touched
    out2 = torch.full_like(out, 0xA5)
    _, _, K = sh.to_records(b)
    detector.fit_hand_eye_device(rigs, dP.data_ptr(), dQ.data_ptr(), b["n_frames"], K, out2.data_ptr() + GUARD, None, opts=sh.he_opts(b))
    detector.sync()
    assert out2.cpu().numpy().tobytes() == o.tobytes()
    nofr, none = fit(detector, b, frames=False)
    assert none is None and nofr.tobytes() == host.tobytes()
