"""The track smoother's kernels (k_track.hip) against tests/track_statement.py, one undamped Gauss-Newton step from the start
(max_iterations = 1, lambda0 = 0): every field of every record within track_statement.BAR_STEP for every allowed segment_frames on every
batch of tests/track_shapes.py; status, flags and the piece table exact; a piece's bytes wherever it lies; nothing written outside the
two output arrays."""
import numpy as np
import pytest
import torch

import track_shapes as sh
import track_statement as ts
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

SEGMENTS = (8, 16, 32, 64, 0)
GUARD = 4096


smooth, opts_of, check_against = sh.device_smooth, sh.track_opts, sh.check_against


@pytest.mark.parametrize("name", sh.BATCHES)
@pytest.mark.parametrize("L", SEGMENTS)
def test_single_step_matches_statement(detector, name, L):
    b = sh.batch(name)
    rec, stat = smooth(detector, b, max_iterations=1, lambda0=0.0, segment_frames=L)
    assert (stat["rounds"] == sh.single_step(name)[1]["rounds"]).all()
    check_against(rec, stat, sh.single_step(name), "%s L=%d" % (name, L), ts.BAR_STEP)


def test_piece_table_is_the_statements(detector):
    """the pieces as the records show them: runs of tracked frames split where the statement splits them"""
    for name in ("lengths", "gaps"):
        b = sh.batch(name)
        rec, stat = smooth(detector, b, max_iterations=1, lambda0=0.0)
        _, wstat, table = sh.single_step(name)
        for g, pcs in enumerate(table):
            tracked = np.zeros(b["n_frames"], bool)
            for a, e in pcs:
                tracked[a:e + 1] = True
            assert ((rec["status"][:, g] == ts.OK) == tracked).all()
            assert stat["n_pieces"][g] == len(pcs) and stat["longest_piece"][g] == max([e - a + 1 for a, e in pcs] or [0])


def cut(b, rig, a, e):
    """frames a .. e of one rig of batch b as a one-rig batch"""
    c = dict(b, n_frames=e - a + 1, n_rigs=1, times=None if b["times"] is None else b["times"][a:e + 1] - b["times"][a])
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov"):
        c[k] = np.ascontiguousarray(b[k][a:e + 1, rig:rig + 1])
    c["rec_rig"] = np.zeros((e - a + 1, 1), np.int32)
    c["rec_frame"] = np.arange(e - a + 1, dtype=np.int32)[:, None]
    return c


def body(rec):
    """a record's bytes without its rig and frame fields"""
    c = np.array(rec, copy=True)
    c["rig"], c["frame"] = 0, 0
    return c.tobytes()


@pytest.mark.parametrize("L", (8, 32))
def test_a_piece_has_the_same_bytes_anywhere(detector, L):
    """the 65-frame piece of rig 1 of `lengths`: on a second run, in another rig slot beside other rigs, and alone in a batch of its own
    at another frame offset (there with times that are multiples of 2^-5, so that every difference of times is the same number wherever
    the piece lies)"""
    b = sh.batch("lengths")
    _, _, table = sh.single_step("lengths")
    a, e = table[1][2]
    assert e - a + 1 == 65
    full, _ = smooth(detector, b, segment_frames=L)
    again, _ = smooth(detector, b, segment_frames=L)
    assert full.tobytes() == again.tobytes()
    # the same rig moved to slot 3 of a batch whose other rigs are different
    c = dict(b)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov"):
        c[k] = np.array(b[k], copy=True)
        c[k][:, 3], c[k][:, 1] = b[k][:, 1], b[k][:, 0]
    moved, _ = smooth(detector, c, segment_frames=L)
    assert body(moved[a:e + 1, 3]) == body(full[a:e + 1, 1])
    t = np.arange(b["n_frames"]) * 0.03125
    fullt, _ = smooth(detector, dict(b, times=t), segment_frames=L)
    alone, _ = smooth(detector, cut(dict(b, times=t), 1, a - 3, e + 2), segment_frames=L)
    assert body(alone[3:3 + 65, 0]) == body(fullt[a:e + 1, 1])


def test_no_byte_outside_the_two_arrays(detector):
    b = sh.batch("gaps")
    P, Q = sh.to_records(b)
    n, nr = b["n_frames"] * b["n_rigs"], b["n_rigs"]
    dev = torch.device("cuda:0")
    dP = torch.from_numpy(P.view(np.uint8)).to(dev)
    dQ = torch.from_numpy(Q.view(np.uint8)).to(dev)
    out = torch.full((GUARD + n * capi.TRACK_DT.itemsize + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    stat = torch.full((GUARD + nr * capi.TRACK_STAT_DT.itemsize + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    rigs = sh.RigSet(nr)
    torch.cuda.synchronize()
    detector.smooth_rig_track_device(rigs, dP.data_ptr(), dQ.data_ptr(), b["n_frames"], out.data_ptr() + GUARD, stat.data_ptr() + GUARD,
                                     times=b["times"], opts=opts_of(b))
    detector.sync()
    o, s = out.cpu().numpy(), stat.cpu().numpy()
    assert (o[:GUARD] == 0xA5).all() and (o[-GUARD:] == 0xA5).all() and (s[:GUARD] == 0x5A).all() and (s[-GUARD:] == 0x5A).all()
    rec = o[GUARD:-GUARD].view(capi.TRACK_DT).reshape(b["n_frames"], nr)
    st = s[GUARD:-GUARD].view(capi.TRACK_STAT_DT)
    host, hstat = smooth(detector, b)
    assert rec.tobytes() == host.tobytes() and st.tobytes() == hstat.tobytes()   # device form against host form, byte for byte
