"""The track filter's kernel (k_track_filter.hip through include/ctag_pose.h, track filtering) against the float64 statement of
tests/track_filter_statement.py on every batch of tests/track_filter_shapes.py -- statuses and flags exact, the rest within the statement's
measured bars -- and what rule 8 promises byte for byte: the same records however the frames are divided among calls, wherever the rig
sits and whatever the other rigs hold."""
import numpy as np
import pytest

import track_filter_shapes as fsh
import track_filter_statement as fs
import track_shapes as sh

pytestmark = pytest.mark.gpu


body = fsh.body


@pytest.mark.parametrize("name", fsh.BATCHES)
def test_device_matches_statement(detector, name):
    rec = fsh.device_run(detector, fsh.batch(name))
    fsh.check_against(rec, fsh.statement(name), name)


def test_covariances_of_the_long_batch_are_positive_definite(detector):
    rec = fsh.device_run(detector, fsh.batch("long"))
    ok = rec["status"] == fs.OK
    assert ok.sum() > 7000
    assert np.linalg.eigvalsh(rec["cov"][ok]).min() > 0 and (rec["vel_sigma"][ok] > 0).all()


@pytest.mark.parametrize("name", ("n129", "gaps"))
def test_split_invariance_byte_for_byte(detector, name):
    """129 frames as one call, as 129 calls of one, as (64, 1, 64) and as (63, 66) (and `gaps`, with times, in the same manner)"""
    b = fsh.batch(name)
    n = b["n_frames"]
    whole = fsh.device_run(detector, b)
    splits = ([1] * n, [64, 1, n - 65], [63, n - 63]) if n > 65 else ([1] * n, [n // 2, n - n // 2])
    for split in splits:
        with fsh.DeviceFilter(detector, b) as F:
            parts, a = [], 0
            for k in split:
                parts.append(F.run(fs.frames_slice(b, a, a + k), times=None if b["times"] is None else b["times"][a:a + k]))
                a += k
        got = np.concatenate(parts)
        assert (got["frame"] == np.concatenate([np.arange(k) for k in split])[:, None]).all()
        assert body(got) == body(whole), split[:3]


def test_rig_permutation_and_rig_count(detector):
    """a rig's bytes do not depend on its index, on n_rigs or on the other rigs"""
    b = fsh.batch("gaps")
    whole = fsh.device_run(detector, b)
    perm = [2, 0, 1]
    c = dict(b)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov"):
        c[k] = np.ascontiguousarray(b[k][:, perm])
    moved = fsh.device_run(detector, c)
    for new, old in enumerate(perm):
        assert body(moved[:, new]) == body(whole[:, old])
    one = dict(c, n_rigs=1)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov", "rec_rig", "rec_frame"):
        one[k] = np.ascontiguousarray(c[k][:, :1])
    alone = fsh.device_run(detector, one)
    assert body(alone[:, 0]) == body(whole[:, perm[0]])
    again = fsh.device_run(detector, b)
    assert again.tobytes() == whole.tobytes()


def test_bad_input_rig_leaves_its_state_and_the_other_rigs_alone(detector):
    b = fsh.batch("bad_rig")
    clean = dict(b, rec_rig=np.tile(np.arange(3, dtype=np.int32), (b["n_frames"], 1)))
    want = fsh.device_run(detector, clean)
    with fsh.DeviceFilter(detector, b) as F:
        first = F.run(fs.frames_slice(clean, 0, 10))
        bad = F.run(fs.frames_slice(b, 10, 30))       # the misplaced record is frame 17 of rig 1: the whole call of that rig
        assert (bad["status"][:, 1] == fs.BAD_INPUT).all() and (bad["rig"][:, 1] == 1).all() and (bad["frame"][:, 1] == np.arange(20)).all()
        for k in sh.FIELDS[1:]:
            assert not bad[k][:, 1].any(), k
        assert body(bad[:, 0]) == body(want[10:30, 0]) and body(bad[:, 2]) == body(want[10:30, 2])
    # the state of rig 1 is what frame 9 left: clean frames given afterwards (a second later: the filter's clock has moved on) continue
    # the track exactly as they do in a filter that never saw the bad call
    t = np.arange(b["n_frames"]) / 30.0
    tail = fs.frames_slice(clean, 10, 30)
    with fsh.DeviceFilter(detector, b) as F:
        F.run(fs.frames_slice(clean, 0, 10), times=t[:10])
        F.run(fs.frames_slice(b, 10, 30), times=t[10:30])
        after = F.run(tail, times=t[10:30] + 1.0)
    with fsh.DeviceFilter(detector, b) as F:
        F.run(fs.frames_slice(clean, 0, 10), times=t[:10])
        ref = F.run(tail, times=t[10:30] + 1.0)
    assert (ref["status"][:, 1] == fs.OK).all() and not (ref["flags"][:, 1] & fs.FLAG_STARTED).any()
    assert body(after[:, 1]) == body(ref[:, 1])
