"""GPU tests of the verdicts of the member walk that the record kernels of the rig assembly, the camera set fit and the intrinsics fit
share (fit_member_walk, ctag_pose_dev.h), through the probes: one observation record of the smallest batch of each shapes file is made
not to describe its detection record, and the system must be, byte for byte, the one without that record -- or, for a mask bit at or
above the frame's marker count, which these kernels ignore (k_pose_cov rejects it), the untouched one."""
import numpy as np
import pytest

import cam_fit_shapes as csh
import cylindertag_amd as ca
import intr_fit_shapes as ish
import pose_statement as ps
import rig_fit_shapes as rsh
from cam_fit_testlib import device_mv_poses, set_of
from cam_fit_testlib import input_of as cam_input_of
from intr_fit_testlib import NOT_SEEN, camera_c
from intr_fit_testlib import input_of as intr_input_of
from rig_fit_testlib import Detectors, device_rig_poses, model_at

pytestmark = pytest.mark.gpu
LAMBDA = 1e-3
KEYS = ("S", "g", "delta")


@pytest.fixture(scope="module")
def dets():
    d = Detectors()
    yield d
    d.close()


def _rig(dets, name, g=0):
    """(probe(records) of rig g, device rig-pose records, detection records) of a rig batch at the rule-2 start."""
    b, A = rsh.batch(name), rsh.assembled(name)
    det, cam, M = dets.of(b), ca.make_camera(b["K"], b["dist"]), model_at(b, A["X0"])
    rigs = ca.Rigs(M, A["rig_placed"], b["n_rigs"])
    recs = device_rig_poses(det, b["recs"], M, rigs, cam)
    return (lambda r: det.rig_fit_system(b["recs"], r, M, rigs, cam, g, LAMBDA)), recs, b["recs"]


def _cam(dets, name):
    """(probe(records), device multi-view records, detection records [camera][instant] of the placed cameras) at the rule-2 start."""
    b, A = csh.case(name), csh.assembled(name)
    det = dets.of(b)
    M, rigs, _ = cam_input_of(b)
    placed = A["init"]["placed"]
    cs = set_of(b, placed, A["R0"], A["t0"])
    frames = np.ascontiguousarray(b["recs"][placed])
    mvp = device_mv_poses(det, frames, M, rigs, cs)
    return (lambda r: det.camera_fit_system(frames, r, M, rigs, cs, A["slot"], LAMBDA)), mvp, frames


def _intr(dets, name):
    """(probe(records), device rig-pose records under the planted camera, detection records)."""
    c = ish.case(name)
    det = dets.of(c)
    M, rigs, _ = intr_input_of(c)
    cam = camera_c(ish.planted_camera(c), c)
    recs = device_rig_poses(det, c["recs"], M, rigs, cam)
    return (lambda r: det.intrinsics_fit_system(c["recs"], r, M, rigs, cam, LAMBDA, free_mask=c["mask"], tie_focal=int(c["tie"]))), recs, c["recs"]


SETUPS = {"rig": (_rig, rsh.NAMES[0]), "camera": (_cam, "a noise-free"), "intrinsics": (_intr, "a noise-free")}


@pytest.fixture(scope="module")
def state(dets):
    memo = {}

    def of(kind):
        """(probe, records, detection records, index of the observation record the cases touch, the untouched result, the baseline:
        the result with that record's status not OK, so that it is no observation at all)."""
        if kind not in memo:
            make, name = SETUPS[kind]
            probe, recs, frames = make(dets, name)
            counted = "n_cameras" if kind == "camera" else "n_members"
            w = next(i for i in range(len(recs)) if recs[i]["status"] == 0 and recs[i][counted] >= (1 if kind == "intrinsics" else 2))
            untouched = probe(recs)
            out = recs.copy()
            out[w]["status"] = NOT_SEEN
            base = probe(out)
            assert not untouched["bad_pivot"] and not base["bad_pivot"]
            assert untouched["S"].tobytes() != base["S"].tobytes(), "the record chosen does not matter to the system"
            memo[kind] = (probe, recs, frames, w, untouched, base)
        return memo[kind]
    return of


def _same(got, ref, kind, flagged):
    """got is ref to the byte.  A record the walk turned down is left out; the intrinsics probe alone counts every flagged record as
    bad, and its delta is then not part of the statement."""
    if kind == "intrinsics" and flagged:
        assert got["bad_pivot"] == 1
        keys = ("S", "g")
    else:
        assert got["bad_pivot"] == ref["bad_pivot"]
        keys = KEYS
    for k in keys:
        assert got[k].tobytes() == ref[k].tobytes(), k


@pytest.mark.parametrize("kind", list(SETUPS))
@pytest.mark.parametrize("off", [-1, 1])
def test_a_point_count_off_by_one_leaves_the_record_out(state, kind, off):
    probe, recs, _, w, _, base = state(kind)
    out = recs.copy()
    out[w]["n_points"] += off
    _same(probe(out), base, kind, True)


@pytest.mark.parametrize("kind", list(SETUPS))
def test_a_frame_past_the_last_leaves_the_record_out(state, kind):
    probe, recs, frames, w, _, base = state(kind)
    out = recs.copy()
    out[w]["frame"] = frames.shape[-1]
    _same(probe(out), base, kind, True)


@pytest.mark.parametrize("kind", list(SETUPS))
def test_a_mask_bit_past_the_frames_markers_is_ignored(state, kind):
    """The bit of the first marker index the frame does not have, and the last bit of the mask."""
    probe, recs, frames, w, untouched, _ = state(kind)
    f = int(recs[w]["frame"])
    if kind == "camera":
        c = next(c for c in range(frames.shape[0]) if recs[w]["points_of_camera"][c] > 0)
        n_markers, mask = int(frames[c][f]["n_markers"]), lambda r: r["member_mask"][c]
    else:
        n_markers, mask = int(frames[f]["n_markers"]), lambda r: r["member_mask"]
    assert 0 < n_markers < 127
    out = recs.copy()
    for k in (n_markers, 127):
        assert not (mask(out[w])[k >> 5] >> (k & 31)) & 1
        mask(out[w])[k >> 5] |= np.uint32(1 << (k & 31))
    _same(probe(out), untouched, kind, False)


def test_a_member_outside_every_rig_system_leaves_the_record_out(dets):
    """Rig probe, batch (c): a loose model's marker stands in frames of rig 0.  Its bit set in a record's mask, with the record's counts
    raised by the marker's, the walk adds up to n_points and only the model's missing slot turns the record down."""
    name = rsh.NAMES[2]
    b, A = rsh.batch(name), rsh.assembled(name)
    loose = [m for m in range(len(b["rig_of_model"])) if b["rig_of_model"][m] < 0]
    assert loose, "batch (c) has a model outside every rig"
    probe, recs, frames = _rig(dets, name)
    ids = [int(b["model"]["ids"][m]) for m in loose]
    w, k = next((i, k) for i in range(len(recs)) if recs[i]["status"] == 0 and recs[i]["rig"] == 0 and recs[i]["n_members"] >= 2
                for k in range(ps.marker_count(frames[recs[i]["frame"]])) if int(frames[recs[i]["frame"]]["markers"][k]["marker_id"]) in ids)
    st, _, n, _, _ = ps.expected_record(frames[recs[w]["frame"]], k, b["model"])
    assert st == ps.OK and not (recs[w]["member_mask"][k >> 5] >> (k & 31)) & 1
    base = recs.copy()
    base[w]["status"] = NOT_SEEN
    out = recs.copy()
    out[w]["member_mask"][k >> 5] |= np.uint32(1 << (k & 31))
    out[w]["n_members"] += 1
    out[w]["n_points"] += n
    ref = probe(base)
    assert probe(recs)["S"].tobytes() != ref["S"].tobytes(), "the record chosen does not matter to the system"
    _same(probe(out), ref, "rig", True)
