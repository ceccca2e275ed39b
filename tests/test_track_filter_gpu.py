"""The track filter's object and calls (include/ctag_pose.h, track filtering): predict, reset, several filters on one handle, the device
forms enqueued behind the pose and covariance kernels without a wait, every CTAG_ERR_ARG, and the live loop end to end."""
import ctypes as C

import numpy as np
import pytest

import track_filter_shapes as fsh
import track_filter_statement as fs
import track_shapes as sh
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu
body = fsh.body


def test_predict_is_the_unmeasured_frames_record_and_leaves_the_state(detector):
    b = fsh.batch("n65")
    head, nxt = fs.frames_slice(b, 0, 40), fs.frames_slice(b, 40, 41)
    t_next = 40 / 30.0
    unmeasured = dict(nxt, pose_status=np.full_like(nxt["pose_status"], sh.POSE_NOT_SEEN))
    with fsh.DeviceFilter(detector, b) as F:
        F.run(head)
        want = F.run(unmeasured, times=[t_next])[0]
    with fsh.DeviceFilter(detector, b) as F:
        F.run(head)
        p1 = F.f.predict(t_next)
        p2 = F.f.predict(t_next)
        far = F.f.predict(t_next + 0.05)
        after = F.run(nxt, times=[t_next])[0]
    with fsh.DeviceFilter(detector, b) as F:
        F.run(head)
        plain = F.run(nxt, times=[t_next])[0]
    assert (want["status"] == fs.OK).all() and p1.tobytes() == want.tobytes() == p2.tobytes()
    assert far.tobytes() != p1.tobytes()
    assert after.tobytes() == plain.tobytes()
    # the statement's prediction
    S = fs.Filter(b["n_rigs"], fs.filter_opts(b))
    S.run(head)
    fsh.check_against(p1.reshape(1, -1), S.predict(t_next), "predict")
    # an EMPTY track
    with fsh.DeviceFilter(detector, b) as F:
        e = F.f.predict(1.0)
        assert (e["status"] == fs.NOT_TRACKED).all() and (e["rig"] == np.arange(b["n_rigs"])).all()
        for k in sh.FIELDS[1:]:
            assert not e[k].any()


def test_reset(detector):
    b = fsh.batch("n63")
    with fsh.DeviceFilter(detector, b) as F:
        first = F.run(b)
        F.f.reset()
        assert (F.f.predict(0.5)["status"] == fs.NOT_TRACKED).all()
        second = F.run(b)       # times == NULL count from 0 again, and an earlier time is accepted again
    assert first.tobytes() == second.tobytes()


def test_two_filters_on_one_handle_do_not_interact(detector):
    a, b = fsh.batch("n65"), fsh.batch("spin")
    wa, wb = fsh.device_run(detector, a), fsh.device_run(detector, b)
    with fsh.DeviceFilter(detector, a) as FA, fsh.DeviceFilter(detector, b) as FB:
        ga = [FA.run(fs.frames_slice(a, 0, 30))]
        gb = [FB.run(fs.frames_slice(b, 0, 17))]
        ga.append(FA.run(fs.frames_slice(a, 30, 65)))
        gb.append(FB.run(fs.frames_slice(b, 17, 50)))
    assert body(np.concatenate(ga)) == body(wa) and body(np.concatenate(gb)) == body(wb)


def test_device_form_writes_no_byte_outside_its_records(detector):
    import torch
    b = fsh.batch("gaps")
    P, Q = sh.to_records(b)
    n, GUARD = b["n_frames"] * b["n_rigs"], 4096
    dP, dQ = torch.from_numpy(P.view(np.uint8)).cuda(), torch.from_numpy(Q.view(np.uint8)).cuda()
    out = torch.full((GUARD + n * capi.TRACK_DT.itemsize + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with fsh.DeviceFilter(detector, b) as F:
        F.f.step_device(dP.data_ptr(), dQ.data_ptr(), out.data_ptr() + GUARD, b["n_frames"], times=b["times"])
        detector.sync()
    o = out.cpu().numpy()
    assert (o[:GUARD] == 0xA5).all() and (o[-GUARD:] == 0xA5).all()
    assert o[GUARD:-GUARD].tobytes() == fsh.device_run(detector, b).tobytes()


def test_multi_frame_device_calls_in_a_row_without_a_wait(detector):
    """four calls of several frames enqueued back to back, each with its own times array that is overwritten as soon as the call returns
    (the filter stages them in two buffers in turn): the bytes of the one call"""
    import torch
    b = fsh.batch("n129")
    P, Q = sh.to_records(b)
    nr, split = b["n_rigs"], (40, 30, 33, 26)
    t_all = np.arange(b["n_frames"]) / 30.0
    P["frame"] = np.repeat(np.concatenate([np.arange(k) for k in split]), nr)   # the frame fields count within the call
    dP, dQ = torch.from_numpy(P.view(np.uint8)).cuda(), torch.from_numpy(Q.view(np.uint8)).cuda()
    out = torch.zeros(len(P) * capi.TRACK_DT.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with fsh.DeviceFilter(detector, b) as F:
        whole = F.run(b, times=t_all)
    with fsh.DeviceFilter(detector, b) as F:
        a = 0
        for k in split:
            t = t_all[a:a + k].copy()
            F.f.step_device(dP.data_ptr() + a * nr * P.itemsize, dQ.data_ptr() + a * nr * Q.itemsize, out.data_ptr() + a * nr * capi.TRACK_DT.itemsize, k, times=t)
            t[:] = -1.0
            a += k
        detector.sync()
    got = out.cpu().numpy().view(capi.TRACK_DT).reshape(b["n_frames"], nr)
    assert body(got) == body(whole)


BAD_OPTS = [dict(struct_size=68), dict(loss=3), dict(loss=-1), dict(max_gap=0), dict(gate=-1.0), dict(gate=float("nan")), dict(gate=float("inf"))]
for _k in ("dt", "q_rot", "q_trans", "vel0_sigma_rot", "vel0_sigma_trans", "loss_scale"):
    BAD_OPTS += [{_k: 0.0}, {_k: -1.0}, {_k: float("inf")}, {_k: float("nan")}]


def create(det, rigs, opts):
    f = C.c_void_p()
    return det.L.ctag_track_filter_create(det.h, rigs.r if rigs is not None else None, C.byref(opts) if opts is not None else None, C.byref(f)), f


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_every_bad_option_alone_is_err_arg(detector, bad):
    rigs = sh.RigSet(2)
    st, f = create(detector, rigs, capi.track_filter_opts())
    assert st == 0
    detector.L.ctag_track_filter_free(f)
    st, f = create(detector, rigs, capi.track_filter_opts(**bad))
    assert st == capi.ERR_ARG and not f.value


def test_defaults_are_the_smoothers(detector):
    o, t = capi.track_filter_opts(), capi.track_opts()
    assert (o.loss, o.max_gap, o.dt, o.gate) == (capi.TRACK_LOSS_NONE, 5, 1.0 / 30.0, 0.0)
    for k in ("q_rot", "q_trans", "vel0_sigma_rot", "vel0_sigma_trans", "loss_scale"):
        assert getattr(o, k) == getattr(t, k)


def test_bad_arguments_times_and_sizes_are_err_arg(detector):
    L = detector.L
    b = fsh.batch("n2")
    P, Q = sh.to_records(b)
    out = np.zeros(len(P), capi.TRACK_DT)
    rigs = sh.RigSet(2)
    assert create(detector, None, None)[0] == capi.ERR_ARG
    assert L.ctag_track_filter_create(detector.h, rigs.r, None, None) == capi.ERR_ARG
    assert L.ctag_track_filter_create(None, rigs.r, None, C.byref(C.c_void_p())) == capi.ERR_ARG
    st, f = create(detector, rigs, None)     # opts == NULL: the defaults
    assert st == 0
    try:
        p, q, o = P.ctypes.data, Q.ctypes.data, out.ctypes.data
        step = L.ctag_rig_track_filter
        for args in ((None, p, q, 2, None, o), (f, None, q, 2, None, o), (f, p, None, 2, None, o), (f, p, q, 2, None, None), (f, p, q, 0, None, o)):
            assert step(*args) == capi.ERR_ARG
        assert L.ctag_rig_track_filter_device(f, 1, 1, capi.TRACK_MAX_ITEMS // 2 + 1, None, 1) == capi.ERR_ARG   # refused before anything is read
        for bad in ([0.1, 0.1], [0.2, 0.1], [float("nan"), 1.0], [0.1, float("inf")]):
            t = np.array(bad)
            assert step(f, p, q, 2, t.ctypes.data, o) == capi.ERR_ARG
        t = np.array([0.5, 0.6])
        assert step(f, p, q, 2, t.ctypes.data, o) == 0
        first = out.copy()
        for bad in ([0.6, 0.7], [0.3, 0.9]):   # a time that does not exceed the last one given
            t = np.array(bad)
            assert step(f, p, q, 2, t.ctypes.data, o) == capi.ERR_ARG
        assert L.ctag_track_filter_predict(f, 0.6, o) == capi.ERR_ARG and L.ctag_track_filter_predict(f, float("nan"), o) == capi.ERR_ARG
        assert L.ctag_track_filter_predict(f, 0.7, None) == capi.ERR_ARG and L.ctag_track_filter_predict_device(None, 0.7, 1) == capi.ERR_ARG
        assert step(f, p, q, 2, None, o) == capi.ERR_ARG   # times == NULL would give (2 + f) dt = 0.067, 0.1: not above 0.6
        # a refused call changed nothing: the next frames continue the track
        t = np.array([0.7, 0.8])
        assert step(f, p, q, 2, t.ctypes.data, o) == 0
        assert (out["status"] == fs.OK).all() and not (out["flags"] & fs.FLAG_STARTED).any() and (first["flags"][:2] & fs.FLAG_STARTED).any()
        assert L.ctag_track_filter_reset(None) == capi.ERR_ARG and L.ctag_track_filter_last_ms(f, None) == capi.ERR_ARG
    finally:
        L.ctag_track_filter_free(f)
    L.ctag_track_filter_free(None)


def test_closing_the_detector_closes_its_filters_first(dictionary):
    """a filter's state hangs on the handle: Detector.close frees the filters it made that are still open, and their own close (or
    collection) afterwards touches nothing"""
    import testkit as tk
    state, fsize = dictionary
    det = tk.Detector(state, fsize, device=0)
    b = fsh.batch("n2")
    kept, closed = fsh.DeviceFilter(det, b), fsh.DeviceFilter(det, b)
    closed.close()
    assert det._filters == [kept.f]
    first = kept.run(b)
    det.close()
    assert kept.f.f is None and det._filters == [] and det.h is None
    kept.close()
    assert (first["status"][1] == fs.OK).all()


def test_timing_slot(detector):
    detector.set_option(capi.OPT_TIMING, 1)
    try:
        b = fsh.batch("n64")
        with fsh.DeviceFilter(detector, b) as F:
            F.run(b)
            assert F.f.track_filter_last_ms() > 0
    finally:
        detector.set_option(capi.OPT_TIMING, 0)


def test_live_loop_end_to_end(detector, dictionary):
    """rendered frames -> detect -> rig pose -> covariance -> filter: a step enqueued directly behind the pose and covariance kernels of its
    frame, nothing waited for in between, gives the bytes of the loop that waits after every call, and of the batch call on all frames"""
    import torch
    import testkit as tk
    import cylindertag_amd as ca
    from dense_testlib import COLS, K_PLANTED, ROWS
    state, _ = dictionary
    n = 6
    M, _ = tk.synth3d_model(state)
    K = K_PLANTED.copy()
    K[0, 2] -= 0.5
    K[1, 2] -= 0.5
    cam = ca.make_camera(K, np.zeros(5))
    nr = state.shape[0]
    rigs = ca.Rigs(M, np.arange(nr, dtype=np.int32))
    frames = torch.empty((n, ROWS, COLS), dtype=torch.uint8, device="cuda")
    detector.synth3d_frames_device(frames.data_ptr(), 0, n, ROWS, COLS, COLS, ROWS * COLS, K_PLANTED)
    res = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    poses = torch.zeros((n, nr * ca.RIG_POSE_DT.itemsize), dtype=torch.uint8, device="cuda")
    covs = torch.zeros((n, nr * ca.POSE_COV_DT.itemsize), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, nr * capi.TRACK_DT.itemsize), dtype=torch.uint8, device="cuda")
    detector.sync()

    def loop(wait):
        out.zero_()
        torch.cuda.synchronize()
        F = detector.track_filter(rigs, None)
        try:
            for f in range(n):
                detector.detect_batch_device(frames[f].data_ptr(), 1, ROWS, COLS, COLS, ROWS * COLS, res[f].data_ptr(), 5, True, 5)
                wait()
                detector.rig_pose_batch_device(res[f].data_ptr(), 1, M, rigs, cam, poses[f].data_ptr())
                wait()
                detector.rig_pose_cov_batch_device(res[f].data_ptr(), 1, M, rigs, cam, poses[f].data_ptr(), covs[f].data_ptr())
                wait()
                F.step_device(poses[f].data_ptr(), covs[f].data_ptr(), out[f].data_ptr())
                wait()
            detector.sync()
        finally:
            F.close()
        return out.cpu().numpy().view(capi.TRACK_DT).reshape(n, nr).copy()

    waited = loop(detector.sync)
    enqueued = loop(lambda: None)
    assert enqueued.tobytes() == waited.tobytes()
    tracked = waited["status"][-1] == fs.OK   # four objects a frame
    assert tracked.sum() >= 3 and ((waited["flags"][:, tracked] & fs.FLAG_STARTED) != 0).sum(0).min() >= 1
    # the batch: every frame's records in one call of each kind
    detector.detect_batch_device(frames.data_ptr(), n, ROWS, COLS, COLS, ROWS * COLS, res.data_ptr(), 5, True, 5)
    detector.rig_pose_batch_device(res.data_ptr(), n, M, rigs, cam, poses.data_ptr())
    detector.rig_pose_cov_batch_device(res.data_ptr(), n, M, rigs, cam, poses.data_ptr(), covs.data_ptr())
    F = detector.track_filter(rigs, None)
    try:
        F.step_device(poses.data_ptr(), covs.data_ptr(), out.data_ptr(), n_frames=n)
        detector.sync()
    finally:
        F.close()
    batch = out.cpu().numpy().view(capi.TRACK_DT).reshape(n, nr)
    assert body(batch) == body(waited)
