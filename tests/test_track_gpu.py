"""The track smoother end to end (include/ctag_pose.h, track smoothing): the full Levenberg-Marquardt loop against the statement's loop
and against the statement's scipy minimum, rig against multi-view records, bad input, and every CTAG_ERR_ARG of the options."""
import ctypes as C

import numpy as np
import pytest

import track_shapes as sh
import track_statement as ts
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

smooth = sh.device_smooth


@pytest.mark.parametrize("name", sh.SMALL)
def test_full_lm_matches_statement(detector, name):
    rec, stat = smooth(detector, sh.batch(name))
    sh.check_against(rec, stat, sh.full_lm(name), name + " LM")


@pytest.mark.parametrize("name", sh.SCIPY_BATCHES)
def test_full_lm_reaches_scipy_minimum(detector, name):
    """the distance to scipy's minimum of the same cost, in units of the smoothed cov, within 16 x what the statement's own loop is off it"""
    rec, stat = smooth(detector, sh.batch(name))
    want, wstat, _ = sh.scipy_min(name)
    dev = ts.deviation(sh.as_dict(rec), want)
    print(name, "to scipy", {k: "%.3g" % v for k, v in dev.items()})
    assert max(dev["pose"], dev["vel"]) <= ts.SCIPY_BAR
    assert (stat["cost"] <= wstat["cost"] * (1 + 1e-9)).all()


def test_planted_gross_error_is_downweighted(detector):
    for name in ("huber", "cauchy"):
        b = sh.batch(name)
        rec, _ = smooth(detector, b)
        f, g = b["planted"]
        assert rec["flags"][f, g] == capi.TRACK_FLAG_MEASURED | capi.TRACK_FLAG_DOWNWEIGHTED and rec["weight"][f, g] < 0.5
        assert rec["mahalanobis2"][f, g] > 64   # the loss leaves it at least 8 sigma off: a weight below 4 / 8


def test_rig_and_multi_view_records_give_the_same_bytes(detector):
    """one camera at the reference: the multi-view record's pose is the rig record's, and so is every byte of the result"""
    b = sh.batch("gaps")
    a, sa = smooth(detector, b)
    m, sm = smooth(detector, dict(b, kind="mv"))
    assert a.tobytes() == m.tobytes() and sa.tobytes() == sm.tobytes()


def test_bad_input(detector):
    b = sh.batch("noise")
    clean, cstat = smooth(detector, b)
    for what in ("rvec_param", "rig_field", "frame_field"):
        c = dict(b)
        for k in ("cov_param", "rec_rig", "rec_frame"):
            c[k] = np.array(b[k], copy=True)
        if what == "rvec_param":
            c["cov_param"][7, 1] = capi.COV_PARAM_RVEC
        elif what == "rig_field":
            c["rec_rig"][9, 1] = 0
        else:
            c["rec_frame"][9, 1] = 8
        rec, stat = smooth(detector, c)
        assert list(stat["status"]) == [capi.TRACK_OK, capi.TRACK_BAD_INPUT, capi.TRACK_OK]
        assert (rec["status"][:, 1] == capi.TRACK_BAD_INPUT).all()
        assert (rec["rig"][:, 1] == 1).all() and (rec["frame"][:, 1] == np.arange(b["n_frames"])).all()
        for k in sh.FIELDS[1:]:
            assert not rec[k][:, 1].any(), k
        for k in ("n_measured", "n_pieces", "n_tracked", "longest_piece", "rounds", "cost0", "cost"):
            assert stat[k][1] == 0
        # the other rigs are what they were
        assert rec[:, 0].tobytes() == clean[:, 0].tobytes() and rec[:, 2].tobytes() == clean[:, 2].tobytes()
        assert stat[0].tobytes() == cstat[0].tobytes()
    # an RVEC covariance whose status is not OK is just an unmeasured frame
    c = dict(b, cov_param=np.array(b["cov_param"], copy=True), cov_status=np.array(b["cov_status"], copy=True))
    c["cov_param"][7, 1], c["cov_status"][7, 1] = capi.COV_PARAM_RVEC, capi.COV_SINGULAR
    rec, stat = smooth(detector, c)
    assert stat["status"][1] == capi.TRACK_OK and rec["flags"][7, 1] == 0 and rec["status"][7, 1] == capi.TRACK_OK


BAD_OPTS = [dict(struct_size=76), dict(loss=3), dict(loss=-1), dict(max_iterations=0), dict(max_gap=0), dict(segment_frames=12), dict(segment_frames=128),
            dict(segment_frames=-8), dict(lambda0=-1e-3), dict(lambda0=float("nan"))]
for _k in ("dt", "q_rot", "q_trans", "vel0_sigma_rot", "vel0_sigma_trans", "loss_scale"):
    BAD_OPTS += [{_k: 0.0}, {_k: -1.0}, {_k: float("inf")}, {_k: float("nan")}]


def call(det, b, opts, times=None, n_frames=None):
    P, Q = sh.to_records(b)
    rigs = sh.RigSet(b["n_rigs"])
    nf = b["n_frames"] if n_frames is None else n_frames
    out, stat = np.zeros(len(P), capi.TRACK_DT), np.zeros(b["n_rigs"], capi.TRACK_STAT_DT)
    return det.L.ctag_rig_track_smooth(det.h, rigs.r, P.ctypes.data, Q.ctypes.data, nf, None if times is None else times.ctypes.data,
                                       C.byref(opts) if opts is not None else None, out.ctypes.data, stat.ctypes.data)


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_every_bad_option_alone_is_err_arg(detector, bad):
    b = sh.batch("huber")
    assert call(detector, b, sh.track_opts(b)) == 0
    assert call(detector, b, sh.track_opts(b, **bad)) == capi.ERR_ARG


def test_bad_times_and_sizes_are_err_arg(detector):
    b = sh.batch("huber")
    n = b["n_frames"]
    t = np.arange(n) * 0.04
    assert call(detector, b, None, times=t) == 0          # opts == NULL: the defaults
    for f, v in ((5, t[4]), (5, t[3]), (0, float("nan")), (n - 1, float("inf"))):
        bad = t.copy()
        bad[f] = v
        assert call(detector, b, None, times=bad) == capi.ERR_ARG
    assert call(detector, b, None, n_frames=0) == capi.ERR_ARG
    # n_frames x n_rigs above the bound: refused before anything is read
    rigs = sh.RigSet(2)
    assert detector.L.ctag_rig_track_smooth_device(detector.h, rigs.r, 1, 1, capi.TRACK_MAX_ITEMS // 2 + 1, None, None, 1, 1) == capi.ERR_ARG


def test_timing_slots(detector):
    detector.set_option(capi.OPT_TIMING, 1)
    try:
        smooth(detector, sh.batch("noise"))
        ms = detector.track_last_ms()
        assert ms["total"] > 0 and abs(ms["setup"] + ms["rounds"] + ms["marginals"] - ms["total"]) < 0.05 * ms["total"] + 0.01
    finally:
        detector.set_option(capi.OPT_TIMING, 0)
