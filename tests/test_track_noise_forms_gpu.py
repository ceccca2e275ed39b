"""The track noise fit's calls (include/ctag_pose.h, track noise fit): what rule 9 promises byte for byte, every status, the EDGE flag,
every CTAG_ERR_ARG, the device forms' writes, calls of different sizes behind one another, and ctag_track_filter_set_cov_scale."""
import ctypes as C

import numpy as np
import pytest

import track_filter_shapes as fsh
import track_filter_statement as fs
import track_noise_shapes as nsh
import track_noise_statement as ns
import track_shapes as sh
from cylindertag_amd import capi

pytestmark = pytest.mark.gpu

FAST = dict(free_mask=3, rounds=3)


def body(rec):
    r = np.atleast_1d(rec).copy()   # (np.array(copy=True) of one record of a structured array still shares its memory)
    r["rig"] = 0
    return r.tobytes()


def test_per_rig_bytes_do_not_depend_on_the_other_rigs(detector):
    b = nsh.batch("planted_s4")
    rec, trace = nsh.device_fit(detector, b, **FAST)
    assert (rec["rig"] == [0, 1, 2]).all() and (rec["status"] == capi.NOISE_OK).all()
    perm = [2, 0, 1]
    prec, ptrace = nsh.device_fit(detector, nsh.select_rigs(b, perm), **FAST)
    for new, old in enumerate(perm):
        assert body(prec[new]) == body(rec[old]) and ptrace[new].tobytes() == trace[old].tobytes()
    one, otrace = nsh.device_fit(detector, nsh.select_rigs(b, [1]), **FAST)
    assert body(one[0]) == body(rec[1]) and otrace[0].tobytes() == trace[1].tobytes()
    # the pooled search of one rig is the per-rig search
    pooled, pt = nsh.device_fit(detector, nsh.select_rigs(b, [1]), mode=ns.POOLED, **FAST)
    assert pooled["rig"][0] == -1 and body(pooled[0]) == body(rec[1]) and pt[0].tobytes() == trace[1].tobytes()
    again, _ = nsh.device_fit(detector, b, **FAST)
    assert again.tobytes() == rec.tobytes()


def test_bad_input_too_few_and_singular(detector):
    b = nsh.batch("bad_rig")
    rec, trace = nsh.device_fit(detector, b, free_mask=1, rounds=2)
    assert list(rec["status"]) == [capi.NOISE_OK, capi.NOISE_BAD_INPUT, capi.NOISE_OK]
    bad = rec[1]
    assert (bad["q_rot"], bad["q_trans"], bad["cov_scale"]) == tuple(nsh.start_of(b)) and bad["rounds"] == 0 and bad["n_terms"] == 0
    assert (trace["winner"][1] == -1).all() and not trace["L"][1].any()
    pooled, _ = nsh.device_fit(detector, b, free_mask=1, rounds=2, mode=ns.POOLED)
    assert pooled["status"][0] == capi.NOISE_OK and pooled["n_terms"][0] == rec["n_terms"][0] + rec["n_terms"][2]
    want = ns.fit(b, free_mask=1, rounds=2, mode=ns.POOLED)[0][0]
    assert pooled["q_rot"][0] == want["q_rot"] and nsh.per_term(pooled["score"][0], want["score"], want["n_terms"]) <= ns.BAR["L"]
    only_bad, _ = nsh.device_fit(detector, dict(nsh.select_rigs(b, [1]), rec_rig=b["rec_rig"][:, [0]] + 1), mode=ns.POOLED, rounds=1)
    assert only_bad["status"][0] == capi.NOISE_BAD_INPUT and only_bad["rig"][0] == -1
    # too few updates at the start values: two frames give one
    rec, trace = nsh.device_fit(detector, nsh.batch("n2"), rounds=2)
    sc = nsh.device_score(detector, nsh.batch("n2"), nsh.start_of(nsh.batch("n2"))[None, :])[0]
    for g in range(2):
        R = rec[g]
        assert R["status"] == capi.NOISE_TOO_FEW and R["rounds"] == 1 and R["n_terms"] == sc["n_terms"][g] < 8
        assert (R["q_rot"], R["q_trans"], R["cov_scale"]) == tuple(nsh.start_of(nsh.batch("n2"))) and R["score"] == R["score_start"] == sc["L"][g]
    assert (trace["winner"] == -1).all()
    rec = nsh.device_fit(detector, nsh.batch("n2"), rounds=2, min_terms=1, trace=False)
    assert rec["status"][0] == capi.NOISE_OK and rec["n_terms"][0] == 1
    # every candidate singular: the scale fixed where s * cov_f overflows
    b = nsh.batch("overflow")
    rec, trace = nsh.device_fit(detector, b, free_mask=3, rounds=3, cov_scale=2.0 ** 11, min_terms=4)
    assert list(rec["status"]) == [capi.NOISE_SINGULAR, capi.NOISE_OK] and rec["rounds"][0] == 1 and (trace["winner"][0] == -1).all()
    assert (rec["q_rot"][0], rec["q_trans"][0], rec["cov_scale"][0]) == tuple(nsh.start_of(b, cov_scale=2.0 ** 11))
    # some candidates singular: the search stays among the others
    rec = nsh.device_fit(detector, nsh.select_rigs(b, [0]), free_mask=4, rounds=3, cov_scale=2.0 ** 9, span=8.0, trace=False)
    assert rec["status"][0] == capi.NOISE_OK and rec["cov_scale"][0] <= 2.0 ** 10


def test_edge_flag(detector):
    """span 1 around a start 8 octaves above the planted q_rot: the winner of every round lies at k = -2"""
    b = nsh.select_rigs(nsh.batch("planted_s1"), [0])
    rec, trace = nsh.device_fit(detector, b, free_mask=1, rounds=3, span=1.0, q_rot=b["planted"][0] * 2.0 ** 8, q_trans=b["planted"][1], cov_scale=1.0)
    R = rec[0]
    assert R["status"] == capi.NOISE_OK and R["flags"] == capi.NOISE_FLAG_EDGE << 0 and R["log2_sigma"][0] == 0.0 and (trace["winner"][0] == 0).all()
    assert trace["u"][0, -1, 0] == -2 * (0.5 + 0.25 + 0.125)


def test_every_err_arg(detector):
    b = nsh.batch("n65")
    P, Q = sh.to_records(b)
    rigs = sh.RigSet(b["n_rigs"])
    L, h, nf = detector.L, detector.h, b["n_frames"]
    out, tr = np.zeros(2, capi.TRACK_NOISE_DT), np.zeros(32, capi.TRACK_NOISE_ROUND_DT)
    sc, cand = np.zeros(64 * 2, capi.TRACK_NOISE_SCORE_DT), np.tile(nsh.start_of(b), (65, 1))
    out[:] = np.frombuffer(b"\xA5" * out.nbytes, capi.TRACK_NOISE_DT)
    before = out.tobytes()

    def fit(opts=None, recs=P.ctypes.data, cov=Q.ctypes.data, n_frames=nf, times=None, o=out.ctypes.data, r=rigs.r, hh=h):
        return L.ctag_rig_track_noise_fit(hh, r, recs, cov, n_frames, times, C.byref(opts) if opts is not None else None, o, tr.ctypes.data)

    def score(n_cand, c=cand, opts=None):
        return L.ctag_rig_track_noise_score(h, rigs.r, P.ctypes.data, Q.ctypes.data, nf, None, C.byref(opts) if opts is not None else None, c.ctypes.data, n_cand,
                                            sc.ctypes.data)

    assert fit(nsh.noise_opts_c(b, rounds=1)) == 0
    out[:] = np.frombuffer(before, capi.TRACK_NOISE_DT)
    for bad in (dict(struct_size=72), dict(mode=2), dict(mode=-1), dict(free_mask=8), dict(free_mask=-1), dict(rounds=0), dict(rounds=17), dict(min_terms=0),
                dict(max_gap=0), dict(span=0.0), dict(span=-1.0), dict(span=np.inf), dict(span=np.nan), dict(dt=0.0), dict(q_rot=0.0), dict(q_trans=-1.0),
                dict(cov_scale=0.0), dict(cov_scale=np.inf), dict(vel0_sigma_rot=0.0), dict(vel0_sigma_trans=np.nan)):
        o = nsh.noise_opts_c(b)
        for k, v in bad.items():
            setattr(o, k, v)
        assert fit(o) == -1, bad
        assert score(1, opts=o) == -1, bad
    assert fit(recs=None) == -1 and fit(cov=None) == -1 and fit(o=None) == -1 and fit(r=None) == -1 and fit(hh=None) == -1 and fit(n_frames=0) == -1
    t = np.arange(nf) / 30.0
    t[7] = t[6]
    assert fit(times=t.ctypes.data) == -1
    t[7] = np.nan
    assert fit(times=t.ctypes.data) == -1
    assert score(0) == -1 and score(65) == -1 and score(64) == 0
    for v in (0.0, -1.0, np.inf, np.nan):
        c = cand.copy()
        c[3, 1] = v
        assert score(5, c) == -1
    assert L.ctag_rig_track_noise_score(h, rigs.r, P.ctypes.data, Q.ctypes.data, nf, None, None, None, 1, sc.ctypes.data) == -1
    assert out.tobytes() == before   # a refused call writes nothing
    assert fit(n_frames=capi.TRACK_MAX_ITEMS // 2 + 1) == -1   # n_frames x n_rigs above the bound: refused before a record is read
    assert L.ctag_track_noise_last_ms(h, None) == -1


def test_device_forms_write_no_byte_outside_their_outputs(detector):
    import torch
    b = nsh.batch("gaps")
    P, Q = sh.to_records(b)
    nr, rounds, GUARD = b["n_rigs"], 3, 4096
    dP, dQ = torch.from_numpy(P.view(np.uint8)).cuda(), torch.from_numpy(Q.view(np.uint8)).cuda()
    sizes = (nr * capi.TRACK_NOISE_DT.itemsize, nr * rounds * capi.TRACK_NOISE_ROUND_DT.itemsize, 5 * nr * capi.TRACK_NOISE_SCORE_DT.itemsize)
    bufs = [torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    rigs, opts = sh.RigSet(nr), nsh.noise_opts_c(b, free_mask=5, rounds=rounds)
    cands = nsh.candidates("gaps")[:5]
    # the fit, the score call and a fit without a trace enqueued behind one another, nothing waited for in between
    detector.fit_track_noise_device(rigs, dP.data_ptr(), dQ.data_ptr(), b["n_frames"], bufs[0].data_ptr() + GUARD, bufs[1].data_ptr() + GUARD, times=b["times"], opts=opts)
    detector.score_track_noise_device(rigs, dP.data_ptr(), dQ.data_ptr(), b["n_frames"], cands, bufs[2].data_ptr() + GUARD, times=b["times"], opts=opts)
    detector.sync()
    host = [x.cpu().numpy() for x in bufs]
    for x, n in zip(host, sizes):
        assert (x[:GUARD] == 0xA5).all() and (x[GUARD + n:] == 0xA5).all()
    rec, trace = nsh.device_fit(detector, b, free_mask=5, rounds=rounds)
    assert host[0][GUARD:GUARD + sizes[0]].tobytes() == rec.tobytes() and host[1][GUARD:GUARD + sizes[1]].tobytes() == trace.tobytes()
    assert host[2][GUARD:GUARD + sizes[2]].tobytes() == nsh.device_score(detector, b, cands).tobytes()
    # trace == NULL is allowed and changes no record
    bufs[0].fill_(0xA5)
    detector.fit_track_noise_device(rigs, dP.data_ptr(), dQ.data_ptr(), b["n_frames"], bufs[0].data_ptr() + GUARD, None, times=b["times"], opts=opts)
    detector.sync()
    x = bufs[0].cpu().numpy()
    assert x[GUARD:GUARD + sizes[0]].tobytes() == rec.tobytes() and (x[:GUARD] == 0xA5).all() and (x[GUARD + sizes[0]:] == 0xA5).all()


def test_smaller_call_after_a_larger_one_and_calls_back_to_back(detector):
    import torch
    big, small = nsh.batch("planted_s1"), nsh.batch("n63")
    want_small = nsh.device_fit(detector, small, **FAST)[0]
    want_big = nsh.device_fit(detector, big, free_mask=7, rounds=2)[0]     # 125 candidates x 3 rigs
    assert nsh.device_fit(detector, small, **FAST)[0].tobytes() == want_small.tobytes()   # ... then 25 x 2 in the same workspace
    # two device calls back to back on different batches, each with its own times array overwritten as soon as the call returns
    outs = []
    for b, over in ((big, dict(free_mask=7, rounds=2)), (small, FAST)):
        P, Q = sh.to_records(b)
        outs.append((torch.from_numpy(P.view(np.uint8)).cuda(), torch.from_numpy(Q.view(np.uint8)).cuda(),
                     torch.zeros(b["n_rigs"] * capi.TRACK_NOISE_DT.itemsize, dtype=torch.uint8, device="cuda"), b, over))
    torch.cuda.synchronize()
    for dP, dQ, out, b, over in outs:
        t = np.arange(b["n_frames"]) * ns.noise_opts(b)["dt"]
        detector.fit_track_noise_device(sh.RigSet(b["n_rigs"]), dP.data_ptr(), dQ.data_ptr(), b["n_frames"], out.data_ptr(), times=t, opts=nsh.noise_opts_c(b, **over))
        t[:] = -1.0
    detector.sync()
    got = [np.frombuffer(o[2].cpu().numpy().tobytes(), capi.TRACK_NOISE_DT) for o in outs]
    for g, w in zip(got, (want_big, want_small)):   # times given as f * dt in float64 are the times of times == NULL
        assert g.tobytes() == w.tobytes()


def test_mv_records(detector):
    b = nsh.batch("mv")
    rec = nsh.device_fit(detector, b, trace=False, **FAST)
    as_rig = nsh.device_fit(detector, dict(b, kind="rig"), trace=False, **FAST)
    assert (rec["status"] == capi.NOISE_OK).all() and rec.tobytes() == as_rig.tobytes()


def test_apply_track_noise(detector):
    rec = nsh.device_fit(detector, nsh.select_rigs(nsh.batch("planted_s4"), [0]), trace=False, **FAST)
    o, s = capi.apply_track_noise(rec, gate=5.0)
    assert (o.q_rot, o.q_trans, o.gate, s) == (rec["q_rot"][0], rec["q_trans"][0], 5.0, rec["cov_scale"][0])
    with pytest.raises(ValueError):
        capi.apply_track_noise(np.zeros(2, capi.TRACK_NOISE_DT))


# ---- ctag_track_filter_set_cov_scale -----------------------------------------------------------------------------------------------------------
def scaled(b, s):
    return dict(b, cov=b["cov"] * s)


@pytest.mark.parametrize("name", ("gaps", "huber", "gated_run"))
def test_cov_scale_one_and_four(detector, name):
    b = fsh.batch(name)
    plain = fsh.device_run(detector, b)
    with fsh.DeviceFilter(detector, b) as F:
        F.f.set_cov_scale(1.0)
        assert F.run(b).tobytes() == plain.tobytes()
    with fsh.DeviceFilter(detector, b) as F:
        F.f.set_cov_scale(4.0)
        four = F.run(b)
    assert four.tobytes() == fsh.device_run(detector, scaled(b, 4.0)).tobytes() and four.tobytes() != plain.tobytes()


def test_cov_scale_against_the_filter_statement(detector):
    b = fsh.batch("gaps")
    with fsh.DeviceFilter(detector, b) as F:
        F.f.set_cov_scale(2.5)
        rec = F.run(b)
    # the statement on records whose cov is 2.5 x: rule 1 is scale-free, so measured and bad input are those of cov itself
    fsh.check_against(rec, fs.run_batch(scaled(b, 2.5)), "gaps x 2.5")


def test_refused_cov_scale_changes_nothing(detector):
    b = fsh.batch("n65")
    with fsh.DeviceFilter(detector, b) as F:
        F.f.set_cov_scale(4.0)
        for bad in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(capi.CtagError):
                F.f.set_cov_scale(bad)
        assert detector.L.ctag_track_filter_set_cov_scale(None, 1.0) == -1
        got = F.run(b)
    assert got.tobytes() == fsh.device_run(detector, scaled(b, 4.0)).tobytes()
