"""The batches the hand-eye fit is held to (tests/hand_eye_statement.py says what a batch is).  All but `long` and `chi2` are small: the
hazard is in the structure -- used-frame counts on each side of a chunk of 64, unused frames and a whole empty chunk, link rotations past
the start's 3 rad bound, motions that leave the problem singular -- not in the size.  Every batch plants P and Q, draws link poses,
composes A_f = P o C_f o Q and adds noise drawn from the frame's own covariance, so that the estimate is calibrated by construction."""
import functools

import numpy as np

import hand_eye_statement as hs
from track_shapes import RigSet, cov_of

POSE_NOT_SEEN, COV_NO_POSE = 5, 1


def rand_rot(rng, scale):
    return hs.so3_exp(rng.standard_normal(3) * scale)


def draw_links(rng, n, ang=0.6, kind="free"):
    """(rvec [n, 3], tvec [n, 3]) of link = base <- gripper"""
    rv = rng.standard_normal((n, 3)) * ang
    if kind == "bigangle":     # angles up to a half turn: many pairs with the first frame are past 3 rad
        ax = rng.standard_normal((n, 3))
        rv = ax / np.linalg.norm(ax, axis=1)[:, None] * rng.uniform(0.2, 3.1, n)[:, None]
    elif kind == "oneaxis":
        rv = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]) * (rng.standard_normal(n) * ang)[:, None]
    elif kind == "translate":
        rv = np.tile(np.array([0.2, 0.1, -0.3]), (n, 1))
    return rv, rng.standard_normal((n, 3)) * 0.3


def make_batch(name, seed, n_frames, masks, kinds, opts=None, kind="rig", links="free", cov_scale=None):
    """masks[g]: which frames of rig g have a pose and a covariance; kinds[g]: 'good', 'weak' or 'mixed' (track_shapes.cov_of);
    cov_scale[f]: a factor on frame f's sigmas"""
    rng = np.random.default_rng(seed)
    n_rigs = len(masks)
    o = dict(opts or {})
    lr, lt = draw_links(rng, n_frames, kind=links)
    b = dict(name=name, kind=kind, n_frames=n_frames, n_rigs=n_rigs, opts=o, links_rvec=lr, links_tvec=lt,
             pose_status=np.full((n_frames, n_rigs), POSE_NOT_SEEN, np.int32), rvec=np.zeros((n_frames, n_rigs, 3)), tvec=np.zeros((n_frames, n_rigs, 3)),
             cov_status=np.full((n_frames, n_rigs), COV_NO_POSE, np.int32), cov_param=np.zeros((n_frames, n_rigs), np.int32),
             cov=np.zeros((n_frames, n_rigs, 6, 6)), rec_rig=np.tile(np.arange(n_rigs, dtype=np.int32), (n_frames, 1)),
             rec_frame=np.tile(np.arange(n_frames, dtype=np.int32)[:, None], (1, n_rigs)),
             true_P=[], true_Q=[])
    C = hs.link_transforms(b, np.float64)
    for g in range(n_rigs):
        RP, tP = rand_rot(rng, 1.0), rng.standard_normal(3) * 0.1
        RQ, tQ = rand_rot(rng, 1.0), rng.standard_normal(3) * 0.3
        b["true_P"].append((RP, tP))
        b["true_Q"].append((RQ, tQ))
        for f in range(n_frames):
            if not masks[g][f]:
                continue
            RC, tC = C[f]
            R, t = RP @ RC @ RQ, RP @ (RC @ tQ + tC) + tP
            k = kinds[g] if kinds[g] != "mixed" else ("weak" if rng.random() < 0.4 else "good")
            cov = cov_of(rng, k)
            if cov_scale is not None:
                cov = cov * cov_scale[f] ** 2
            eps = np.linalg.cholesky(cov) @ rng.standard_normal(6)
            b["pose_status"][f, g] = 0
            b["cov_status"][f, g] = 0
            b["cov"][f, g] = cov
            b["rvec"][f, g] = hs.so3_log(hs.so3_exp(eps[0:3]) @ R)
            b["tvec"][f, g] = t + eps[3:6]
    return b


def subset(rng, n_frames, count):
    m = np.zeros(n_frames, bool)
    m[rng.choice(n_frames, count, replace=False)] = True
    return m


COUNTS = (2, 3, 4, 63, 64, 65, 129)


def _counts():
    n = 140
    rng = np.random.default_rng(100)
    return make_batch("counts", 31, n, [subset(rng, n, c) for c in COUNTS], ["good", "good", "weak", "mixed", "good", "weak", "mixed"])


def _long():
    n = 4100
    rng = np.random.default_rng(101)
    m0 = rng.random(n) > 0.1
    return make_batch("long", 32, n, [m0, np.ones(n, bool)], ["mixed", "good"], opts=dict(max_iterations=3))


def _holes():
    n = 200
    rng = np.random.default_rng(102)
    m0 = rng.random(n) > 0.3
    m0[0] = False              # the first frame is unused: k0 is a later one
    m0[64:128] = False         # a whole empty chunk
    m1 = rng.random(n) > 0.5
    m1[0:3] = False
    b = make_batch("holes", 33, n, [m0, m1], ["good", "mixed"])
    for f in (1, 5, 130, 131, 199):   # dropped by the caller: a link pose with a non-finite entry
        b["links_rvec"][f, f % 3] = np.nan if f % 2 else np.inf
    b["links_tvec"][140, 2] = np.nan
    b["pose_status"][150, 0] = 3      # a pose that failed, a covariance that did not come
    b["cov_status"][151, 1] = 3
    return b


def _simple(name, seed, n=24, links="free", **kw):
    return make_batch(name, seed, n, [np.ones(n, bool), np.ones(n, bool)], ["good", "mixed"], links=links, **kw)


def _illscaled():
    n = 30
    scale = 10.0 ** np.random.default_rng(103).uniform(0.0, 3.0, n)   # sigmas over 1e3: covariances over 1e6
    return make_batch("illscaled", 37, n, [np.ones(n, bool)], ["good"], cov_scale=scale)


def _robust(name, seed, loss):
    """2 of 40 frames carry a link pose that is wrong by 30 sigma of the frame's measurement.  loss_scale = 5: a good frame's squared
    Mahalanobis norm is chi-square(6) and exceeds 25 with probability 3.4e-4, so that the 38 good frames all stay inside the scale with
    probability 0.987 whatever the seed, while at the default 4 (1.4e-2 a frame) they would with probability 0.59 only."""
    n = 40
    b = make_batch(name, seed, n, [np.ones(n, bool)], ["good"], opts=dict(loss=loss, loss_scale=5.0, max_iterations=40))
    b["planted"] = (7, 29)
    for f in b["planted"]:
        L = np.linalg.cholesky(b["cov"][f, 0])
        eps = 30.0 * L[:, 0]
        b["links_rvec"][f] = hs.so3_log(hs.so3_exp(eps[0:3]) @ hs.so3_exp(b["links_rvec"][f]))
        b["links_tvec"][f] = b["links_tvec"][f] + 30.0 * np.sqrt(np.diag(b["cov"][f, 0])[3:6])
    return b


def _badinput():
    n = 20
    b = make_batch("badinput", 40, n, [np.ones(n, bool)] * 4, ["good"] * 4)
    b["cov_param"][7, 1] = 1          # RVEC
    b["rec_rig"][9, 2] = 0            # a misplaced rig field
    b["rec_frame"][11, 3] = 10        # a misplaced frame field
    return b


def _chi2():
    n, nr = 20, 200
    return make_batch("chi2", 42, n, [np.ones(n, bool)] * nr, ["good", "weak", "mixed", "mixed"] * (nr // 4))


BUILDERS = dict(counts=_counts, holes=_holes, bigangle=lambda: _simple("bigangle", 34, links="bigangle"),
                oneaxis=lambda: _simple("oneaxis", 35, links="oneaxis"), translate=lambda: _simple("translate", 36, links="translate"),
                illscaled=_illscaled, mv=lambda: _simple("mv", 38, kind="mv"), huber=lambda: _robust("huber", 39, hs.LOSS_HUBER),
                cauchy=lambda: _robust("cauchy", 41, hs.LOSS_CAUCHY), badinput=_badinput,
                mode1=lambda: _simple("mode1", 43, opts=dict(mode=hs.RIG_ON_LINK)), long=_long, chi2=_chi2)
BATCHES = tuple(BUILDERS)
SMALL = tuple(k for k in BATCHES if k != "long")
SINGULAR_BATCHES = ("oneaxis", "translate")
SCIPY_BATCHES = ("huber", "cauchy", "mode1", "mv", "illscaled")


@functools.lru_cache(maxsize=None)
def batch(name):
    return BUILDERS[name]()


def with_opts(b, **fields):
    """a shallow copy of the batch with option fields replaced"""
    c = dict(b)
    c["opts"] = dict(b["opts"], **fields)
    return c


@functools.lru_cache(maxsize=None)
def single_step(name, longdouble=False):
    """the statement's result for one undamped Gauss-Newton step from the start (computed once, shared by the tests)"""
    return hs.fit(with_opts(batch(name), max_iterations=1, lambda0=0.0), np.longdouble if longdouble else np.float64)


@functools.lru_cache(maxsize=None)
def full_lm(name, longdouble=False):
    return hs.fit(batch(name), np.longdouble if longdouble else np.float64)


@functools.lru_cache(maxsize=None)
def scipy_min(name):
    return hs.fit(batch(name), runner=hs.scipy_minimum)


def truth(b):
    """the planted transforms as the record fields of a result"""
    return dict(status=np.zeros(b["n_rigs"], np.int32), P_rvec=np.array([hs.so3_log(R) for R, _ in b["true_P"]]), P_tvec=np.array([t for _, t in b["true_P"]]),
                Q_rvec=np.array([hs.so3_log(R) for R, _ in b["true_Q"]]), Q_tvec=np.array([t for _, t in b["true_Q"]]))


def chi2_mean(rec, b):
    """the mean over the OK problems of delta^T cov^-1 delta, delta = the result's tangent distance from the planted transforms"""
    d = np.asarray(hs.tangent_difference(rec, truth(b)), np.float64)
    ok = np.asarray(rec["status"]) == hs.OK
    return float(np.mean([d[g] @ np.linalg.solve(np.asarray(rec["cov"][g], np.float64), d[g]) for g in np.nonzero(ok)[0]])), int(ok.sum())


CHI2_HALF_WIDTH = 5.0 * np.sqrt(24.0 / 200.0)    # five standard errors of the mean of 200 chi-square(12) draws


# ---- the library on a batch ------------------------------------------------------------------------------------------------------------------
def to_records(b):
    """the batch as the device sees it: (pose records, covariance records, link poses), record w = f * n_rigs + g"""
    from cylindertag_amd import capi
    dt = capi.MV_POSE_DT if b["kind"] == "mv" else capi.RIG_POSE_DT
    n = b["n_frames"] * b["n_rigs"]
    P, Q, K = np.zeros(n, dt), np.zeros(n, capi.POSE_COV_DT), np.zeros(b["n_frames"], capi.LINK_POSE_DT)
    P["status"], P["rig"], P["frame"] = b["pose_status"].reshape(-1), b["rec_rig"].reshape(-1), b["rec_frame"].reshape(-1)
    P["rvec"], P["tvec"] = b["rvec"].reshape(n, 3), b["tvec"].reshape(n, 3)
    Q["status"], Q["param"], Q["cov"] = b["cov_status"].reshape(-1), b["cov_param"].reshape(-1), b["cov"].reshape(n, 6, 6)
    K["rvec"], K["tvec"] = b["links_rvec"], b["links_tvec"]
    return P, Q, K


def he_opts(b, **over):
    from cylindertag_amd import capi
    o = dict(b["opts"])
    o.update(over)
    return capi.hand_eye_opts(**o)


def device_fit(det, b, frames=True, **over):
    """the host form of the library on batch b -> (HAND_EYE_DT [n_rigs], HAND_EYE_FRAME_DT [n_frames, n_rigs])"""
    P, Q, K = to_records(b)
    fn = det.fit_mv_hand_eye if b["kind"] == "mv" else det.fit_hand_eye
    return fn(RigSet(b["n_rigs"]), P, Q, b["n_frames"], K, opts=he_opts(b, **over), frames=frames)


def as_dicts(rec, frames):
    """the library's records in the statement's field names"""
    r = {k: rec[k] for k in ("status", "n_used", "n_downweighted", "rounds", "dof", "cost0", "cost", "sigma2_hat", "min_pivot", "cov")}
    r.update(P_rvec=rec["P"]["rvec"], P_tvec=rec["P"]["tvec"], Q_rvec=rec["Q"]["rvec"], Q_tvec=rec["Q"]["tvec"], lam=rec["lambda"])
    return r, (None if frames is None else {k: frames[k] for k in hs.FRAME_FIELDS})


def check_against(rec, frames, want, b, label, bar=None, rounds=True):
    """every field of the library's records against the statement's (rec, frames): statuses, flags and counts exact, the rest within bar"""
    wrec, wfr = want
    bar = hs.BAR if bar is None else bar
    got, gfr = as_dicts(rec, frames)
    assert (got["status"] == wrec["status"]).all(), (label, got["status"], wrec["status"])
    for k in ("n_used", "dof"):
        assert (got[k] == wrec[k]).all(), (label, k)
    ok = wrec["status"] == hs.OK
    if rounds:
        assert (got["rounds"][ok] == wrec["rounds"][ok]).all(), label
    assert (got["n_downweighted"][ok] == wrec["n_downweighted"][ok]).all(), label
    assert (rec["rig"] == np.arange(b["n_rigs"])).all()
    assert (rec["cov"] == rec["cov"].transpose(0, 2, 1)).all(), "cov is symmetric bit for bit"
    assert not rec["cov"][~ok].any(), "cov is 0 where the problem is not OK"
    none = np.isin(wrec["status"], (hs.TOO_FEW, hs.BAD_INPUT))
    for k in ("rounds", "dof", "P", "Q", "cost0", "cost", "lambda", "sigma2_hat", "min_pivot", "n_downweighted"):
        assert not rec[k][none].tobytes().strip(b"\0"), (label, k)
    if frames is not None:
        nf, nr = frames["status"].shape
        assert (frames["rig"] == np.arange(nr)[None, :]).all() and (frames["frame"] == np.arange(nf)[:, None]).all()
        assert (frames["flags"][:, ok] == wfr["flags"][:, ok]).all(), label
        assert (frames["status"][:, ok] == wfr["status"][:, ok]).all(), label
        unused = (frames["flags"] & hs.FLAG_USED) == 0
        for k in hs.FRAME_FIELDS:
            assert not frames[k][unused].any(), (label, k)
    dev = hs.deviation(got, wrec, gfr, wfr, hs.frame_sigma(b))
    print(label, {k: "%.3g" % v for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= bar[k], (label, k, v, bar[k])
