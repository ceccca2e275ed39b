"""The batches the track smoother is held to (tests/track_statement.py says what a batch is).  All are small: the hazard is in the
structure -- piece lengths on each side of every segment length, gaps at the bridging limit, separators that fall into gaps -- not in the
size.  Every trajectory is drawn from the model itself: velocities from the prior, motion from white noise on acceleration with the
batch's q, measurements with noise from the batch's own covariances, so that the estimate is calibrated by construction."""
import functools

import numpy as np

import track_statement as ts

POSE_NOT_SEEN, COV_NO_POSE, COV_SINGULAR = 5, 1, 3
BASE_OPTS = dict(q_rot=0.5, q_trans=0.02, vel0_sigma_rot=1.0, vel0_sigma_trans=0.3, dt=1.0 / 30.0, max_gap=4)
PIECE_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 129, 200)


def runs_mask(n_frames, first, lengths, gap):
    """measured flags: runs of the given lengths from frame `first`, `gap` unmeasured frames between them"""
    m = np.zeros(n_frames, bool)
    f = first
    for n in lengths:
        assert f + n <= n_frames
        m[f:f + n] = True
        f += n + gap
    return m


def cov_of(rng, kind):
    """a 6x6 covariance as the covariance call returns them: 'good' like a rig of 800 points, 'weak' like a lone 4-point marker (large,
    strongly correlated, ill-scaled between rotation and translation)"""
    if kind == "good":
        sig = np.array([4e-4] * 3 + [2e-4] * 3) * rng.uniform(0.7, 1.4, 6)
        A = np.eye(6) + 0.2 * rng.standard_normal((6, 6))
    else:
        sig = np.array([3e-2, 3e-2, 4e-3, 2e-3, 2e-3, 6e-2]) * rng.uniform(0.7, 1.4, 6)
        A = np.eye(6) + 0.1 * rng.standard_normal((6, 6))
        A[0, 4] = A[1, 3] = 2.5   # the rotation / translation ambiguity of a small marker
        A[4, 0] = A[3, 1] = 2.4
    C = A @ A.T
    d = 1.0 / np.sqrt(np.diag(C))
    C = C * np.outer(d, d)
    cov = C * np.outer(sig, sig)
    return 0.5 * (cov + cov.T)


def draw_track(rng, times, opts):
    """a trajectory from the model: (R [n, 3, 3], t [n, 3])"""
    n = len(times)
    R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    R[0] = ts.so3_exp(rng.uniform(-0.6, 0.6, 3))
    t[0] = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.2, 0.2, 3)
    w, v = rng.standard_normal(3) * opts["vel0_sigma_rot"], rng.standard_normal(3) * opts["vel0_sigma_trans"]
    for k in range(n - 1):
        dt = times[k + 1] - times[k]
        Q = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
        Lq = np.linalg.cholesky(Q)
        nr = (Lq @ rng.standard_normal((2, 3))) * np.sqrt(opts["q_rot"])
        nt = (Lq @ rng.standard_normal((2, 3))) * np.sqrt(opts["q_trans"])
        R[k + 1] = ts.so3_exp(dt * w + nr[0]) @ R[k]
        t[k + 1] = t[k] + dt * v + nt[0]
        w, v = w + nr[1], v + nt[1]
    return R, t


def make_batch(name, seed, n_frames, masks, kinds, opts=None, times=None, kind="rig", restart_at_pieces=True):
    """masks[g]: measured flags of rig g; kinds[g]: 'good', 'weak' or 'mixed'.  The truth restarts (a fresh draw from the prior) at every
    piece, so that pieces are independent samples."""
    rng = np.random.default_rng(seed)
    o = dict(BASE_OPTS)
    o.update(opts or {})
    full = dict(ts.DEFAULTS)
    full.update(o)
    n_rigs = len(masks)
    tt = np.arange(n_frames) * full["dt"] if times is None else np.asarray(times, np.float64)
    b = dict(name=name, kind=kind, n_frames=n_frames, n_rigs=n_rigs, times=None if times is None else tt, opts=o,
             pose_status=np.full((n_frames, n_rigs), POSE_NOT_SEEN, np.int32), rvec=np.zeros((n_frames, n_rigs, 3)), tvec=np.zeros((n_frames, n_rigs, 3)),
             cov_status=np.full((n_frames, n_rigs), COV_NO_POSE, np.int32), cov_param=np.zeros((n_frames, n_rigs), np.int32),
             cov=np.zeros((n_frames, n_rigs, 6, 6)), rec_rig=np.tile(np.arange(n_rigs, dtype=np.int32), (n_frames, 1)),
             rec_frame=np.tile(np.arange(n_frames, dtype=np.int32)[:, None], (1, n_rigs)),
             true_R=np.zeros((n_frames, n_rigs, 3, 3)), true_t=np.zeros((n_frames, n_rigs, 3)))
    for g in range(n_rigs):
        for a, e in ts.pieces(masks[g], full["max_gap"]):
            R, t = draw_track(rng, tt[a:e + 1], full)
            b["true_R"][a:e + 1, g], b["true_t"][a:e + 1, g] = R, t
            for f in range(a, e + 1):
                if not masks[g][f]:
                    continue
                k = kinds[g] if kinds[g] != "mixed" else ("weak" if rng.random() < 0.4 else "good")
                cov = cov_of(rng, k)
                eps = np.linalg.cholesky(cov) @ rng.standard_normal(6)
                b["pose_status"][f, g] = 0
                b["cov_status"][f, g] = 0
                b["cov"][f, g] = cov
                b["rvec"][f, g] = ts.so3_log(ts.so3_exp(eps[0:3]) @ R[f - a])
                b["tvec"][f, g] = t[f - a] + eps[3:6]
    return b


def plant_gross_error(b, f, g, n_sigma=30.0):
    """moves the measurement of (f, g) by n_sigma along the first axis of its covariance's Cholesky factor"""
    L = np.linalg.cholesky(b["cov"][f, g])
    eps = n_sigma * L[:, 0]
    R = ts.so3_exp(b["rvec"][f, g])
    b["rvec"][f, g] = ts.so3_log(ts.so3_exp(eps[0:3]) @ R)
    b["tvec"][f, g] = b["tvec"][f, g] + eps[3:6]
    b["planted"] = (f, g)


def _lengths():
    n = 260
    m0 = runs_mask(n, 2, (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33), 8)
    m1 = runs_mask(n, 5, (63, 64, 65), 9)
    m2 = runs_mask(n, 11, (200,), 0)
    m3 = runs_mask(n, 40, (129,), 0)
    m4 = np.zeros(n, bool)
    m5 = runs_mask(n, 77, (1,), 0)
    return make_batch("lengths", 11, n, [m0, m1, m2, m3, m4, m5], ["good", "mixed", "good", "weak", "good", "good"])


def _gaps():
    n, mg = 150, 4
    m0 = np.zeros(n, bool)
    m0[3:100] = True
    for lo in (10, 18, 34, 66):     # local frames 7-9, 15-17, 31-33, 63-65 of the piece that starts at 3: every separator of L = 8 .. 64 falls into a gap
        m0[lo:lo + 3] = False
    m1 = np.zeros(n, bool)          # index distances 2, max_gap - 1, max_gap (bridged) and max_gap + 1 (a new piece)
    f = 1
    for d in (1, 1, 2, 1, mg - 1, 1, 1, mg, 1, 1, mg + 1, 1, 1, 1, 2, 2, mg, mg, 1):
        m1[f] = True
        f += d
    m1[f] = True
    m2 = runs_mask(n, 20, (30, 40), mg)   # two runs exactly max_gap unmeasured frames apart: distance max_gap + 1, two pieces
    times = np.cumsum(np.random.default_rng(5).uniform(0.02, 0.05, n))
    b = make_batch("gaps", 12, n, [m0, m1, m2], ["good", "mixed", "weak"], opts=dict(max_gap=mg), times=times)
    # frames that have a pose but no usable covariance are unmeasured too
    b["pose_status"][101, 0] = 0
    b["cov_status"][101, 0] = COV_SINGULAR
    return b


def _noise():
    n = 48
    return make_batch("noise", 13, n, [runs_mask(n, 0, (48,), 0), runs_mask(n, 1, (45,), 0), runs_mask(n, 0, (48,), 0)], ["weak", "good", "mixed"])


def _mv():
    n = 40
    return make_batch("mv", 14, n, [runs_mask(n, 1, (20, 12), 6), runs_mask(n, 0, (40,), 0)], ["good", "mixed"], kind="mv")


def _robust(name, seed, loss):
    n = 44
    b = make_batch(name, seed, n, [runs_mask(n, 2, (40,), 0)], ["good"], opts=dict(loss=loss, loss_scale=4.0, max_iterations=30))
    plant_gross_error(b, 21, 0)
    return b


def _long():
    n = 4100
    m0 = np.ones(n, bool)
    m0[np.random.default_rng(6).random(n) < 0.15] = False
    m0[0] = m0[-1] = True
    m1 = runs_mask(n, 7, (2000, 1500, 500), 20)
    return make_batch("long", 17, n, [m0, m1], ["mixed", "good"], opts=dict(max_iterations=3))


BUILDERS = dict(lengths=_lengths, gaps=_gaps, noise=_noise, mv=_mv, huber=lambda: _robust("huber", 15, ts.LOSS_HUBER),
                cauchy=lambda: _robust("cauchy", 16, ts.LOSS_CAUCHY), long=_long)
BATCHES = tuple(BUILDERS)
SMALL = tuple(k for k in BATCHES if k != "long")


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
    return ts.smooth(with_opts(batch(name), max_iterations=1, lambda0=0.0), np.longdouble if longdouble else np.float64)


@functools.lru_cache(maxsize=None)
def full_lm(name, longdouble=False):
    return ts.smooth(batch(name), np.longdouble if longdouble else np.float64)


SCIPY_BATCHES = ("huber", "cauchy", "noise", "mv")


@functools.lru_cache(maxsize=None)
def scipy_min(name):
    """the statement's independent minimum (scipy.optimize.least_squares on rule 4's residual vector) of every piece of the batch"""
    return ts.smooth(batch(name), runner=ts.scipy_minimum)


def to_records(b):
    """the batch as the device sees it: (pose records, covariance records), record w = f * n_rigs + g"""
    from cylindertag_amd import capi
    dt = capi.MV_POSE_DT if b["kind"] == "mv" else capi.RIG_POSE_DT
    n = b["n_frames"] * b["n_rigs"]
    P, Q = np.zeros(n, dt), np.zeros(n, capi.POSE_COV_DT)
    P["status"], P["rig"], P["frame"] = b["pose_status"].reshape(-1), b["rec_rig"].reshape(-1), b["rec_frame"].reshape(-1)
    P["rvec"], P["tvec"] = b["rvec"].reshape(n, 3), b["tvec"].reshape(n, 3)
    Q["status"], Q["param"], Q["cov"] = b["cov_status"].reshape(-1), b["cov_param"].reshape(-1), b["cov"].reshape(n, 6, 6)
    return P, Q


class RigSet:
    """a rig set of n_rigs one-model rigs over a model made for it (the smoother only reads n_rigs)"""

    def __init__(self, n_rigs):
        from cylindertag_amd import capi
        self.model = capi.Model(ids=np.arange(n_rigs), corners=np.zeros((n_rigs, 8, 3)), model_size=1)
        self.rigs = capi.Rigs(self.model, np.arange(n_rigs, dtype=np.int32), n_rigs)
        self.r, self.n_rigs = self.rigs.r, n_rigs


def track_opts(b, **over):
    from cylindertag_amd import capi
    o = dict(b["opts"])
    o.update(over)
    return capi.track_opts(**o)


def device_smooth(det, b, **over):
    """the host form of the library on batch b -> (TRACK_DT [n_frames, n_rigs], TRACK_STAT_DT [n_rigs])"""
    P, Q = to_records(b)
    fn = det.smooth_mv_rig_track if b["kind"] == "mv" else det.smooth_rig_track
    return fn(RigSet(b["n_rigs"]), P, Q, b["n_frames"], times=b["times"], opts=track_opts(b, **over))


FIELDS = ("status", "flags", "rvec", "tvec", "w", "v", "cov", "vel_sigma", "mahalanobis2", "weight")


def as_dict(rec):
    return {k: rec[k] for k in FIELDS}


def check_against(rec, stat, want, label, bar=None):
    """every field of the library's records against the statement's (rec, stat, table): status, flags and counts exact, the rest within bar"""
    wrec, wstat, _ = want
    bar = ts.BAR if bar is None else bar
    assert (rec["status"] == wrec["status"]).all(), label
    assert (rec["flags"] == wrec["flags"]).all(), label
    for k in ("status", "n_measured", "n_pieces", "n_tracked", "longest_piece"):
        assert (stat[k] == wstat[k]).all(), (label, k)
    nf, nr = rec["status"].shape
    assert (rec["rig"] == np.arange(nr)[None, :]).all() and (rec["frame"] == np.arange(nf)[:, None]).all()
    assert (rec["cov"] == rec["cov"].transpose(0, 1, 3, 2)).all(), "cov is symmetric bit for bit"
    off = rec["status"] != ts.OK
    for k in FIELDS[2:]:
        assert not rec[k][off].any(), (label, k)
    dev = ts.deviation(as_dict(rec), wrec, wstat, {k: stat[k] for k in ("cost0", "cost")})
    print(label, {k: "%.3g" % v for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= bar[k], (label, k, v, bar[k])


@functools.lru_cache(maxsize=None)
def calibration_batch():
    """many short independent pieces (CPU test only): 16 rigs x 30 pieces of 8 frames"""
    n = 400
    masks = [runs_mask(n, g % 5, (8,) * 30, 5) for g in range(16)]
    return make_batch("calibration", 21, n, masks, ["good", "weak", "mixed", "mixed"] * 4)
