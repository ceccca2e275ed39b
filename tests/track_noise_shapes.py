"""The batches the track noise fit is held to (tests/track_noise_statement.py says what a batch is).  The small batches of
track_filter_shapes.py are reused as they are: frame counts on each side of the kernel's 64-frame pre-pass, gaps at the dropping limit,
the half turn, the spin, multi-view records, a bad rig beside good ones.  Added here:
  planted_s1 / planted_s4 / planted_times   3 rigs x 160 frames drawn from the model itself under PLANTED's q_rot and q_trans, measurements
                  drawn with covariance s_true * cov_f for s_true = 1 / 4 / 1, 8 % of the frames unmeasured, the last with non-uniform times;
                  the batch's own opts (the start values of a fit) lie some octaves off the planted values
  stride          64 candidates x 40 rigs x 8 frames, 2560 items: more than twice the 1024 blocks of a launch, so every block takes the
                  grid-stride loop.  The 40 rigs are ten copies of four, so the statement is needed for four
  overflow        one frame's covariance is so large that s * cov_f is not finite for the larger candidates' s: rule 4 gives SINGULAR there
                  and only there
Nothing longer than 200 frames goes into a fit."""
import functools

import numpy as np

import track_filter_shapes as fsh
import track_noise_statement as ns
import track_shapes as sh

REUSED = tuple("n%d" % n for n in fsh.EDGE_FRAMES) + ("gaps", "half_turn", "spin", "mv", "bad_rig")
PLANTED = dict(q_rot=0.004, q_trans=0.001)
PLANTED_START_U = np.array([3.0, -2.0, 1.0])   # log2(start / planted) of the planted batches' own opts
STRIDE_COPIES, STRIDE_DISTINCT = 10, 4

# 16 fixed candidates as octaves from a batch's start values, spread over +-12
CANDIDATE_U = np.array([[-12, -12, -12], [12, 12, 12], [-12, 12, 0], [12, -12, 4], [0, 0, 12], [0, 0, -12], [-7, 3, 1], [5, -9, -2],
                        [1.5, 2.5, -0.5], [-3.25, -1, 2], [8, 8, -6], [-8, -4, 6], [10, 0, 0], [0, -10, 0], [2, 11, 3], [-0.5, 0.5, 0.25]], np.float64)


def _planted(name, seed, s_true, nonuniform=False):
    n, nr = 160, 3
    rng = np.random.default_rng(seed)
    masks = [rng.random(n) >= 0.08 for _ in range(nr)]
    for m in masks:
        m[0] = True
    times = np.cumsum(rng.uniform(0.02, 0.05, n)) if nonuniform else None
    b = sh.make_batch(name, seed + 1, n, masks, ["good"] * nr, opts=dict(PLANTED, max_gap=5), times=times)
    b["cov"] = b["cov"] / s_true   # the measurements were drawn with s_true x the covariance the records now carry
    truth = np.array([PLANTED["q_rot"], PLANTED["q_trans"], float(s_true)])
    start = truth * np.exp2(PLANTED_START_U)
    b["planted"] = truth
    b["opts"] = dict(b["opts"], q_rot=start[0], q_trans=start[1], cov_scale=start[2])
    return b


def _stride():
    n = 8
    rng = np.random.default_rng(50)
    masks = [rng.random(n) < 0.85 for _ in range(STRIDE_DISTINCT)]
    d = sh.make_batch("stride", 51, n, masks, ["good", "weak", "mixed", "good"])
    nr = STRIDE_DISTINCT * STRIDE_COPIES
    b = dict(d, n_rigs=nr)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov", "true_R", "true_t"):
        b[k] = np.concatenate([d[k]] * STRIDE_COPIES, axis=1)   # rig g is distinct rig g % 4
    b["rec_rig"] = np.tile(np.arange(nr, dtype=np.int32), (n, 1))
    b["rec_frame"] = np.tile(np.arange(n, dtype=np.int32)[:, None], (1, nr))
    return b


def stride_distinct():
    """the four distinct rigs of `stride` as a batch of their own"""
    b = batch("stride")
    d = dict(b, n_rigs=STRIDE_DISTINCT)
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov", "true_R", "true_t", "rec_rig", "rec_frame"):
        d[k] = b[k][:, :STRIDE_DISTINCT]
    return d


def stride_candidates():
    """64 candidates for `stride`: a 4 x 4 x 4 grid of octaves around its start values"""
    o = ns.noise_opts(batch("stride"))
    g = np.array([-6.0, -1.5, 2.0, 7.0])
    U = np.array([[a, b_, c] for a in g for b_ in g for c in g])
    return np.array([o["q_rot"], o["q_trans"], o["cov_scale"]]) * np.exp2(U)


OVERFLOW_FRAME = 6


def _overflow(scale=1e305):
    n = 14
    b = sh.make_batch("overflow", 52, n, [np.ones(n, bool), np.ones(n, bool)], ["good", "good"])
    b["cov"] = np.array(b["cov"], copy=True)
    b["cov"][OVERFLOW_FRAME, 0] = b["cov"][OVERFLOW_FRAME, 0] * scale / b["cov"][OVERFLOW_FRAME, 0, 0, 0]   # s * cov overflows for s above about 2^10
    return b


BUILDERS = {k: functools.partial(fsh.batch, k) for k in REUSED}
BUILDERS.update(planted_s1=lambda: _planted("planted_s1", 60, 1.0), planted_s4=lambda: _planted("planted_s4", 62, 4.0),
                planted_times=lambda: _planted("planted_times", 64, 1.0, nonuniform=True), stride=_stride, overflow=_overflow)
BATCHES = tuple(BUILDERS)
PLANTED_BATCHES = ("planted_s1", "planted_s4", "planted_times")


@functools.lru_cache(maxsize=None)
def batch(name):
    return BUILDERS[name]()


def start_of(b, **over):
    o = ns.noise_opts(b, **over)
    return np.array([o["q_rot"], o["q_trans"], o["cov_scale"]])


def candidates(name):
    """the candidates a batch is scored at: its start values first, then the 16 fixed ones (`stride`: its own 64)"""
    if name == "stride":
        return stride_candidates()
    s = start_of(batch(name))
    return np.concatenate([s[None, :], s * np.exp2(CANDIDATE_U)])


@functools.lru_cache(maxsize=None)
def statement_scores(name, longdouble=False):
    """the statement's score of every (candidate, rig) of the batch: list over candidates of lists over rigs (computed once, shared; do
    not write into them).  `stride` is computed for its four distinct rigs and repeated."""
    T = np.longdouble if longdouble else np.float64
    b = stride_distinct() if name == "stride" else batch(name)
    out = ns.score_many(b, candidates(name), T)
    if name == "stride":
        out = [row * STRIDE_COPIES for row in out]
    return out


# ---- the library on a batch ------------------------------------------------------------------------------------------------------------------
OPT_FIELDS = ("mode", "free_mask", "rounds", "max_gap", "min_terms", "dt", "q_rot", "q_trans", "cov_scale", "vel0_sigma_rot", "vel0_sigma_trans", "span")


def noise_opts_c(b, **over):
    from cylindertag_amd import capi
    o = ns.noise_opts(b, **over)
    return capi.track_noise_opts(**{k: o[k] for k in OPT_FIELDS})


def device_score(det, b, cands, **over):
    """the host form of the score call -> TRACK_NOISE_SCORE_DT [n_cand, n_rigs]"""
    P, Q = sh.to_records(b)
    fn = det.score_mv_track_noise if b["kind"] == "mv" else det.score_track_noise
    return fn(sh.RigSet(b["n_rigs"]), P, Q, b["n_frames"], cands, times=b.get("times"), opts=noise_opts_c(b, **over))


def device_fit(det, b, trace=True, **over):
    """the host form of the fit -> (TRACK_NOISE_DT [searches], TRACK_NOISE_ROUND_DT [searches, rounds])"""
    P, Q = sh.to_records(b)
    fn = det.fit_mv_track_noise if b["kind"] == "mv" else det.fit_track_noise
    return fn(sh.RigSet(b["n_rigs"]), P, Q, b["n_frames"], times=b.get("times"), opts=noise_opts_c(b, **over), trace=trace)


def select_rigs(b, rigs):
    """the batch with only the rigs listed, in that order, renumbered"""
    rigs = list(rigs)
    c = dict(b, n_rigs=len(rigs))
    for k in ("pose_status", "rvec", "tvec", "cov_status", "cov_param", "cov", "true_R", "true_t", "rec_frame"):
        c[k] = b[k][:, rigs]
    c["rec_rig"] = np.tile(np.arange(len(rigs), dtype=np.int32), (b["n_frames"], 1))
    return c


def per_term(got, want, n_terms):
    return abs(float(got) - float(want)) / max(1, n_terms)
