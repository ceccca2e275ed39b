"""The batches the track filter is held to (tests/track_filter_statement.py says what a batch is), drawn from the model itself as
track_shapes.py draws the smoother's.  All are small: frame counts on each side of the kernel's 64-frame pre-pass, gaps at the dropping
limit, gated runs, a half turn, a spin fast enough for the left Jacobian to matter, many rigs, one long call."""
import functools

import numpy as np

import track_filter_statement as fs
import track_shapes as sh
import track_statement as ts

MG = 4  # sh.BASE_OPTS' max_gap
EDGE_FRAMES = (1, 2, 63, 64, 65, 129)


def _edge(n):
    m0 = np.ones(n, bool)
    m1 = np.ones(n, bool)
    m1[:min(2, n - 1)] = False   # unmeasured first frames
    return sh.make_batch("n%d" % n, 100 + n, n, [m0, m1], ["good", "mixed"])


def _gaps():
    n = 90
    m0 = np.zeros(n, bool)       # index distances max_gap - 1, max_gap (one track) and max_gap + 1 (dropped and restarted)
    f = 3
    for d in (1, 1, MG - 1, 1, 1, MG, 1, 1, MG + 1, 1, 1, 1, 2, MG, MG, 1, MG + 1, MG + 3, 1, 1):
        m0[f] = True
        f += d
    m0[f] = True
    m1 = sh.runs_mask(n, 0, (30, 40), MG)   # two runs max_gap unmeasured frames apart: distance max_gap + 1, two tracks
    m2 = sh.runs_mask(n, 5, (80,), 0)
    times = np.cumsum(np.random.default_rng(7).uniform(0.02, 0.05, n))  # non-uniform
    return sh.make_batch("gaps", 31, n, [m0, m1, m2], ["good", "weak", "mixed"], times=times)


def _robust(name, seed, **opts):
    n = 40
    b = sh.make_batch(name, seed, n, [sh.runs_mask(n, 1, (39,), 0), sh.runs_mask(n, 0, (40,), 0)], ["good", "good"], opts=opts)
    sh.plant_gross_error(b, 21, 0)
    return b


def _gated_run():
    n = 40
    b = sh.make_batch("gated_run", 35, n, [sh.runs_mask(n, 0, (40,), 0)], ["good"], opts=dict(gate=5.0))
    for f in range(20, 20 + MG):   # max_gap gated frames in a row: the last one drops the track, frame 20 + max_gap restarts it
        sh.plant_gross_error(b, f, 0, n_sigma=1000.0)   # far enough to stay outside the gate while the prediction widens
    return b


def _half_turn():
    n = 24
    b = sh.make_batch("half_turn", 36, n, [np.ones(n, bool)], ["good"], opts=dict(vel0_sigma_rot=0.2, q_rot=0.05))
    # the whole track turned by a constant on the right so that frame 12 is 5e-4 short of a half turn: R' = R C keeps the left noise model
    axis = np.array([0.6, -0.64, 0.48])
    Cm = b["true_R"][12, 0].T @ ts.so3_exp((np.pi - 5e-4) * axis)
    for f in range(n):
        b["rvec"][f, 0] = ts.so3_log(ts.so3_exp(b["rvec"][f, 0]) @ Cm)
        b["true_R"][f, 0] = b["true_R"][f, 0] @ Cm
    return b


def _spin():
    n = 50   # |w| about 17 sqrt(3) rad/s at 30 frames/s: D |w| about 1 rad
    return sh.make_batch("spin", 37, n, [np.ones(n, bool), sh.runs_mask(n, 0, (20, 25), 3)], ["good", "mixed"], opts=dict(vel0_sigma_rot=17.0, q_rot=2.0))


def _mv():
    n = 40
    return sh.make_batch("mv", 38, n, [sh.runs_mask(n, 1, (20, 12), 6), np.ones(n, bool)], ["good", "mixed"], kind="mv")


def _bad_rig():
    n = 30
    b = sh.make_batch("bad_rig", 39, n, [np.ones(n, bool)] * 3, ["good", "good", "weak"])
    b["rec_rig"] = np.array(b["rec_rig"], copy=True)
    b["rec_rig"][17, 1] = 0
    return b


def _wide():
    n, nr = 20, 200
    rng = np.random.default_rng(8)
    masks = [rng.random(n) < 0.8 for _ in range(nr)]
    return sh.make_batch("wide", 40, n, masks, ["good", "weak", "mixed", "mixed"] * (nr // 4))


def _long():
    n = 4100
    m0 = np.ones(n, bool)
    m0[np.random.default_rng(9).random(n) < 0.15] = False
    m1 = sh.runs_mask(n, 7, (2000, 1500, 500), 20)
    return sh.make_batch("long", 41, n, [m0, m1], ["mixed", "good"])


BUILDERS = {("n%d" % n): functools.partial(_edge, n) for n in EDGE_FRAMES}
BUILDERS.update(gaps=_gaps, gate=lambda: _robust("gate", 32, gate=5.0), gated_run=_gated_run,
                huber=lambda: _robust("huber", 32, loss=ts.LOSS_HUBER, loss_scale=4.0), cauchy=lambda: _robust("cauchy", 32, loss=ts.LOSS_CAUCHY, loss_scale=4.0),
                half_turn=_half_turn, spin=_spin, mv=_mv, bad_rig=_bad_rig, wide=_wide, long=_long)
BATCHES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def batch(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def statement(name, longdouble=False):
    """the statement's records for the batch in one call (computed once, shared by the tests; do not write into them)"""
    return fs.run_batch(batch(name), np.longdouble if longdouble else np.float64)


def filter_opts(b, **over):
    from cylindertag_amd import capi
    o = {k: v for k, v in fs.filter_opts(b).items()}
    o.update(over)
    return capi.track_filter_opts(**o)


class DeviceFilter:
    """a library filter for batch b's rig count and options on detector det"""

    def __init__(self, det, b, n_rigs=None, **over):
        self.rigset = sh.RigSet(b["n_rigs"] if n_rigs is None else n_rigs)
        self.kind = b["kind"]
        self.f = det.track_filter(self.rigset, filter_opts(b, **over))

    def run(self, b, times="batch"):
        """one host-form step call on the frames of b"""
        P, Q = sh.to_records(b)
        t = b.get("times") if isinstance(times, str) else times
        fn = self.f.step_mv if self.kind == "mv" else self.f.step
        return fn(P, Q, b["n_frames"], times=t)

    def close(self):
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def device_run(det, b, **over):
    with DeviceFilter(det, b, **over) as F:
        return F.run(b)


def body(rec):
    """the bytes of records without their rig and frame fields"""
    r = np.array(rec, copy=True)
    r["rig"] = 0
    r["frame"] = 0
    return r.tobytes()


def check_against(rec, want, label, bar=None):
    """the library's records against the statement's: status and flags exact, rig and frame their place, cov symmetric bit for bit,
    everything 0 where the status is not OK, the rest within bar"""
    bar = fs.BAR if bar is None else bar
    assert (rec["status"] == want["status"]).all(), label
    assert (rec["flags"] == want["flags"]).all(), label
    nf, nr = rec["status"].shape
    assert (rec["rig"] == np.arange(nr)[None, :]).all() and (rec["frame"] == np.arange(nf)[:, None]).all()
    assert (rec["cov"] == rec["cov"].transpose(0, 1, 3, 2)).all(), "cov is symmetric bit for bit"
    off = rec["status"] != fs.OK
    for k in sh.FIELDS[2:]:
        assert not rec[k][off].any(), (label, k)
    dev = fs.deviation(sh.as_dict(rec), want)
    print(label, {k: "%.3g" % v for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= bar[k], (label, k, v, bar[k])
