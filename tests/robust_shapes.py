"""Source pose records, their detection records and the option sets for the robust refit (k_pose_robust.hip), shared by
tests/test_robust_statement_cpu.py (which qualifies them and measures the statement's own float64 error on them:
robust_statement.EVAL, LOOP, STOP) and tests/test_robust_pose_gpu.py (the device): both build the same cases here.

A case has the form of tests/cov_shapes.py's, whose builders make most of them, plus "runs": the names of the option sets (OPTION_SETS,
or the case's own "own_opts") it is run under.  The smallest records at which the kernel can go wrong:

  marker 20 golden    per-marker point counts 4 8 28 32 36 60 64 68 124 128 132 160: fewer points than lanes, both sides of a mask
                      word's edge (32), of the lane wrap (64) and of its second turn (128), the largest marker.  Every feature gives 4 or
                      8 points (pose_estimation.cpp:77-94), so a record's count is a multiple of 4: counts such as 5, 31, 33, 63, 65 and
                      129 cannot be built through the correspondence rule, and the median's rank (n - 1) / 2 always falls between the two
                      middle values.  A second marker of 16 points in every frame; cov_shapes.OUTLIER_PX on one corner of the 64-point
                      marker.  Every loss and scale, max_iterations 0, 1, 2 and 50 (1 and 2 run into the cap), scale_px = 1e9
  marker 12 / 16      the 8- and 12-coefficient cameras
  rig, rig n_dist12   164 256 796 800 points
  mv                  2, 3 (own intrinsics, n_dist 0 5 12) and 8 cameras
  noise free          pixels of the planted pose, rounded to float only: 2.5 sigma_hat lies far below min_scale_px, which decides
  tied median         a feature given twice: every norm occurs twice, the median's rank lies inside a pair
  feature shifted     all 8 corners of one of five features moved by 5 px: 8 of 40 points
  threshold edge      scale_px chosen so that one point's s_i lies 2e-5 a^2 inside, and for another option set outside, the inlier
                      threshold (max_iterations = 0: the statement says where the point is)
  rules               every source status, every cause of CTAG_ROBUST_BAD_RECORD (cov_shapes.rules_case without its two singular
                      records -- a robust refit of a problem without a minimum has no pose to be held to -- rig_rules, mv_rules), a NaN
                      pixel (CTAG_ROBUST_DEGENERATE)"""
import numpy as np

import cov_shapes as sh
import robust_statement as rb
from ctag_testlib import RESULT_DT
from pose_testlib import POSE_DT, golden_camera_and_model, make_cylinder_model
import rig_statement as rs
from rig_shapes import FULL, _pixels, _place, _place_rig, _pose, layout
from rig_testlib import cylinder_model

MARKER_COUNTS = (4, 8, 28, 32, 36, 60, 64, 68, 124, 128, 132, 160)
GRID = 4096  # wavefronts of one k_pose_robust launch at most


def _o(**kw):
    return rb.default_opts(**kw)


OPTION_SETS = {
    "cauchy auto": _o(), "cauchy auto eval": _o(max_iterations=0), "cauchy auto 1": _o(max_iterations=1), "cauchy auto 2": _o(max_iterations=2),
    "huber auto": _o(loss=rb.HUBER), "huber auto eval": _o(loss=rb.HUBER, max_iterations=0),
    "cauchy 1.0": _o(scale_px=1.0), "cauchy 1.0 eval": _o(scale_px=1.0, max_iterations=0),
    "huber 0.5": _o(loss=rb.HUBER, scale_px=0.5), "huber 0.5 eval": _o(loss=rb.HUBER, scale_px=0.5, max_iterations=0),
    "huber k 4": _o(loss=rb.HUBER, auto_k=4.0, min_scale_px=0.01),
    "weight one": _o(loss=rb.HUBER, scale_px=1e9), "weight one eval": _o(loss=rb.HUBER, scale_px=1e9, max_iterations=0),
}
ALL_RUNS = tuple(OPTION_SETS)
BOTH = ("cauchy auto", "cauchy auto eval", "huber auto", "huber auto eval")


def _marker_records(name, model, K, dist, items, noise, seed):
    """One frame, one marker per item = (model index, patterns, edit); edit(rec, marker index) bends the marker's pixels afterwards."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(1, RESULT_DT)
    src = []
    for mi, pat, edit in items:
        pose = _pose(rng, model["corners"][mi])
        p0 = int(rng.integers(0, model["size"] - len(pat) + 1))
        k = _place(rec[0], int(model["ids"][mi]), _pixels(rng, model, mi, K, dist, pose, noise), p0, pat)
        P = np.zeros((), POSE_DT)
        P["model_index"], P["marker"], P["rvec"], P["tvec"] = mi, k, pose[0], pose[1]
        if edit is not None:
            edit(rec[0], k)
        P["n_points"] = len(sh.ps.correspondences(rec[0], k, model, mi)[1])
        src.append(P)
    return sh._fill_costs({"kind": "marker", "name": name, "recs": rec, "model": model, "cameras": [(K, dist)], "camera_poses": [sh.ZERO_POSE],
                           "sources": np.array(src), "n_rigs": None})


def rig_case(dist_name, counts, seed):
    """cov_shapes.rig_case with a seed of its own: one rig, one frame per count, members by rig_shapes.layout over markers of 20
    columns.  (cov_shapes' own draw has a record whose covariance pivot lies below the 1e-6 every refitted record here must keep.)"""
    K, golden_dist, _ = golden_camera_and_model()
    dist = golden_dist if dist_name == "golden" else sh.test_cameras()[dist_name]
    model = cylinder_model(6, 20)
    rig_of_model = np.zeros(6, np.int32)
    rng = np.random.default_rng(seed)
    recs = np.zeros(len(counts), RESULT_DT)
    src = np.zeros(len(counts), rs.RIG_POSE_DT)
    for f, n in enumerate(counts):
        members = layout(n, 20)
        pose = _pose(rng, model["corners"][:len(members)])
        _place_rig(recs[f], rng, model, range(len(members)), members, K, dist, pose, 0.2)
        src[f] = rs.expected_header(recs[f], model, rig_of_model, 0, f)[0]
        assert src[f]["status"] == 0 and src[f]["n_points"] == n
        src[f]["rvec"], src[f]["tvec"] = pose
    return sh._fill_costs({"kind": "rig", "name": "rig %s" % dist_name, "recs": recs, "model": model, "cameras": [(K, dist)], "camera_poses": [sh.ZERO_POSE],
                           "sources": src, "n_rigs": 1, "rig_of_model": rig_of_model})


def noise_free_case():
    K, dist, _ = golden_camera_and_model()
    model = make_cylinder_model(3, 20)
    return dict(_marker_records("noise free", model, K, dist, [(0, [FULL] * 2, None), (1, sh.marker_patterns(36), None), (2, [FULL] * 9, None)], 0.0, 1901), runs=BOTH)


def tied_median_case():
    def twice(rec, k):
        f0 = int(rec["markers"][k]["first_feature"])
        rec["features"][f0 + 1] = rec["features"][f0]
    K, dist, _ = golden_camera_and_model()
    model = make_cylinder_model(1, 12)
    case = _marker_records("tied median", model, K, dist, [(0, [FULL] * 3, twice)], 0.2, 1903)
    assert int(case["sources"][0]["n_points"]) == 24
    return dict(case, runs=BOTH)


def feature_shifted_case():
    def shift(rec, k):
        f0 = int(rec["markers"][k]["first_feature"])
        rec["features"][f0 + 2]["corners"][0::2] += np.float32(sh.OUTLIER_PX)  # u of all 8 corners
    K, dist, _ = golden_camera_and_model()
    model = make_cylinder_model(2, 20)
    case = _marker_records("feature shifted", model, K, dist, [(0, [FULL] * 5, shift), (1, [FULL] * 10, shift)], 0.2, 1903)
    return dict(case, runs=BOTH + ("cauchy 1.0", "huber 0.5"), shifted=[range(16, 24), range(16, 24)])


def nan_pixel_case():
    def nan(rec, k):
        rec["features"][int(rec["markers"][k]["first_feature"]) + 1]["corners"][3] = np.float32(np.nan)
    K, dist, _ = golden_camera_and_model()
    model = make_cylinder_model(2, 12)
    case = _marker_records("nan pixel", model, K, dist, [(0, [FULL] * 3, nan), (1, [FULL] * 3, None)], 0.2, 1904)
    return dict(case, runs=("cauchy auto", "huber 0.5 eval"), expect=[rb.ROBUST_DEGENERATE, rb.ROBUST_OK])


def threshold_edge_case(marker):
    """Record 10 of the marker case (60 points) alone, under two given scales: point 7's s_i at the source pose is a^2 (1 - 2e-5) under
    the first and a^2 (1 + 2e-5) under the second (the longdouble statement's s_i)."""
    sub = dict(marker, name="threshold edge", sources=marker["sources"][10:11].copy(), outlier=None)
    e = rb.expected_of(sub, _o(max_iterations=0), np.longdouble)[0]
    s = e["s"][7]
    own = {"edge inside": _o(max_iterations=0, scale_px=float(np.sqrt(s / np.longdouble(1 - 2e-5)))),
           "edge outside": _o(loss=rb.HUBER, max_iterations=0, scale_px=float(np.sqrt(s / np.longdouble(1 + 2e-5))))}
    return dict(sub, runs=tuple(own), own_opts=own, edge_point=7)


def _robust_expect(case, keep=None):
    """A rules case of cov_shapes with its expectations as robust statuses (the three codes mean the same)."""
    n = len(case["sources"]) if keep is None else keep
    assert all(e in (0, 1, 2) for e in case["expect"][:n])
    return dict(case, sources=case["sources"][:n], expect=list(case["expect"][:n]), runs=("cauchy auto", "huber 0.5 eval"))


_CACHE = {}


def all_cases():
    """Every case, in one list; built once per process."""
    if "cases" not in _CACHE:
        marker = dict(sh.marker_case(20, "golden", counts=MARKER_COUNTS, outlier_at=64, seed=19), runs=ALL_RUNS)
        rig = rig_case("golden", sh.RIG_COUNTS, 2050)
        mv = sh.mv_cases()
        cases = [marker,
                 dict(sh.marker_case(12, "n_dist8", counts=(4, 8, 60, 64, 68, 96), seed=21), runs=BOTH),
                 dict(sh.marker_case(16, "n_dist12", counts=(4, 68, 96), outlier_at=0, seed=20), runs=BOTH),
                 dict(rig, runs=("cauchy auto", "cauchy auto eval", "huber 0.5", "huber 0.5 eval")),
                 dict(rig_case("n_dist12", (164, 800), 1967), runs=("cauchy auto", "huber auto eval"))]
        cases += [dict(c, runs=("cauchy auto", "cauchy auto eval", "huber auto")) for c in mv]
        cases += [noise_free_case(), tied_median_case(), feature_shifted_case(), threshold_edge_case(marker), nan_pixel_case(),
                  _robust_expect(sh.rules_case(), keep=len(sh.rules_case()["sources"]) - 2), _robust_expect(sh.rig_rules(rig)),
                  _robust_expect(sh.mv_rules(mv[0]))]
        _CACHE["cases"] = cases
    return _CACHE["cases"]


def runs_of(case):
    """[(name, option dict)] of a case."""
    own = case.get("own_opts", {})
    return [(name, own[name] if name in own else OPTION_SETS[name]) for name in case["runs"]]


def expected_of(case, opts, ft=np.float64):
    """The statement's dicts for every source record of a case, cached per (case, options, float type)."""
    key = (case["name"], tuple(sorted(opts.items())), ft.__name__)
    if key not in _CACHE:
        _CACHE[key] = rb.expected_of(case, opts, ft)
    return _CACHE[key]


def pparts_of(case, ft=np.float64):
    """w -> the problem parts of source record w (for check_robust_records)."""
    return lambda w: rb.cs.problem_parts(rb.parts_of(case, case["sources"][w]), case["cameras"], case["camera_poses"], ft)


def log64_points():
    """Arguments of ctm::log64 the host and the device are probed with: the Cauchy loss's 1 + s / a^2 from 1 upwards, both sides of the
    reduction's sqrt(2) breaks, powers of two, subnormals, the ends of the range."""
    rng = np.random.default_rng(64)
    x = np.concatenate([1.0 + 10.0 ** rng.uniform(-16, 6, 4000), 2.0 ** rng.uniform(-1074, 1023, 2000), 2.0 ** np.arange(-1074, 1024, 7.0),
                        np.sqrt(2.0) * (1 + np.arange(-50, 51) * 2.0 ** -52), np.sqrt(0.5) * (1 + np.arange(-50, 51) * 2.0 ** -53),
                        [1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0), 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308]])
    return np.ascontiguousarray(x, np.float64)


def log64_ulps(x, got):
    """|got - log(x)| in units of the last place of the true value, against longdouble's log."""
    want = np.log(x.astype(np.longdouble))
    ulp = np.spacing(np.abs(want.astype(np.float64))).astype(np.longdouble)
    return float((np.abs(got.astype(np.longdouble) - want) / ulp).max())
