"""GPU tests of the model reconstruction through the public calls (Detector.fit_model / fit_model_device, Model.save): every batch of
tests/model_fit_shapes.py is fitted once and the result is held to rules 1-8 of include/ctag_pose.h and to the independent
statement's joint minimum (tests/model_fit_statement.py)."""
import ctypes as C

import numpy as np
import pytest

import cylindertag_amd as ca
import model_fit_shapes as sh
import model_fit_statement as ms
from cylindertag_amd import capi
from model_fit_testlib import Detectors, device_poses, model_of, observation_cost

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    e = {"dets": Detectors(), "fit": {}}
    yield e
    e["dets"].close()


def _opts(b, **kw):
    return ca.model_fit_opts(min_obs=b["min_obs"], **kw)


def _fit(env, name):
    """The batch fitted once (host entry, no metric scale) and shared: (batch, detector, camera, seed Model, fitted Model, its view, stats)."""
    if name not in env["fit"]:
        b = sh.batch(name)
        det, cam, seed = env["dets"].of(b), ca.make_camera(b["K"], b["dist"]), model_of(b["seed"])
        M, stats = det.fit_model(b["recs"], seed, cam, _opts(b))
        env["fit"][name] = (b, det, cam, seed, M, M.view(), stats)
    return env["fit"][name]


@pytest.mark.parametrize("name", sh.NAMES)
def test_result_obeys_the_rules(env, name):
    """Cost monotonicity; stats.cost = the sum of the public pose call's record costs on the returned model, byte for byte (rule 3);
    held corners, base, axis and ids bit-equal to the seed; counts as the statement has them; a model no frame shows comes back as
    the seed with CTAG_POSE_NOT_SEEN."""
    b, det, cam, seed, M, view, stats = _fit(env, name)
    obs, held, _ = sh.observed(name)
    s = b["seed"]
    assert view["ids"].tobytes() == s["ids"].tobytes() and view["base"].tobytes() == s["base"].tobytes() and view["axis"].tobytes() == s["axis"].tobytes()
    assert view["size"] == s["size"] and view["corners"].dtype == np.float32
    seed_poses = device_poses(det, b["recs"], seed, cam)
    assert [o is not None for o in obs] == [bool(p["status"] == 0) for p in seed_poses]
    poses = device_poses(det, b["recs"], M, cam)
    for m, st in enumerate(stats):
        n_rec = sum(o is not None and o["model"] == m for o in obs)
        assert st["n_records"] == n_rec and st["n_points_held"] == held[m].sum() and st["n_points_fitted"] == (~held[m]).sum() and st["reserved"] == 0
        assert view["corners"][m][held[m]].tobytes() == s["corners"][m][held[m]].tobytes()
        if n_rec == 0 or held[m].all():
            assert st["status"] == capi.POSE_NOT_SEEN and view["corners"][m].tobytes() == s["corners"][m].tobytes() and st["rounds"] == 0
            continue
        assert st["status"] == 0 and 1 <= st["rounds"] <= 30
        assert st["cost"] <= st["cost0"]
        assert st["cost0"] == observation_cost(seed_poses, obs, m)
        assert st["cost"] == observation_cost(poses, obs, m), "stats.cost is not the cost of the returned model"
        n_pts = sum(len(o["ids"]) for o in obs if o is not None and o["model"] == m)
        assert st["rms_px"] == np.sqrt(2.0 * st["cost"] / n_pts)
        print("%s model %d: %d records, %d rounds, cost %.4g -> %.4g, rms %.3g px, lambda %.3g" % (name, m, n_rec, st["rounds"], st["cost0"], st["cost"], st["rms_px"], st["lambda"]))
    if "unseen_model" in b["claims"]:
        assert stats[b["claims"]["unseen_model"]]["status"] == capi.POSE_NOT_SEEN


@pytest.mark.parametrize("name", sh.NAMES)
def test_corners_against_the_joint_minimum(env, name):
    """Every model of every batch: in the seed's gauge, held corners untouched, within 16 x the float32 spacing of the statement's joint
    minimum over corners and poses (ms.CORNER_BAR_MM; two statement minima from different starts lie closer than the spacing)."""
    b, det, cam, seed, M, view, stats = _fit(env, name)
    _, held, _ = sh.observed(name)
    for m, ref in sh.joint_reference(name).items():
        if ref is None:
            continue
        d = ms.check_result(view["corners"][m], b["seed"]["corners"][m], held[m], ref["X"], "%s model %d" % (name, m))
        print("%s model %d: %.2e mm from the joint minimum (bar %.2e); cost %.6g, the statement's %.6g" % (name, m, d, ms.CORNER_BAR_MM, stats[m]["cost"], ref["cost"]))


@pytest.mark.parametrize("name", [n for n in sh.NAMES if sh.batch(n)["claims"].get("recover")])
def test_noise_free_batches_recover_the_planted_model(env, name):
    b, det, cam, seed, M, view, stats = _fit(env, name)
    _, held, _ = sh.observed(name)
    for m in range(len(b["seed"]["ids"])):
        fit_ = ~held[m]
        if stats[m]["status"] != 0:
            continue
        X, truth = view["corners"][m].astype(np.float64), b["truth"]["corners"][m].astype(np.float64)
        err = np.abs(ms.apply_similarity(ms.similarity(X[fit_], truth[fit_]), X[fit_]) - truth[fit_]).max()
        print("%s model %d: planted model recovered to %.2e mm (bar %.2e)" % (name, m, err, 16 * ms.F32_SPACING_MM))
        assert err <= 16 * ms.F32_SPACING_MM


@pytest.mark.parametrize("name", [sh.NAMES[1], sh.NAMES[4]])
def test_two_calls_and_both_entries_return_the_same_bytes(env, name):
    import torch
    b, det, cam, seed, M, view, stats = _fit(env, name)
    M2, stats2 = det.fit_model(b["recs"], seed, cam, _opts(b))
    d_recs = torch.from_numpy(np.ascontiguousarray(b["recs"]).view(np.uint8).reshape(-1)).cuda()
    M3, stats3 = det.fit_model_device(d_recs.data_ptr(), len(b["recs"]), seed, cam, _opts(b))
    for other, st in ((M2, stats2), (M3, stats3)):
        v = other.view()
        assert all(v[k].tobytes() == view[k].tobytes() for k in ("ids", "base", "axis", "corners")) and st.tobytes() == stats.tobytes()


def test_metric_scale_restores_the_planted_scale(env):
    name = sh.NAMES[5]
    b, det, cam, seed, M, view, stats = _fit(env, name)
    _, held, _ = sh.observed(name)
    Ms, st = det.fit_model(b["recs"], seed, cam, _opts(b, strip_height=b["strip_height"]))
    vs = Ms.view()
    poses = device_poses(det, b["recs"], Ms, cam)
    obs = sh.observed(name)[0]
    for m in range(len(b["seed"]["ids"])):
        fit_ = ~held[m]
        X, truth = vs["corners"][m].astype(np.float64), b["truth"]["corners"][m].astype(np.float64)
        scale_before = ms.similarity(view["corners"][m].astype(np.float64)[fit_], truth[fit_])[0]
        scale = ms.similarity(X[fit_], truth[fit_])[0]
        want, factor, centre = ms.metric_scale(view["corners"][m], held[m], b["strip_height"])
        print("model %d: scale to the truth %.7f before, %.7f after; factor %.7f" % (m, scale_before, scale, factor))
        assert abs(scale_before - 1 / b["claims"]["scaled_seed"]) < 1e-4 and abs(scale - 1.0) <= 16 * ms.F32_SPACING_MM / 25.0   # 25 mm: half the strip
        assert np.abs(X - want).max() <= 2 * ms.F32_SPACING_MM
        assert vs["corners"][m][held[m]].tobytes() == b["seed"]["corners"][m][held[m]].tobytes()
        base = centre + factor * (b["seed"]["base"][m].astype(np.float64) - centre)
        assert np.abs(vs["base"][m] - base).max() <= 2 * ms.F32_SPACING_MM and vs["axis"][m].tobytes() == b["seed"]["axis"][m].tobytes()
        assert st[m]["cost"] == observation_cost(poses, obs, m)


def test_model_file_round_trip(env, tmp_path):
    b, det, cam, seed, M, view, stats = _fit(env, sh.NAMES[0])
    path = str(tmp_path / "fitted.model")
    M.save(path)
    back = ca.Model(path).view()
    assert all(back[k].tobytes() == view[k].tobytes() for k in ("ids", "base", "axis", "corners")) and back["size"] == view["size"]


def test_rejections(env):
    """Rule 8, each on its own."""
    b = sh.batch(sh.NAMES[0])
    det, cam, seed = env["dets"].of(b), ca.make_camera(b["K"], b["dist"]), model_of(b["seed"])
    L = det.L
    recs = np.ascontiguousarray(b["recs"])
    stats = np.zeros(3, ca.MODEL_FIT_STAT_DT)
    out = C.c_void_p()

    def call(h=det.h, res=recs.ctypes.data, n=len(recs), s=seed.m, camera=cam, opts=None, o=C.byref(out), st=stats.ctypes.data, fn=L.ctag_model_fit):
        return fn(h, res, n, s, C.byref(camera) if camera is not None else None, C.byref(opts) if opts is not None else None, o, st)

    assert call(h=None) == capi.ERR_ARG and call(res=None) == capi.ERR_ARG and call(s=None) == capi.ERR_ARG and call(camera=None) == capi.ERR_ARG
    assert call(o=None) == capi.ERR_ARG and call(st=None) == capi.ERR_ARG
    assert call(n=0) == capi.ERR_ARG and call(n=-1) == capi.ERR_ARG
    for bad in (dict(max_rounds=-1), dict(min_obs=0), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda_max=0.0), dict(rel_tol=0.0), dict(lambda0=float("nan")),
                dict(strip_height=float("inf"))):
        assert call(opts=ca.model_fit_opts(**bad)) == capi.ERR_ARG, bad
    other = sh.batch(sh.NAMES[2])   # 20 columns against a handle of 12
    assert call(s=model_of(other["seed"]).m) == capi.ERR_ARG
    tilted = ca.make_camera(b["K"], np.float32([0] * 12 + [0.1, 0]))
    assert call(camera=tilted) == capi.ERR_UNSUPPORTED
    odd = ca.make_camera(b["K"], np.zeros(3, np.float32))
    assert call(camera=odd) == capi.ERR_UNSUPPORTED
    for fn in (L.ctag_model_fit_device,):
        assert call(fn=fn, res=None) == capi.ERR_ARG and call(fn=fn, n=0, res=1) == capi.ERR_ARG
    assert not out.value
    assert L.ctag_model_save(None, b"x") == capi.ERR_ARG and L.ctag_model_save(seed.m, None) == capi.ERR_ARG
    # max_rounds = 0: the seed comes back, cost = cost0
    M0, st0 = det.fit_model(recs, seed, cam, ca.model_fit_opts(max_rounds=0))
    assert M0.view()["corners"].tobytes() == b["seed"]["corners"].tobytes() and (st0["cost"] == st0["cost0"]).all() and (st0["rounds"] == 0).all()
