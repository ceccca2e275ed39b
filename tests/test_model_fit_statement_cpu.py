"""CPU tests of the model reconstruction's independent statement (tests/model_fit_statement.py) on the batches of
tests/model_fit_shapes.py: it recovers planted models, its reduced Gauss-Newton and its joint minimum agree, it rejects planted
errors, and the bars the device is held to are measured here.  Plus the host-only parts of the library: the ideal-cylinder seed
and the .model text written by ctag_model_save."""
import os

import numpy as np
import pytest

import cylindertag_amd as ca
import model_fit_shapes as sh
import model_fit_statement as ms
import testkit as tk
from ctag_testlib import GOLDEN
from cylindertag_amd import models
from pose_testlib import read_model_file


def test_batches_cover_what_they_claim():
    assert [b["name"] for b in sh.all_batches()] == sh.NAMES
    for b in sh.all_batches():
        assert sh.check_claims(b)
    sizes = {b["seed"]["size"] for b in sh.all_batches()}
    assert sizes == {4, 12, 20}
    assert {len(b["dist"]) for b in sh.all_batches()} >= {0, 5, 8, 12}
    assert {b["noise"] for b in sh.all_batches()} == {0.0, 0.1}


@pytest.mark.parametrize("name", [n for n in sh.NAMES if sh.batch(n)["claims"].get("recover")])
def test_statement_recovers_planted_models_from_noise_free_records(name):
    """The loop of rule 4 from a seed 20 % (or 1 mm, or a factor 1.1) off ends on the planted model, up to a similarity, to within
    16 float32 spacings of a coordinate (the records' pixels and the models are float32)."""
    b = sh.batch(name)
    _, held, _ = sh.observed(name)
    for m, fit in sh.fit_reference(name).items():
        if fit is None:
            continue
        ref = {"fit": fit}
        fit_ = ~held[m]
        truth = b["truth"]["corners"][m].astype(np.float64)
        X = ref["fit"]["X"]
        err = np.abs(ms.apply_similarity(ms.similarity(X[fit_], truth[fit_]), X[fit_]) - truth[fit_]).max()
        print("%s model %d: %d rounds, cost %.3g -> %.3g, recovered to %.2e mm" % (name, m, ref["fit"]["rounds"], ref["fit"]["cost0"], ref["fit"]["cost"], err))
        assert ref["fit"]["cost"] < 1e-5   # what float32 pixels leave: ~1200 points x (2^-13 px)^2
        assert err <= 16 * ms.F32_SPACING_MM


@pytest.mark.parametrize("name", sh.NAMES)
def test_reduced_gauss_newton_and_joint_minimum_agree(name):
    _, held, _ = sh.observed(name)
    b = sh.batch(name)
    for m, joint in sh.joint_reference(name).items():
        if joint is None:
            continue
        ref = {"fit": sh.fit_reference(name)[m], "joint": joint}
        d = ms.check_result(ref["fit"]["X"].astype(np.float32), b["seed"]["corners"][m], held[m], ref["joint"]["X"], "%s model %d" % (name, m))
        print("%s model %d: reduced GN vs joint minimum %.2e mm (bar %.2e), costs %.9g %.9g" % (name, m, d, ms.CORNER_BAR_MM, ref["fit"]["cost"], ref["joint"]["cost"]))
        assert ref["joint"]["cost"] <= ref["fit"]["cost"] * (1 + 1e-6) + 1e-7   # 1e-7: a third of what float32 pixels leave of a noise-free cost


def test_two_joint_minima_from_different_starts_coincide():
    """The distance between two statement minima started from different points: one of the two candidates for the corner bar."""
    worst = 0.0
    for name, m in ((sh.NAMES[1], 1), (sh.NAMES[4], 2)):
        b, ref = sh.batch(name), {"fit": sh.fit_reference(name)[m], "joint": sh.joint_reference(name)[m], "batch": sh.joint_reference(name)[m]["batch"]}
        _, held, _ = sh.observed(name)
        rng = np.random.default_rng(5)
        X0 = ref["fit"]["X"] + rng.normal(0, 0.05, ref["fit"]["X"].shape)
        J = ms.joint_minimum(ref["batch"], X0, b["seed"]["corners"][m].astype(np.float64), held[m], ref["fit"]["poses"])
        worst = max(worst, float(np.abs(J["X"] - ref["joint"]["X"])[~held[m]].max()))
    print("two joint minima differ by at most %.2e mm; float32 spacing %.2e mm" % (worst, ms.F32_SPACING_MM))
    assert worst <= ms.CORNER_ERR_MM


def test_statement_rejects_planted_errors():
    name = sh.NAMES[0]
    b = sh.batch(name)
    obs, held, _ = sh.observed(name)
    ref = {"fit": sh.fit_reference(name)[0], "joint": sh.joint_reference(name)[0], "batch": sh.joint_reference(name)[0]["batch"]}
    seed = b["seed"]["corners"][0]
    good = ref["fit"]["X"].astype(np.float32)
    ms.check_result(good, seed, held[0], ref["joint"]["X"])
    # the gauge left free: the same shape, moved by a similarity
    free = ms.apply_similarity((1.01, np.eye(3), np.array([0.3, 0, 0])), good).astype(np.float32)
    free[held[0]] = seed[held[0]]
    with pytest.raises(AssertionError, match="gauge"):
        ms.check_result(free, seed, held[0], ref["joint"]["X"])
    B = ref["batch"]
    F = ms.fit(B, seed.astype(np.float64), held[0], ref["fit"]["poses"], max_rounds=3, wrong="free gauge")
    with pytest.raises(AssertionError):
        ms.check_result(F["X"].astype(np.float32), seed, held[0], ref["joint"]["X"])
    # held corners moved
    moved = good.copy()
    moved[np.nonzero(held[0])[0][0]] += np.float32(1e-3)
    with pytest.raises(AssertionError, match="held"):
        ms.check_result(moved, seed, held[0], ref["joint"]["X"])
    # a wrong corner order in the correspondences: the planted model is no longer a minimum
    swap = np.arange(8)
    swap[[4, 5]] = 5, 4
    wrong_obs = [None if o is None else dict(o, ids=o["ids"] // 8 * 8 + swap[o["ids"] % 8]) for o in obs]
    Bw = ms.Batch(wrong_obs, 0, sh.camera_of(b))
    truth = b["truth"]["corners"][0].astype(np.float64)
    pl = sh.planted_poses(b, B)
    assert B.costs(truth, pl).sum() < 1e-3 < 1.0 < Bw.costs(truth, ms.solve_poses(Bw, truth, pl)).sum()
    # a record of another model counted in
    mixed = [dict(o, model=0) if o is not None and o["model"] == 1 and i % 7 == 0 else o for i, o in enumerate(obs)]
    Bm = ms.Batch(mixed, 0, sh.camera_of(b))
    assert len(Bm.recs) > len(B.recs)
    Sm, _ = ms.reduced_system(Bm, seed.astype(np.float64), ms.solve_poses(Bm, seed.astype(np.float64), sh.planted_poses(b, Bm)), len(seed))
    S, _ = ms.reduced_system(B, seed.astype(np.float64), ref["fit"]["poses"] * 0 + ms.solve_poses(B, seed.astype(np.float64), pl), len(seed))
    assert ms.system_deviation(Sm, np.zeros(len(S)), np.zeros(len(S)), S, np.ones(len(S)), np.ones(len(S)), held[0], 1.0)[0] > 1e3 * ms.SYSTEM_BAR["S"]


def test_measured_bars():
    """The figures of DESIGN.md section 15: the float64 statement of (S, g, delta) against numpy.longdouble on every model of every
    batch, the same with the summation order reversed, and the relative cost change float32 rounding of the model causes."""
    worst, worst_rev, rel = np.zeros(3), np.zeros(3), 0.0
    for name in sh.NAMES:
        b = sh.batch(name)
        obs, held, _ = sh.observed(name)
        P = b["seed"]["size"] * 8
        for m, fit in sh.fit_reference(name).items():
            if fit is None or (name == sh.NAMES[4] and m > 1):
                continue
            ref = {"fit": fit}
            B, seed = ms.Batch(obs, m, sh.camera_of(b)), b["seed"]["corners"][m].astype(np.float64)
            poses = ms.solve_poses(B, seed, sh.planted_poses(b, B))
            cost = float(B.costs(seed, poses).sum())
            S, g = ms.reduced_system(B, seed, poses, P)
            d, pd = ms.step(S, g, held[m], 1e-3)
            BL = ms.Batch(obs, m, sh.camera_of(b), np.longdouble)
            SL, gL = ms.reduced_system(BL, seed.astype(np.longdouble), poses.astype(np.longdouble), P)
            dL, pdL = ms.step(SL, gL, held[m], 1e-3)
            Sr, gr = ms.reduced_system(B, seed, poses, P, reverse=True)
            dr, _ = ms.step(Sr, gr, held[m], 1e-3)
            assert pd and pdL
            worst = np.maximum(worst, ms.system_deviation(S, g, d, SL, gL, dL, held[m], cost))
            worst_rev = np.maximum(worst_rev, ms.system_deviation(Sr, gr, dr, S, g, d, held[m], cost))
            if b["noise"]:
                X = ref["fit"]["X"]
                c64 = float(B.costs(X, ms.solve_poses(B, X, ref["fit"]["poses"])).sum())
                X32 = X.astype(np.float32).astype(np.float64)
                c32 = float(B.costs(X32, ms.solve_poses(B, X32, ref["fit"]["poses"])).sum())
                rel = max(rel, abs(c32 - c64) / c64)
    print("float64 statement vs long double: S %.2e g %.2e delta %.2e" % tuple(worst))
    print("summation order reversed:         S %.2e g %.2e delta %.2e" % tuple(worst_rev))
    print("float32 rounding of the model changes the cost by %.2e relative (0.1 px batches)" % rel)
    for k, v in zip(("S", "g", "delta"), worst):
        assert abs(v / ms.SYSTEM_ERR[k] - 1) <= 0.02, (k, v)   # the recorded figure IS the measurement
    assert (worst_rev <= worst).all()
    assert abs(rel / ms.REL_TOL_F32 - 1) <= 0.02, rel
    o = ca.model_fit_opts()
    assert o.rel_tol == 4 * ms.REL_TOL_F32


def test_cylinder_model_equals_the_synthetic_scenes_model(dictionary):
    state, _ = dictionary
    _, want = tk.synth3d_model(state)
    radii = [models.default_radius(r, state.shape[1]) for r in range(state.shape[0])]
    got = models.cylinder_model(state, 60.0, radii)
    assert got.dtype == np.float32 and got.shape == want.shape
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(got - want) <= ulp).all()   # sin / cos of two math libraries: at most the last float32 bit
    print("cylinder_model vs ctag_synth3d_model: %d of %d coordinates differ in the last bit" % (int((got != want).sum()), want.size))


def test_model_text_round_trip(tmp_path):
    """ctag_model_save's text parses back to the same float bits with a plain Python parser, and the fixture survives
    parse -> write -> parse."""
    fixture = os.path.join(GOLDEN, "CTag_2f12c.model")
    a = read_model_file(fixture)
    M = ca.Model(fixture)
    out = str(tmp_path / "copy.model")
    M.save(out)
    b = read_model_file(out)
    for k in ("ids", "base", "axis", "corners"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ca.Model(out).view()["corners"].tobytes() == M.view()["corners"].tobytes()
    rng = np.random.default_rng(0)
    corners = (rng.normal(0, 300, (3, 32, 3)) * 10.0 ** rng.integers(-6, 3, (3, 32, 3))).astype(np.float32)
    base = rng.normal(0, 1, (3, 3)).astype(np.float32)
    M2 = ca.Model(ids=[5, 7, 9], corners=corners, model_size=4, base=base, axis=base[::-1].copy())
    out2 = str(tmp_path / "random.model")
    M2.save(out2)
    c = read_model_file(out2)
    assert c["corners"].tobytes() == corners.tobytes() and c["base"].tobytes() == base.tobytes() and list(c["ids"]) == [5, 7, 9] and c["size"] == 4
    with pytest.raises(ca.CtagError):
        M2.save(str(tmp_path / "no" / "such" / "dir.model"))


def test_a_wrong_seed_at_a_held_but_seen_corner_biases_the_fit():
    """What the first batch avoids by giving its once-seen corners (held at min_obs 2) the consistent seed value: with the ideal
    cylinder's +20 % value left there, the record that sees them is posed against wrong points and pulls the corners fitted from
    it.  The size of that bias is recorded here; it is above the bar the consistent batch is held to."""
    name = sh.NAMES[0]
    b = sh.batch(name)
    obs, held, seen = sh.observed(name)
    odd = held[0] & (seen[0] > 0)
    assert odd.sum() == 8
    B = ms.Batch(obs, 0, sh.camera_of(b))
    truth = b["truth"]["corners"][0].astype(np.float64)
    seed = b["seed"]["corners"][0].astype(np.float64)
    fit_ = ~held[0]
    wrong = seed.copy()
    wrong[odd] = _ideal_seed(b)[odd]
    errs = {}
    for label, s in (("consistent", seed), ("wrong", wrong)):
        F = ms.fit(B, s, held[0], sh.planted_poses(b, B), max_rounds=15, round_float=False)
        X = F["X"]
        errs[label] = float(np.abs(ms.apply_similarity(ms.similarity(X[fit_], truth[fit_]), X[fit_]) - truth[fit_]).max())
    print("fitted corners against the planted model: %.2e mm with the consistent seed value, %.2e mm with the ideal cylinder's" % (errs["consistent"], errs["wrong"]))
    assert errs["consistent"] <= 16 * ms.F32_SPACING_MM < errs["wrong"]


def _ideal_seed(b):
    """The +20 % ideal cylinder the first batch's seed was before its once-seen corners were made consistent (model 0)."""
    from cylindertag_amd.models import cylinder_model
    ideal = cylinder_model(b["state"], sh.STRIP, sh.RADIUS * 1.2).astype(np.float64)
    ideal[..., 2] += 500.0
    return ideal[0].astype(np.float32).astype(np.float64)
