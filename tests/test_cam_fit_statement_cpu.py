"""CPU tests of the independent statement of the camera set fit (tests/cam_fit_statement.py) on the cases of tests/cam_fit_shapes.py:
every case covers what it claims, the statement recovers planted camera poses and reaches scipy's joint minimum, planted errors in
its text are refused, and the bars the device is held to are measured again."""
import numpy as np
import pytest

import cam_fit_shapes as sh
import cam_fit_statement as cf

SMALL = [n for n in sh.NAMES if not n.startswith("e")]   # (e) is (a)'s geometry 572 times over: its claims and its system only
NOISE_FREE = [n for n in SMALL if n.endswith("noise-free")]
NOISY = [n for n in SMALL if n.endswith("0.1 px")]


@pytest.mark.parametrize("name", sh.NAMES)
def test_every_case_covers_what_it_claims(name):
    assert sh.check_claims(sh.case(name))


@pytest.mark.parametrize("name", NOISE_FREE)
def test_noise_free_cases_recover_the_planted_poses(name):
    """Rule 2 alone, the loop and the joint minimum all land on the planted set carried into the anchor's frame."""
    b, A = sh.case(name), sh.assembled(name)
    want = sh.planted_set(b, A["init"]["placed"], A["init"]["anchor"])
    ref, own = sh.joint_reference(name), sh.fit_reference(name)
    for what, R, t in (("rule 2", A["R0"], A["t0"]), ("joint minimum", ref["R"], ref["t"]), ("loop", own["R"], own["t"])):
        d = sh.set_distance(R, t, *want)
        print("%s %s: %.2e rad, %.2e of the distance from the planted set" % (name, what, d[0], d[1]))
        assert sh.within_bar(d), (what, d)
    anchor = A["slot"]
    assert (own["R"][anchor] == np.eye(3)).all() and not own["t"][anchor].any(), "the anchor moved"


@pytest.mark.parametrize("name", SMALL)
def test_the_loop_reaches_the_joint_minimum(name):
    ref, own = sh.joint_reference(name), sh.fit_reference(name)
    d = sh.set_distance(own["R"], own["t"], ref["R"], ref["t"])
    print("%s: %d rounds, cost %.6g -> %.6g (joint %.6g), %.2e rad %.2e from the joint minimum" % (name, own["rounds"], own["cost_init"], own["cost"], ref["cost"], d[0], d[1]))
    assert sh.within_bar(d) and own["cost"] <= own["cost_init"] and abs(own["cost"] - ref["cost"]) <= 1e-6 * max(ref["cost"], 1e-3)


def test_noise_leaves_the_initial_assembly_away_from_the_minimum():
    """Why the refinement is the product: at 0.1 px the averaged relative poses alone are more than ten bars off, at a higher cost."""
    for name in NOISY:
        A, ref, own = sh.assembled(name), sh.joint_reference(name), sh.fit_reference(name)
        d = sh.set_distance(A["R0"], A["t0"], ref["R"], ref["t"])
        print("%s: rule 2 alone %.2e rad %.2e from the minimum, cost %.4g against %.4g" % (name, d[0], d[1], own["cost_init"], ref["cost"]))
        assert d[0] > 10 * cf.POSE_BAR[0] and own["cost_init"] > ref["cost"]


@pytest.mark.parametrize("wrong", ["cross sign", "update without Exp(w) tc", "camera dropped"])
def test_planted_errors_in_the_loop_are_refused(wrong):
    name = "b 0.1 px"
    b, A, ref = sh.case(name), sh.assembled(name), sh.joint_reference(name)
    out = cf.fit(A["obs"], A["R0"], A["t0"], A["slot"], sh.planted_rig_poses(b, A["obs"], A["init"]["anchor"]), max_rounds=15, wrong=wrong)
    d = sh.set_distance(out["R"], out["t"], ref["R"], ref["t"])
    print("%s: %.3g rad %.3g from the joint minimum, cost %.6g against %.6g" % (wrong, d[0], d[1], out["cost"], ref["cost"]))
    assert not sh.within_bar(d)


def test_the_anchors_rows_taken_at_index_0_are_refused():
    """The cameras of case (c) in reverse order, so that the anchor is the last slot: dropping slot 0 instead lets the anchor move."""
    name = "c 0.1 px"
    b, A = sh.case(name), sh.assembled(name)
    placed = A["init"]["placed"][::-1]
    slot = placed.index(A["init"]["anchor"])
    assert slot != 0
    O = cf.Observations(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], placed)
    R0, t0 = A["R0"][::-1], A["t0"][::-1]
    poses0 = sh.planted_rig_poses(b, O, A["init"]["anchor"])
    ref = sh.joint_reference(name)
    good = cf.fit(O, R0, t0, slot, poses0, max_rounds=15)
    assert sh.within_bar(sh.set_distance(good["R"], good["t"], ref["R"][::-1], ref["t"][::-1]))
    bad = cf.fit(O, R0, t0, slot, poses0, max_rounds=15, wrong="anchor at 0")
    assert not sh.within_bar(sh.set_distance(bad["R"], bad["t"], ref["R"][::-1], ref["t"][::-1]))


@pytest.mark.parametrize("wrong", ["edge direction", "tie order"])
def test_planted_errors_in_the_initial_assembly_are_refused(wrong):
    name = "c noise-free"
    b, A = sh.case(name), sh.assembled(name)
    init = cf.initial_assembly(A["rr"], len(b["cameras"]), b["recs"].shape[1] * b["n_rigs"], b["min_items"], wrong=wrong)
    if wrong == "tie order":
        assert init["parent"] != b["claims"]["parents"]
        return
    want = sh.planted_set(b, init["placed"], init["anchor"])
    d = sh.set_distance(np.array([init["T"][c][0] for c in init["placed"]]), np.array([init["T"][c][1] for c in init["placed"]]), *want)
    assert d[0] > 0.1 or d[1] > 0.1, d


def test_the_per_item_rotation_in_the_translation_mean_is_refused():
    """The edge translation is the mean of t_b - Rbar t_a: with the per-item rotation R_b R_a^T it comes out elsewhere once there is noise."""
    name = "a 0.1 px"
    b, A = sh.case(name), sh.assembled(name)
    init = cf.initial_assembly(A["rr"], 2, b["recs"].shape[1], b["min_items"], wrong="per-item rotation")
    assert np.abs(init["T"][1][1] - A["init"]["T"][1][1]).max() > 1e-6 and (init["T"][1][0] == A["init"]["T"][1][0]).all()


def test_undistorting_with_camera_0s_coefficients_is_refused():
    name = "a noise-free"
    b, A = sh.case(name), sh.assembled(name)
    init = A["init"]
    O = cf.Observations(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], init["placed"], wrong="camera 0's coefficients")
    R, t = sh.planted_set(b, init["placed"], init["anchor"])
    out = cf.joint_minimum(O, R, t, A["slot"], sh.planted_rig_poses(b, O, init["anchor"]))
    assert not sh.within_bar(sh.set_distance(out["R"], out["t"], R, t))


def measure():
    """Every figure of cam_fit_statement's constants, measured: the float64 statement against numpy.longdouble (S, g, delta at the
    rule-2 start with every record's rig pose at its minimum under that set -- the state the device is probed at, where the noise-free
    cases' residuals are float32 roundings of the pixels, 1e-8 of a pixel coordinate; worst over the cases), the distance between two joint minima from different starts
    (0.1 px cases) and the move float32 rounding of the pixel coordinates alone causes (noise-free cases: the joint minimum against
    the planted set)."""
    worst = np.zeros(3)
    for name in sh.NAMES:
        b, A = sh.case(name), sh.assembled(name)
        init = A["init"]
        out = []
        rvecs = np.array([cf.mv.rotvec(R) if np.abs(R - np.eye(3)).max() else np.zeros(3) for R in A["R0"]])
        solved = A["obs"].solve_poses(cf.rot_many(rvecs), A["t0"], sh.planted_rig_poses(b, A["obs"], init["anchor"]))
        for T in (np.float64, np.longdouble):
            O = cf.Observations(b["recs"], b["model"], b["rig_of_model"], b["n_rigs"], b["cameras"], init["placed"], dtype=T)
            poses = solved.astype(T)
            Rc = cf.rot_many(rvecs, T)   # a camera set is given as (rvec, tvec): the rotation matrices are part of the evaluation
            S, g = cf.reduced_system(O, Rc, A["t0"].astype(T), poses)
            d, pd = cf.step(S, g, A["slot"], 1e-3)
            assert pd
            out.append((S, g, d, float(O.costs(Rc, A["t0"], poses).sum())))
        worst = np.maximum(worst, cf.system_deviation(*out[0][:3], *out[1][:3], out[1][3]))
    minima, f32 = np.zeros(2), np.zeros(2)
    for name in NOISY:
        b, A, ref = sh.case(name), sh.assembled(name), sh.joint_reference(name)
        other = cf.joint_minimum(A["obs"], A["R0"], A["t0"], A["slot"], ref["poses"])
        minima = np.maximum(minima, sh.set_distance(other["R"], other["t"], ref["R"], ref["t"]))
    for name in NOISE_FREE:
        b, A, ref = sh.case(name), sh.assembled(name), sh.joint_reference(name)
        f32 = np.maximum(f32, sh.set_distance(ref["R"], ref["t"], *sh.planted_set(b, A["init"]["placed"], A["init"]["anchor"])))
    return {"S": worst[0], "g": worst[1], "delta": worst[2], "minima": tuple(minima), "f32": tuple(f32)}


def test_measured_bars():
    """The constants of cam_fit_statement are what a measurement gives today, to 2 %."""
    m = measure()
    print(m)
    for k in ("S", "g", "delta"):
        assert abs(m[k] - cf.SYSTEM_ERR[k]) <= 0.02 * cf.SYSTEM_ERR[k], (k, m[k])
    for got, want in zip(m["minima"] + m["f32"], cf.MINIMA_DISTANCE + cf.F32_PIXEL_MOVE):
        assert abs(got - want) <= 0.02 * want, (got, want)
    assert cf.POSE_BAR == tuple(16 * max(a, c) for a, c in zip(cf.MINIMA_DISTANCE, cf.F32_PIXEL_MOVE))
