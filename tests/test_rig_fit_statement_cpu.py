"""CPU tests of the independent statement of the rig assembly (tests/rig_fit_statement.py) on the batches of tests/rig_fit_shapes.py:
every batch covers what it claims, the statement recovers planted layouts and rejects planted errors (judged by scipy's joint minimum),
and the bars the device is held to are measured again."""
import numpy as np
import pytest

import model_fit_statement as ms
import rig_fit_shapes as sh
import rig_fit_statement as rf

NOISY = [sh.NAMES[1], sh.NAMES[3]]


@pytest.mark.parametrize("name", sh.NAMES)
def test_every_batch_covers_what_it_claims(name):
    assert sh.check_claims(sh.batch(name))


@pytest.mark.parametrize("name", [n for n in sh.NAMES if sh.batch(n)["claims"].get("recover")])
def test_noise_free_batches_recover_the_planted_layout(name):
    """Rule 2 alone, the loop and the joint minimum all land on the planted layout carried into the anchor's frame."""
    b, A = sh.batch(name), sh.assembled(name)
    for g, ref in sh.joint_reference(name).items():
        rig = A["rigs"][g]
        want = rf.layout(b["model"]["corners"], sh.planted_layout(b, g, rig["anchor"], rig["placed"]), round_float=False)
        own = sh.fit_reference(name).get(g)   # (the loop is not run on batch (f))
        for what, X in [("rule 2", A["X0"]), ("joint minimum", ref["X"])] + ([("loop", own["X"])] if own else []):
            d = sh.corner_distance(X, want, rig["placed"])
            print("%s rig %d %s: %.2e mm from the planted layout" % (name, g, what, d))
            assert d <= rf.CORNER_BAR_MM, (what, d)


def test_noise_leaves_the_initial_assembly_away_from_the_minimum():
    """Why the refinement is the product: at 0.1 px the averaged relative poses alone are more than ten bars off, at a higher cost."""
    for name in NOISY:
        A = sh.assembled(name)
        ref, own = sh.joint_reference(name)[0], sh.fit_reference(name)[0]
        d = sh.corner_distance(A["X0"], ref["X"], A["rigs"][0]["placed"])
        print("%s: rule 2 alone %.3f mm from the minimum, cost %.4g against %.4g" % (name, d, own["cost_init"], ref["cost"]))
        assert d > 10 * rf.CORNER_BAR_MM and own["cost_init"] > ref["cost"] and abs(own["cost"] - ref["cost"]) <= 1e-6 * ref["cost"]


@pytest.mark.parametrize("wrong", ["cross sign", "keep anchor", "member dropped"])
def test_planted_errors_in_the_loop_are_rejected(wrong):
    name = sh.NAMES[1]
    b, A = sh.batch(name), sh.assembled(name)
    rig, ref = A["rigs"][0], sh.joint_reference(name)[0]
    B = ref["batch"]
    out = rf.fit(B, b["model"]["corners"], rig["T"], rig["placed"], rig["anchor"], sh.planted_rig_poses(b, B, rig["anchor"]), max_rounds=15, round_float=False,
                 wrong=wrong)
    d = sh.corner_distance(out["X"], ref["X"], rig["placed"])
    print("%s: %.3g mm from the joint minimum, cost %.6g against %.6g" % (wrong, d, out["cost"], ref["cost"]))
    assert d > rf.CORNER_BAR_MM


def test_edge_averaging_the_wrong_way_round_is_rejected():
    name = sh.NAMES[0]
    b, A = sh.batch(name), sh.assembled(name)
    rig = rf.initial_assembly(A["poses"], len(b["recs"]), sh.members_of(b, 0), b["min_frames"], wrong="edge direction")
    want = rf.layout(b["model"]["corners"], sh.planted_layout(b, 0, rig["anchor"], rig["placed"]), round_float=False)
    assert sh.corner_distance(rf.layout(b["model"]["corners"], rig["T"]), want, rig["placed"]) > 1.0


def measure():
    """Every figure of rig_fit_statement's constants, measured: the float64 statement against numpy.longdouble (S, g, delta at the
    rule-2 start, worst over the batches), the distance between two joint minima from different starts and the relative cost change
    float32 rounding of the model alone causes (0.1 px batches)."""
    worst = np.zeros(3)
    for name in sh.NAMES:
        b, A = sh.batch(name), sh.assembled(name)
        P = b["model"]["size"] * 8
        for g, ref in sh.joint_reference(name).items():
            rig = A["rigs"][g]
            dropped = np.array([m == rig["anchor"] for m in rig["placed"]])
            out = []
            for T in (np.float64, np.longdouble):
                B = ms.Batch(A["obs"], g, sh.camera_of(b), dtype=T)
                poses = sh.planted_rig_poses(b, B, rig["anchor"]).astype(T)
                S, gv = rf.reduced_system(B, A["X0"].reshape(-1, 3).astype(T), poses, rig["placed"], P)
                d, pd = rf.step(S, gv, dropped, 1e-3)
                assert pd
                out.append((S, gv, d, float(B.costs(A["X0"].reshape(-1, 3), poses).sum())))
            worst = np.maximum(worst, rf.system_deviation(*out[0][:3], *out[1][:3], out[1][3]))
    minima, rel = 0.0, 0.0
    for name in NOISY:
        b, A = sh.batch(name), sh.assembled(name)
        rig, ref = A["rigs"][0], sh.joint_reference(name)[0]
        B = ref["batch"]
        other = rf.joint_minimum(B, b["model"]["corners"], rig["T"], rig["placed"], rig["anchor"], ref["poses"])
        minima = max(minima, sh.corner_distance(other["X"], ref["X"], rig["placed"]))
        c32 = rf.rig_cost(B, ref["X"].astype(np.float32), ref["poses"])[0]
        rel = max(rel, abs(c32 - ref["cost"]) / ref["cost"])
    return {"S": worst[0], "g": worst[1], "delta": worst[2], "minima_mm": minima, "rel_f32": rel}


def test_measured_bars():
    """The constants of rig_fit_statement are what a measurement gives today, to 2 %."""
    m = measure()
    print(m)
    for k in ("S", "g", "delta"):
        assert abs(m[k] - rf.SYSTEM_ERR[k]) <= 0.02 * rf.SYSTEM_ERR[k], (k, m[k])
    assert abs(m["minima_mm"] - rf.MINIMA_DISTANCE_MM) <= 0.02 * rf.MINIMA_DISTANCE_MM, m["minima_mm"]
    assert abs(m["rel_f32"] - rf.REL_TOL_F32) <= 0.02 * rf.REL_TOL_F32, m["rel_f32"]
    assert rf.CORNER_BAR_MM == 16 * max(rf.F32_SPACING_MM, rf.MINIMA_DISTANCE_MM)
