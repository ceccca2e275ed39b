"""The host build of cylindertag_amd/csrc/ctag_math.h (through the oracle's math probe) against mpmath at 240 bits, on the argument sets of
tests/math_shapes.py: errors in ulp of the TRUE value, at the edges of every function's stated domain, and the special values pinned exactly.

The functions use only IEEE operations in a fixed order and the sets are fixed, so the worst error over a set is one exact, reproducible number.
BOUNDS holds each of them as measured against mpmath, rounded up to the next tenth of an ulp ("Accuracy of the shared math", has the
table); a change to a polynomial or a reduction is held to them.  tests/test_math_device_gpu.py requires the device's bits to be the host's on the
same sets."""
import math

import mpmath
import numpy as np
import pytest

import math_shapes as ms

mp = mpmath.mp

# (function, set) -> worst error in ulp of the true value, rounded up to the next tenth
BOUNDS = {
    ("sin64", "uniform over |x| <= 1e5"): 1.4,  # 1.3032 at 9890.255985664422
    ("sin64", "the doubles next to k pi/2, k <= 63000"): 0.5,  # 0.4998 at 14966.547401701773
    ("sin64", "|x| <= pi/4, the kernel switch and kcos64's thresholds"): 0.7,  # 0.6112 at 0.7780894950681554
    ("cos64", "uniform over |x| <= 1e5"): 1.3,  # 1.2918 at -81005.200967677
    ("cos64", "the doubles next to k pi/2, k <= 63000"): 0.5,  # 0.4998 at 1870.8184252127216
    ("cos64", "|x| <= pi/4, the kernel switch and kcos64's thresholds"): 1.2,  # 1.1590 at 0.7517462009764289
    ("atan2_64", "|x|, |y| <= 1e3"): 1.2,  # 1.1835 at y, x = 537.6459186959119, -151.65509765281104
    ("atan2_64", "log-uniform over 2^+-430"): 1.0,  # 0.9458 at y, x = 3.9736221690307674e+51, -3.0949873376335483e+40
    ("atan2_64", "either side of the 2^+-60 shortcut"): 0.8,  # 0.7237 at y, x = -1.4867913688443933e-33, -1.6493008980481233e-52
    ("atan2_64", "atan64's range breaks"): 1.1,  # 1.0928 at y, x = -2.437500000000001, -1.0
    ("exp64", "uniform over [-708, 709]"): 1.8,  # 1.7693 at -431.15088458155657
    ("exp64", "r at +-ln2/64 and at 0"): 1.6,  # 1.5370 at -398.0614292859411
    ("exp64", "the clamps and inside them"): 0.6,  # 0.5319 at 708.9999999999999
    ("log64", "log-uniform over the positive doubles"): 0.7,  # 0.6600 at 0.3850648890924553
    ("log64", "subnormals"): 0.5,  # 0.4987 at 1.551072272241772e-308
    ("log64", "next to 1"): 0.5,  # 0.5000 at 0.9999999999999998
    ("log64", "the reduction break sqrt(2)/2, sqrt(2) and the range's ends"): 0.6,  # 0.5078 at 0.7071067811865479
    ("acos64", "float-valued over [-1, 1]"): 2.1,  # 2.0487 at 0.9165493249893188
    ("acos64", "the floats next to +-1"): 1.5,  # 1.4129 at 0.9999988675117493
    ("sin32", "float-valued arguments"): 0.5,  # 0.5000 at -46363.625
    ("cos32", "float-valued arguments"): 0.5,  # 0.5000 at -1.5682541131973267
    ("atan2_32", "float-valued arguments"): 0.5,  # 0.4999 at y, x = 1.2082796096801758, 378.84613037109375
    ("exp32", "float-valued over [-87, 88] and the clamps"): 1.0,  # 0.9481 at -16.932331085205078
}


def _sets():
    """name -> (op, [(set name, x, y)], true value of (x, y) as an mpf, ulp)"""
    trig = [(n, x, np.zeros_like(x)) for n, x in ms.trig_sets()]
    one = lambda sets: [(n, x, np.zeros_like(x)) for n, x in sets]
    fs = ms.float_sets()
    return {
        "sin64": (ms.OP_SIN64, trig, lambda x, y: mpmath.sin(x), ms.ulp_of),
        "cos64": (ms.OP_COS64, trig, lambda x, y: mpmath.cos(x), ms.ulp_of),
        "atan2_64": (ms.OP_ATAN2_64, ms.atan2_sets(), lambda y, x: mpmath.atan2(y, x), ms.ulp_of),
        "exp64": (ms.OP_EXP64, one(ms.exp64_sets()), lambda x, y: mpmath.exp(x), ms.ulp_of),
        "log64": (ms.OP_LOG64, one(ms.log64_sets()), lambda x, y: mpmath.log(x), ms.ulp_of),
        "acos64": (ms.OP_ACOS64, one(ms.acos64_sets()), lambda x, y: mpmath.acos(x), ms.ulp_of),
        "sin32": (ms.OP_SIN32, [("float-valued arguments", fs["trig"], np.zeros_like(fs["trig"]))], lambda x, y: mpmath.sin(x), ms.ulp32_of),
        "cos32": (ms.OP_COS32, [("float-valued arguments", fs["trig"], np.zeros_like(fs["trig"]))], lambda x, y: mpmath.cos(x), ms.ulp32_of),
        "atan2_32": (ms.OP_ATAN2_32, [("float-valued arguments", fs["atan2"][0], fs["atan2"][1])], lambda y, x: mpmath.atan2(y, x), ms.ulp32_of),
        "exp32": (ms.OP_EXP32, [("float-valued over [-87, 88] and the clamps", fs["exp"], np.zeros_like(fs["exp"]))], lambda x, y: mpmath.exp(x), ms.ulp32_of),
    }


_true = {}


def true_values(name, set_name):
    """mpmath's values for one set, computed once"""
    key = (name, set_name)
    if key not in _true:
        op, sets, f, ulp = _sets()[name]
        (x, y), = [(x, y) for n, x, y in sets if n == set_name]
        _true[key] = [f(mpmath.mpf(float(a)), mpmath.mpf(float(b))) for a, b in zip(x, y)]
    return _true[key]


def measure(oracle, name, set_name):
    op, sets, f, ulp = _sets()[name]
    (x, y), = [(x, y) for n, x, y in sets if n == set_name]
    got = oracle.math(op, x, y)
    assert np.isfinite(got).all(), (name, set_name)
    worst, at = ms.worst_ulp(got, true_values(name, set_name), ulp)
    return worst, (float(x[at]), float(y[at])), got


CASES = [(name, s[0]) for name, v in _sets().items() for s in v[1]]


@pytest.mark.parametrize("name,set_name", CASES, ids=["%s-%d" % (n, k) for k, (n, s) in enumerate(CASES)])
def test_worst_error_against_mpmath(oracle, name, set_name):
    worst, at, _ = measure(oracle, name, set_name)
    print("%s over %s: worst %.4f ulp at %r" % (name, set_name, worst, at))
    assert worst <= BOUNDS[(name, set_name)], (worst, at)
    assert worst > BOUNDS[(name, set_name)] - 0.1000001  # the table is the measurement: a better function gets a tighter bound


@pytest.mark.parametrize("name", ["sin32", "cos32", "atan2_32"])
def test_float_entry_points_round_once(oracle, name):
    """Evaluated in double and rounded once: never more than 1 float ulp off, and the correctly rounded float in at least 999 of 1000 cases"""
    op, sets, f, ulp = _sets()[name]
    set_name, x, y = sets[0]
    got = oracle.math(op, x, y)
    true = true_values(name, set_name)
    worst, at = ms.worst_ulp(got, true, ms.ulp32_of)
    exact = np.mean([float(g) == ms.nearest_float32(t) for g, t in zip(got, true) if abs(t) > 2.0 ** -126])
    print("%s: worst %.4f float ulp, %.5f correctly rounded" % (name, worst, exact))
    assert worst <= 1.0 and exact >= 0.999


def test_atan2_special_values_are_c_atan2(oracle):
    """Every pairing of +-0, +-inf, NaN, a finite value and the smallest subnormal: C's atan2, the sign of zero included"""
    y, x = ms.atan2_special()
    got = oracle.math(ms.OP_ATAN2_64, y, x)
    want = np.array([math.atan2(a, b) for a, b in zip(y, x)])
    assert len(y) == 81 and ms.same_bits_or_both_nan(got, want), [(a, b, g, w) for a, b, g, w in zip(y, x, got, want) if not ms.same_bits_or_both_nan([g], [w])]
    assert ms.same_bits_or_both_nan(want, np.arctan2(y, x))


def test_exp_clamps_and_special_values(oracle):
    x, want = ms.exp64_special()
    assert ms.same_bits_or_both_nan(oracle.math(ms.OP_EXP64, x), want)  # inf above 709, 0 below -708: the documented clamps
    assert oracle.math(ms.OP_EXP64, np.array([709.0]))[0] < np.inf and oracle.math(ms.OP_EXP64, np.array([-708.0]))[0] > 2.2250738585072014e-308
    x, want = ms.exp32_special()
    assert ms.same_bits_or_both_nan(oracle.math(ms.OP_EXP32, x), want)  # 0 below -87 (no denormals), inf above 88
    edge = oracle.math(ms.OP_EXP32, np.array([-87.0, 88.0, 0.0, -0.0]))
    assert edge[0] >= 2.0 ** -126 and edge[1] < np.inf and edge[2] == 1.0 and edge[3] == 1.0


def test_log_and_acos_special_values(oracle):
    x, want = ms.log64_special()
    assert ms.same_bits_or_both_nan(oracle.math(ms.OP_LOG64, x), want)
    x, want = ms.acos64_special()
    assert ms.same_bits_or_both_nan(oracle.math(ms.OP_ACOS64, x), want)
    # sin64 does not keep the sign of a zero argument (x + x^3 (S1 + ...) is -0 + +0): +0 for both, where C's sin(-0) is -0; ctag_math.h says so
    z = oracle.math(ms.OP_SIN64, np.array([0.0, -0.0]))
    assert ms.same_bits_or_both_nan(z, np.array([0.0, 0.0])) and (oracle.math(ms.OP_COS64, np.array([0.0, -0.0])) == 1.0).all()


def test_round32_is_roundf(oracle):
    x, want = ms.round32_cases()
    got = oracle.math(ms.OP_ROUND32, x)
    assert ms.same_bits_or_both_nan(got, want), list(zip(x, got, want))  # ties away from zero; -0.3 gives -0
    rng = np.random.RandomState(209)
    r = np.concatenate([rng.uniform(-1e4, 1e4, 4000), rng.randint(-5000, 5000, 2000) + 0.5]).astype(np.float32)
    want = np.where(np.abs(r - np.trunc(r)) >= 0.5, np.trunc(r) + np.sign(r), np.trunc(r))  # exact in float for |r| < 2^23
    assert (oracle.math(ms.OP_ROUND32, r.astype(np.float64)) == want).all()


def test_div64_corners_on_the_host(oracle):
    """The host form of ctm::div64 is `/`: Python's own a / d (correctly rounded) at the corners of the documented domain"""
    a, d = ms.div64_corners()
    want = np.array([float(p) / float(q) for p, q in zip(a, d)])
    assert ms.same_bits_or_both_nan(oracle.math(ms.OP_DIV64, a, d), want) and np.isfinite(want).all()
    assert (np.abs(d).min(), np.abs(d).max()) == (2.0 ** -500, 2.0 ** 500) and (np.abs(want[a != 0]).min() == 2.0 ** -500) and (a == 0).any()
