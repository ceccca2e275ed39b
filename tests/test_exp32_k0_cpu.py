"""`ctm::exp32_nonpos_k0` and `ctm::exp32_k_is_zero` (cylindertag_amd/csrc/ctag_math.h) on the host: where the predicate holds the bare polynomial has the
bits of `exp32_nonpos`, and the predicate says `rintf(x * log2e) == 0` with the very product `exp32_nonpos` rounds.  The loop over the floats runs in the
test kit library (`ctag_testkit_exp32_k0_sweep`), not in Python:
  - EVERY float of the three binades [-0.5, -0.0625) -- the predicate's boundary (x * log2e = -0.5, x ~ -0.3466) and its whole neighbourhood lie there;
  - every 64th float below, down to the smallest denormal, and -0.0 and +0.0.
The counts the sweep returns are checked against the same boundary found here with numpy's float32 product, so a sweep that visited nothing, or a predicate
that is never (or always) true, fails."""
import numpy as np

import testkit as tk

LOG2E = np.float32(1.44269502162933349609375)
NEG_HALF, NEG_SIXTEENTH, NEG_ZERO, NEG_MIN_DENORMAL = 0xBF000000, 0xBD800000, 0x80000000, 0x80000001


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _last_bits_with_k_zero():
    """The float furthest from zero whose product with log2e (rounded to float) is still >= -0.5: bisection over the bit patterns (the product is monotonic)."""
    lo, hi = NEG_SIXTEENTH, NEG_HALF  # predicate true at lo, false at hi
    assert _f32(lo) * LOG2E >= np.float32(-0.5) and not _f32(hi) * LOG2E >= np.float32(-0.5)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _f32(mid) * LOG2E >= np.float32(-0.5):
            lo = mid
        else:
            hi = mid
    return lo


def test_constants_are_the_floats_they_name():
    assert (_f32(NEG_HALF), _f32(NEG_SIXTEENTH), _f32(NEG_MIN_DENORMAL)) == (-0.5, -0.0625, -np.float32(1.401298464324817e-45))
    assert _f32(NEG_ZERO) == 0 and np.signbit(_f32(NEG_ZERO))


def test_every_float_of_the_three_binades_around_the_boundary():
    first = NEG_SIXTEENTH + 1  # the floats of [-0.5, -0.0625): patterns above -0.0625's up to -0.5's
    got = tk.exp32_k0_sweep(first, NEG_HALF)
    boundary = _last_bits_with_k_zero()
    x = _f32(boundary)
    assert -0.347 < x < -0.346 and np.rint(x * LOG2E) == 0 and np.rint(_f32(boundary + 1) * LOG2E) == -1
    assert got["visited"] == 3 * 2 ** 23 and got["k_is_zero"] == boundary - first + 1 and 0 < got["k_is_zero"] < got["visited"]
    assert got["predicate_mismatches"] == 0 and got["bit_mismatches"] == 0, "first at bit pattern 0x%08x" % (got["first_bad"] or 0)


def test_the_boundary_itself_and_its_neighbours():
    """The tie: a product of exactly -0.5 rounds to -0 (half to even), so the predicate's `>=` is right to include it -- if a float gives that product."""
    boundary = _last_bits_with_k_zero()
    for bits in range(boundary - 4, boundary + 5):
        got = tk.exp32_k0_sweep(bits, bits)
        assert got["visited"] == 1 and got["k_is_zero"] == (1 if bits <= boundary else 0)
        assert got["predicate_mismatches"] == 0 and got["bit_mismatches"] == 0, "0x%08x" % bits


def test_every_64th_float_below_down_to_the_smallest_denormal():
    for start in (NEG_MIN_DENORMAL, NEG_MIN_DENORMAL + 63):  # two phases of the stride: the smallest denormal itself, and -0.0625 itself
        got = tk.exp32_k0_sweep(start, NEG_SIXTEENTH, 64)
        assert got["visited"] == (NEG_SIXTEENTH - start) // 64 + 1 >= 2 ** 23 and got["k_is_zero"] == got["visited"]
        assert got["predicate_mismatches"] == 0 and got["bit_mismatches"] == 0, "first at bit pattern 0x%08x" % (got["first_bad"] or 0)
    assert (NEG_SIXTEENTH - (NEG_MIN_DENORMAL + 63)) % 64 == 0


def test_both_zeros():
    for bits in (NEG_ZERO, 0x00000000):
        got = tk.exp32_k0_sweep(bits, bits)
        assert got == dict(visited=1, k_is_zero=1, predicate_mismatches=0, bit_mismatches=0, first_bad=None)


def test_the_sweep_refuses_what_is_outside_the_domain():
    import pytest
    for first, last, step in ((0x00000001, 0x00000001, 1), (0x7FC00000, 0x7FC00000, 1), (0xFFC00000, 0xFFC00000, 1), (NEG_HALF, NEG_SIXTEENTH, 1), (NEG_ZERO, NEG_ZERO, 0)):
        with pytest.raises(tk.CtagError):
            tk.exp32_k0_sweep(first, last, step)
