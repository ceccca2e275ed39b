"""`ctm::welsch_k_is_zero` and `ctm::kWelschK0MaxDist` (cylindertag_amd/csrc/ctag_math.h): k_welsch votes on the point's distance |r| instead of on the
weight's argument a = -r * r * c * c (c = 1 / 2.9846f, three float products left to right), and the two predicates must agree on EVERY float:
    exp32_k_is_zero(a)  ==  |r| <= kWelschK0MaxDist.
  - R0 is found again here by bisection over the bit patterns in numpy.float32 (the chain is monotone in |r|) and compared with the constant read from the header;
  - the header's own two predicates, compiled for the host without contraction, are swept over every float of the two binades around R0 ([1, 2) and [2, 4)),
    every 64th float elsewhere in [0, 2^12] (both phases of the stride that hit 0 and 2^12), the same with the sign set, +-0 and the largest finite float;
  - numpy's float32 statement of the chain is held against the threshold on the floats around R0 and on the special values, NaN included."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "cylindertag_amd", "csrc", "ctag_math.h")
LOG2E = np.float32(1.44269502162933349609375)
C = np.float32(1) / np.float32(2.9846)
ONE, TWO, FOUR, TWO_12, FLT_MAX = 0x3F800000, 0x40000000, 0x40800000, 0x45800000, 0x7F7FFFFF


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def chain_k_is_zero(r):
    """exp32_k_is_zero(-r * r * c * c) in numpy.float32, every product rounded to float as the kernel's is."""
    r = np.asarray(r, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a = -r * r * C * C
        return a * LOG2E >= np.float32(-0.5)


def bisect_r0():
    lo, hi = ONE, FOUR  # the chain's predicate holds at 1.0 and fails at 4.0
    assert chain_k_is_zero(_f32([lo]))[0] and not chain_k_is_zero(_f32([hi]))[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if chain_k_is_zero(_f32([mid]))[0] else (lo, mid)
    return lo


def header_constant():
    src = open(HEADER).read()
    m = re.search(r"constexpr float kWelschK0MaxDist = ([0-9.]+)f;", src)
    assert m, "kWelschK0MaxDist is not stated in ctag_math.h"
    assert re.search(r"CTM_HD bool welsch_k_is_zero\(float abs_r\) \{ return abs_r <= kWelschK0MaxDist; \}", src)
    return m.group(1)


def test_r0_found_by_bisection_is_the_headers_constant():
    bits = bisect_r0()
    r0 = _f32([bits])[0]
    text = header_constant()
    assert np.float32(text) == r0 and float(text) == float(r0), "header %s, bisection 0x%08x = %.30g" % (text, bits, r0)  # the decimal text is the float exactly
    assert bits == 0x3FE0E6FB and ONE < bits < TWO
    a = -r0 * r0 * C * C
    up = _f32([bits + 1])[0]
    assert np.rint(a * LOG2E) == 0 and np.rint((-up * up * C * C) * LOG2E) == -1


def test_numpy_statement_around_r0_and_at_the_special_values():
    bits = bisect_r0()
    r = _f32(np.arange(bits - 2 ** 16, bits + 2 ** 16, dtype=np.uint32))
    assert (chain_k_is_zero(r) == (r <= _f32([bits])[0])).all() and (chain_k_is_zero(-r) == (np.abs(r) <= _f32([bits])[0])).all()
    special = np.array([0.0, -0.0, 1e-45, 1.1754944e-38, 3.4028234663852886e38, -3.4028234663852886e38, np.inf, -np.inf], np.float32)
    assert list(chain_k_is_zero(special)) == [True, True, True, True, False, False, False, False]
    assert list(np.abs(special) <= _f32([bits])[0]) == [True, True, True, True, False, False, False, False]
    assert not chain_k_is_zero(np.float32(np.nan)) and not np.float32(np.nan) <= _f32([bits])[0]  # NaN fails both: the wave takes the general form


SWEEP = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ctag_math.h"
// argv: first last step (bit patterns of |r|, first <= last); for each |r| and for -|r|: the vote as k_welsch took it before (on the argument) and as it
// takes it now (on the distance).  Prints: visited holds mismatches first_bad
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const uint64_t first = std::strtoull(argv[1], nullptr, 0), last = std::strtoull(argv[2], nullptr, 0), step = std::strtoull(argv[3], nullptr, 0);
    if (step == 0 || first > last || last > 0x7f800000ull) return 2;
    const float c = 1 / 2.9846f;
    uint64_t visited = 0, holds = 0, bad = 0, first_bad = 0;
    for (uint64_t b = first; b <= last; b += step) {
        for (int neg = 0; neg < 2; neg++) {
            const float s = ctm::bits_to_f32((uint32_t)b | (neg ? 0x80000000u : 0u));
            const float r = ctm::fabs32(s);
            const bool before = ctm::exp32_k_is_zero(-r * r * c * c), now = ctm::welsch_k_is_zero(r);
            visited++;
            holds += now ? 1 : 0;
            if (before != now && bad++ == 0) first_bad = b;
        }
    }
    std::printf("%llu %llu %llu %llu\n", (unsigned long long)visited, (unsigned long long)holds, (unsigned long long)bad, (unsigned long long)first_bad);
    return 0;
}
"""


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    d = tmp_path_factory.mktemp("welsch_rzero")
    src, exe = d / "sweep.cpp", d / "sweep"
    src.write_text(SWEEP)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "cylindertag_amd", "csrc"), "-o", str(exe), str(src)], check=True)

    def run(first, last, step=1):
        out = subprocess.run([str(exe), str(first), str(last), str(step)], capture_output=True, check=True).stdout.split()
        return dict(zip(("visited", "holds", "mismatches", "first_bad"), (int(v) for v in out)))
    return run


def test_every_float_of_the_two_binades_around_r0(sweep):
    bits = bisect_r0()
    got = sweep(ONE, FOUR - 1)
    assert got["visited"] == 2 * 2 * 2 ** 23 and got["holds"] == 2 * (bits - ONE + 1) and 0 < got["holds"] < got["visited"]
    assert got["mismatches"] == 0, "first at bit pattern 0x%08x" % got["first_bad"]


def test_every_64th_float_elsewhere_up_to_two_to_the_twelfth(sweep):
    for first, last in ((0, ONE), (63, ONE - 1), (FOUR, TWO_12), (FOUR + 63, TWO_12 - 1)):  # two phases of the stride: 0, 1.0, 4.0 and 2^12 themselves are visited
        got = sweep(first, last, 64)
        assert got["visited"] == 2 * ((last - first) // 64 + 1) and got["holds"] == (got["visited"] if last <= ONE else 0)
        assert got["mismatches"] == 0, "first at bit pattern 0x%08x" % got["first_bad"]
    assert ONE % 64 == 0 and (TWO_12 - FOUR) % 64 == 0


def test_zeros_the_largest_finite_float_and_infinity(sweep):
    assert sweep(0, 0) == dict(visited=2, holds=2, mismatches=0, first_bad=0)  # +0 and -0
    assert sweep(FLT_MAX, FLT_MAX) == dict(visited=2, holds=0, mismatches=0, first_bad=0)  # r * r overflows to inf, the argument is -inf
    assert sweep(0x7F800000, 0x7F800000) == dict(visited=2, holds=0, mismatches=0, first_bad=0)
    bits = bisect_r0()
    for b in range(bits - 4, bits + 5):
        assert sweep(b, b) == dict(visited=2, holds=2 if b <= bits else 0, mismatches=0, first_bad=0)
