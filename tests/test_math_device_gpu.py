"""The device build of cylindertag_amd/csrc/ctag_math.h at the edges of its functions' domains: for every op of the math probe the bits of the
gfx950 build are the bits of the host build on exactly the argument sets tests/test_math_statement_cpu.py measures against mpmath -- the doubles next
to k pi/2 up to rem_pio2_64's limit, the exponent shortcut and range breaks of atan2, the clamps of exp, subnormals, signed zeros, infinities and
NaN (a NaN equals any NaN: payloads are not part of the contract).  The broad random sets stay in tests/test_gpu_parity.py.  ctm::div64, the one
function whose device form differs from the host's, is held to Python's correctly rounded a / d at the corners of its documented domain."""
import numpy as np
import pytest

import math_shapes as ms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", range(19))
def test_device_bits_are_host_bits_at_the_edges(detector, oracle, op):
    x, y = ms.device_sets()[op]
    g, c = detector.math(op, x, y), oracle.math(op, x, y)
    bad = np.flatnonzero(~((g.view(np.uint64) == c.view(np.uint64)) | (np.isnan(g) & np.isnan(c))))
    assert 20 <= len(x) < 40000
    assert not len(bad), "math op %d: %d of %d differ, the first at (%r, %r): gfx950 %r, x86-64 %r" % (op, len(bad), len(x), x[bad[0]], y[bad[0]], g[bad[0]], c[bad[0]])


def test_div64_at_the_corners_of_its_domain(detector):
    """|d| at 2^-500 and at 2^500, |a| = 2^500 |d|, a / d at 2^-500, a = 0: the shared-reciprocal form gives the correctly rounded quotient"""
    a, d = ms.div64_corners()
    got = detector.math(ms.OP_DIV64, a, d)
    want = np.array([float(p) / float(q) for p, q in zip(a, d)])
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert not len(bad), "%d of %d differ, the first: %r / %r = %r, the device gave %r" % (len(bad), len(a), a[bad[0]], d[bad[0]], want[bad[0]], got[bad[0]])
