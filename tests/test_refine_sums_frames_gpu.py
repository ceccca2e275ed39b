"""The sums kernel inside the chain (-m gpu): batches of six small synthetic frames, the batch form of edgeRefine (a split form: searches, ordered sums,
lines and corners as kernels of their own), at cornerSubPixDist 5 and 0.  The refined features and the result records must equal the oracle's byte for
byte -- on the default build, and on the build with -DCTAG_REFINE_PLAIN_SYNC=1 (edgeRefine's LDS-only waits replaced by __syncthreads()), made the way
tests/test_variant_builds_gpu.py makes it and run in a child process (tests/refine_sums_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

import refine_sums_worker as worker
from ctag_testlib import ROOT

pytestmark = pytest.mark.gpu


def _held(rep):
    assert rep["refine"].startswith("split") and rep["refine_sums_gx"] == 12, rep  # the batch form, with the sums kernel
    assert not rep["mismatches"], rep
    assert rep["frames"] >= 8 and rep["features"] >= 150, rep                      # frames that had features to refine


def test_six_frame_batches_equal_the_oracle(oracle, dictionary):
    import testkit as tk
    state, fs = dictionary
    det = tk.Detector(state, fs, device=0)  # a handle of its own: default options, whatever ran before
    try:
        rep = worker.compare(det, oracle, state, fs)
    finally:
        det.close()
    print("\n%s" % rep)
    _held(rep)


def test_the_same_with_plain_barriers():
    out = os.path.join("_var", "plainsync")
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cylindertag_amd"), "OUT=" + out, "EXTRA=-DCTAG_REFINE_PLAIN_SYNC=1",
                           os.path.join(out, "libctag_hip.so")])
    env = dict(os.environ, CTAG_HIP_LIB=os.path.join(ROOT, "cylindertag_amd", out, "libctag_hip.so"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refine_sums_worker.py")], capture_output=True, text=True, timeout=600, env=env)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert lines, p.stderr[-3000:]
    rep = json.loads(lines[-1])
    print("\n%s" % rep)
    assert p.returncode == 0 and rep["lib"].endswith(os.path.join(out, "libctag_hip.so")), rep
    _held(rep)
