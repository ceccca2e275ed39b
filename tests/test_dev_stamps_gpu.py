"""The developer phase clocks (CTAG_CCL_STAMPS / CTAG_QUAD_STAMPS / CTAG_FEAT_STAMPS): with all three on, the chain synchronises inside itself, runs without
graph capture and prints a line per kernel family -- and the records must still equal the oracle's byte for byte.  The switches are read at a process's first
call, so tests/variant_worker.py runs once in a child process, on the default library: test.bmp and sequence frames one per call, a 32-frame batch at chunk
1024 and chunk 5, three odd sizes (both kernel families, a few seconds of GPU time).

PREFIXES is what the commit before the clocks' host code became one helper (`Stamps`, ctag_internal.h) printed for this very command (docs/history.md, "Device
layer"): the lines are quoted by tools/ and docs/, so the set is pinned, not derived from the build under test."""
import json
import os
import re
import subprocess
import sys

import pytest

from ctag_testlib import ROOT

pytestmark = pytest.mark.gpu

PREFIXES = frozenset([
    "[k_threshold_ccl cycles]",
    "[packed]", "[packed cycles]", "[whole-wave]", "[whole-wave cycles]", "[whole-wave rdp ticks]", "[whole-wave expand_line]",
    "[k_welsch]",
    "[k_features ticks]", "[k_markers ticks]",
])


def test_records_equal_the_oracle_with_every_phase_clock_on():
    env = dict(os.environ)
    env.pop("CTAG_HIP_LIB", None)
    env.update(CTAG_CCL_STAMPS="1", CTAG_QUAD_STAMPS="1", CTAG_FEAT_STAMPS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "variant_worker.py"), "--welsch", "0", "--lanes", "8"],
                       capture_output=True, text=True, timeout=300, env=env)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert lines, p.stderr[-3000:]
    rep = json.loads(lines[-1])
    assert p.returncode == 0 and rep["mismatches"] == [], rep
    seen = set(m.group(0) for m in (re.match(r"\[[^\]]*\]", l) for l in p.stderr.splitlines()) if m)
    assert seen == PREFIXES, sorted(seen ^ PREFIXES)
