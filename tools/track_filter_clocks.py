"""Where a step of the track filter spends its time, from the kernel's own clocks (needs the GPU).  The library is
built a second time with -DCTAG_TF_CLOCKS=1 into cylindertag_amd/_var/clocks (k_track_filter.hip then reads the 100 MHz clock at the phase
boundaries of its walk and prints the sums of block 0), and a child process that loads that build filters the 4096 x 1 batch of
tools/track_filter_rate.py in one call, then one frame in a call of its own.  The last of five calls of each kind is reported, in
microseconds and per frame.  The clock has a resolution of 10 ns; a phase is read some thousand times.
usage (GPU): python tools/track_filter_clocks.py"""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
VAR = os.path.join(ROOT, "cylindertag_amd", "_var", "clocks")
LIB = os.path.join(VAR, "libctag_hip.so")
PHASES = ("prepass", "predict", "innovation", "gain", "joseph", "record")


def child():
    import torch
    import cylindertag_amd as ca
    from cylindertag_amd import capi
    from ctag_testlib import GOLDEN
    import track_shapes as sh
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = ca.Detector(state, fs, device=0)
    rng = np.random.default_rng(3)
    for n_frames in (4096, 1):
        m = rng.random(n_frames) >= 0.08
        m[0] = m[-1] = True
        b = sh.make_batch("rate", 31, n_frames, [m], ["mixed"])
        P, Q = sh.to_records(b)
        dP, dQ = torch.from_numpy(P.view(np.uint8)).cuda(), torch.from_numpy(Q.view(np.uint8)).cuda()
        out = torch.zeros(n_frames * capi.TRACK_DT.itemsize, dtype=torch.uint8, device="cuda")
        o = {k: v for k, v in b["opts"].items()}
        F = det.track_filter(sh.RigSet(1), capi.track_filter_opts(**o))
        t0 = 0.0
        for _ in range(5):
            t = t0 + np.arange(n_frames) / 30.0
            t0 = t[-1] + 1.0 / 30.0
            F.step_device(dP.data_ptr(), dQ.data_ptr(), out.data_ptr(), n_frames, times=t)
            det.sync()
        F.close()
    det.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j16", "-C", os.path.join(ROOT, "cylindertag_amd"), "OUT=" + VAR, "EXTRA=-DCTAG_TF_CLOCKS=1", LIB])
    env = dict(os.environ, CTAG_HIP_LIB=LIB)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        sys.exit(p.stdout + p.stderr)
    last = {}
    for line in p.stdout.splitlines():
        g = re.match(r"tf_clocks frames (\d+) " + " ".join(k + r" (-?\d+)" for k in PHASES), line)
        if g:
            last[int(g.group(1))] = [int(v) for v in g.groups()[1:]]
    for n, ticks in sorted(last.items()):
        us = {k: v / 100.0 for k, v in zip(PHASES, ticks)}
        print(json.dumps({"n_frames": n, "total_us": round(sum(us.values()), 2), "us": {k: round(v, 2) for k, v in us.items()},
                          "us_per_frame": {k: round(v / n, 3) for k, v in us.items()}}), flush=True)


if __name__ == "__main__":
    main()
