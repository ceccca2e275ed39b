"""Batches of six small synthetic frames through the split form of edgeRefine (k_edge_refine<1>, k_edge_refine_sums, k_edge_refine_tail) against the
oracle: the refined features (CTAG_DBG_FEATURES2) and the result records byte for byte, at cornerSubPixDist 5 and 0.  tests/test_refine_sums_frames_gpu.py
calls `compare` in its own process for the default build, and runs this file as a child process for a build with a compile-time switch (CTAG_HIP_LIB, set by
the parent before anything imports the binding: the binding loads ONE library per process).  Prints one JSON line; exit code 1 on any difference."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, FRAMES = 720, 1280, 6
DISTS = (5, 0)


def compare(det, orc, state, fs):
    """-> dict(plan form, frames, features compared, mismatches: [text])"""
    import testkit as tk
    plan = tk.chunk_plan(rows=ROWS, cols=COLS, nframes=FRAMES)
    frames = np.stack([tk.synth_frame_host(state, 20 + f, rows=ROWS, cols=COLS)[0] for f in range(FRAMES)])
    bad, features, ok_frames = [], 0, 0
    for dist in DISTS:
        got = det.detect_batch(frames, subpix_dist=dist)
        for f in range(FRAMES):
            o = orc.detect(frames[f], state, fs, subpix=True, subpix_dist=dist)
            if got[f].tobytes() != np.asarray(o["result"]).tobytes():
                bad.append("dist %d frame %d: the result record differs from the oracle's" % (dist, f))
            if o["status"] != 0:
                continue
            ok_frames += 1
            k2 = det.debug(f, tk.DBG_FEATURES2)
            features += len(k2)
            if k2.tobytes() != o["features"][2].tobytes():
                bad.append("dist %d frame %d: the refined features differ from the oracle's" % (dist, f))
    return {"refine": plan["refine"], "refine_sums_gx": plan["refine_sums_gx"], "frames": ok_frames, "features": features, "mismatches": bad}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import testkit as tk
    from ctag_testlib import GOLDEN, Oracle, read_marker_file
    state, fs = read_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    rep = compare(det, Oracle(), state, fs)
    det.close()
    rep["lib"] = os.environ.get("CTAG_HIP_LIB", "default")
    print(json.dumps(rep), flush=True)
    return 1 if rep["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())
