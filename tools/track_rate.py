"""Track smoothing rate on the device, by the method of tools/rig_rate.py: n_frames frames of model-drawn rig
pose and covariance records (tests/track_shapes.py) in HBM for 1, 4 and 16 rigs, 8 % of the frames unmeasured, smoothed by
ctag_rig_track_smooth_device for every allowed segment_frames.  Device-resident records; host clock around a synchronised call, median
of 10 after 3 warm-ups, and the device's own split (ctag_track_last_ms) of the last call.  max_iterations = 10, the default.
Prints one JSON line per (rigs, segment_frames).
usage (GPU): python tools/track_rate.py [n_frames [rigs,... [segment_frames,...]]]
    (one rig count and one segment length under a kernel tracer give the timeline of DESIGN.md section 21)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cylindertag_amd as ca  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from ctag_testlib import GOLDEN  # noqa: E402
from rig_rate import timed  # noqa: E402
import track_shapes as sh  # noqa: E402


def main():
    import torch
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    rig_counts = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 4, 16]
    segments = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [8, 16, 32, 64]
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = ca.Detector(state, fs, device=0)
    det.set_option(capi.OPT_TIMING, 1)
    rng = np.random.default_rng(3)
    for n_rigs in rig_counts:
        masks = []
        for g in range(n_rigs):
            m = rng.random(n_frames) >= 0.08
            m[0] = m[-1] = True
            masks.append(m)
        b = sh.make_batch("rate", 30 + n_rigs, n_frames, masks, ["mixed"] * n_rigs)
        P, Q = sh.to_records(b)
        dP = torch.from_numpy(P.view(np.uint8)).cuda()
        dQ = torch.from_numpy(Q.view(np.uint8)).cuda()
        n = n_frames * n_rigs
        out = torch.zeros(n * capi.TRACK_DT.itemsize, dtype=torch.uint8, device="cuda")
        stat = torch.zeros(n_rigs * capi.TRACK_STAT_DT.itemsize, dtype=torch.uint8, device="cuda")
        rigs = sh.RigSet(n_rigs)
        for L in segments:
            opts = sh.track_opts(b, segment_frames=L)
            t = timed(lambda: det.smooth_rig_track_device(rigs, dP.data_ptr(), dQ.data_ptr(), n_frames, out.data_ptr(), stat.data_ptr(), opts=opts), det.sync)
            S = stat.cpu().numpy().view(capi.TRACK_STAT_DT)
            print(json.dumps({"n_frames": n_frames, "n_rigs": n_rigs, "segment_frames": L, "seconds": t, "frames_x_tracks_per_s": n / t,
                              "pieces": int(S["n_pieces"].sum()), "tracked": int(S["n_tracked"].sum()), "rounds": int(S["rounds"].sum()),
                              "device_ms": det.track_last_ms()}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
