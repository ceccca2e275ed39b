"""Hand-eye calibration rate on the device, by the method of tools/track_rate.py: n_frames frames of planted rig
pose and covariance records (tests/hand_eye_shapes.py) in HBM for 1 and 16 problems, 8 % of the frames unmeasured, fitted by
ctag_rig_hand_eye_fit_device with and without frame records.  Device-resident records; host clock around a synchronised call, median of
10 after 3 warm-ups, and the device's own split (ctag_hand_eye_last_ms) of the last call.  max_iterations = 20, the default.
Prints one JSON line per (frames, problems, frame records).
usage (GPU): python tools/hand_eye_rate.py [n_frames,... [problems,...]]"""
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
import hand_eye_shapes as sh  # noqa: E402


def main():
    import torch
    frame_counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [64, 4096]
    rig_counts = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 16]
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = ca.Detector(state, fs, device=0)
    det.set_option(capi.OPT_TIMING, 1)
    rng = np.random.default_rng(3)
    for n_frames in frame_counts:
        for n_rigs in rig_counts:
            masks = [rng.random(n_frames) >= 0.08 for _ in range(n_rigs)]
            b = sh.make_batch("rate", 60 + n_rigs, n_frames, masks, ["mixed"] * n_rigs)
            P, Q, K = sh.to_records(b)
            dP = torch.from_numpy(P.view(np.uint8)).cuda()
            dQ = torch.from_numpy(Q.view(np.uint8)).cuda()
            n = n_frames * n_rigs
            out = torch.zeros(n_rigs * capi.HAND_EYE_DT.itemsize, dtype=torch.uint8, device="cuda")
            frames = torch.zeros(n * capi.HAND_EYE_FRAME_DT.itemsize, dtype=torch.uint8, device="cuda")
            rigs = sh.RigSet(n_rigs)
            for with_frames in (False, True):
                fp = frames.data_ptr() if with_frames else None
                t = timed(lambda: det.fit_hand_eye_device(rigs, dP.data_ptr(), dQ.data_ptr(), n_frames, K, out.data_ptr(), fp), det.sync)
                R = out.cpu().numpy().view(capi.HAND_EYE_DT)
                print(json.dumps({"n_frames": n_frames, "n_problems": n_rigs, "frame_records": with_frames, "seconds": t, "items_per_s": n / t,
                                  "ok": int((R["status"] == capi.HE_OK).sum()), "rounds": [int(v) for v in R["rounds"]],
                                  "device_ms": det.hand_eye_last_ms()}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
