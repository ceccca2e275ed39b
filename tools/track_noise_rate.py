"""Track noise fit rate on the device, by the method of tools/track_filter_rate.py: model-drawn rig pose and
covariance records (tests/track_shapes.py) in HBM, 8 % of the frames unmeasured, for 600 x 1, 4096 x 1 and 4096 x 16 frames x rigs,
per rig and pooled: one round (rounds = 1) and a whole default fit (10 rounds, three free axes, 125 candidates a search) through
ctag_rig_track_noise_fit_device, and beside each one batch call of the filter (ctag_rig_track_filter_device) on the same records in the
same session.  Host clock around a synchronised call, median of 10 after 3 warm-ups, and the device's own time of the last call.
Prints one JSON line per measurement.
usage (GPU): python tools/track_noise_rate.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cylindertag_amd as ca  # noqa: E402
import testkit as tk  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from ctag_testlib import GOLDEN  # noqa: E402
from rig_rate import timed  # noqa: E402
import track_shapes as sh  # noqa: E402


def main():
    import torch
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    det.set_option(capi.OPT_TIMING, 1)
    rng = np.random.default_rng(3)
    for n_frames, n_rigs in ((600, 1), (4096, 1), (4096, 16)):
        masks = []
        for g in range(n_rigs):
            m = rng.random(n_frames) >= 0.08
            m[0] = m[-1] = True
            masks.append(m)
        b = sh.make_batch("rate", 30 + n_rigs, n_frames, masks, ["mixed"] * n_rigs)
        P, Q = sh.to_records(b)
        dP, dQ = torch.from_numpy(P.view(np.uint8)).cuda(), torch.from_numpy(Q.view(np.uint8)).cuda()
        n = n_frames * n_rigs
        out = torch.zeros(n * capi.TRACK_DT.itemsize, dtype=torch.uint8, device="cuda")
        nout = torch.zeros(n_rigs * capi.TRACK_NOISE_DT.itemsize, dtype=torch.uint8, device="cuda")
        rigs = sh.RigSet(n_rigs)
        o = {k: v for k, v in b["opts"].items() if k != "max_gap"}
        F = det.track_filter(rigs, capi.track_filter_opts(max_gap=b["opts"]["max_gap"], **o))
        clock = [0.0]

        def step():
            t = clock[0] + np.arange(n_frames) / 30.0
            clock[0] = t[-1] + 1.0 / 30.0
            F.step_device(dP.data_ptr(), dQ.data_ptr(), out.data_ptr(), n_frames, times=t)

        tf = timed(step, det.sync)
        fms = F.track_filter_last_ms()
        F.close()
        for mode, mname in ((capi.NOISE_PER_RIG, "per_rig"), (capi.NOISE_POOLED, "pooled")):
            row = {"n_frames": n_frames, "n_rigs": n_rigs, "mode": mname, "filter_batch_seconds": tf, "filter_batch_device_ms": fms}
            for rounds, key in ((1, "one_round"), (10, "fit")):
                opts = capi.track_noise_opts(mode=mode, rounds=rounds, max_gap=b["opts"]["max_gap"], **o)
                t = timed(lambda: det.fit_track_noise_device(rigs, dP.data_ptr(), dQ.data_ptr(), n_frames, nout.data_ptr(), opts=opts), det.sync)
                row[key + "_seconds"], row[key + "_device_ms"] = t, det.track_noise_last_ms()
            rec = nout.cpu().numpy().view(capi.TRACK_NOISE_DT)[:1 if mode == capi.NOISE_POOLED else n_rigs]
            row.update(items_a_round=125 * n_rigs, status=[int(v) for v in rec["status"][:4]], q_rot=float(rec["q_rot"][0]), q_trans=float(rec["q_trans"][0]),
                       cov_scale=float(rec["cov_scale"][0]), mean_m2=float(rec["mean_m2"][0]))
            print(json.dumps(row), flush=True)
    det.close()


if __name__ == "__main__":
    main()
