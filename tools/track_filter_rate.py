"""Track filtering rate on the device, by the method of tools/track_rate.py and in the same session as it: model-drawn
rig pose and covariance records (tests/track_shapes.py) in HBM, 8 % of the frames unmeasured, through ctag_rig_track_filter_device for
1 x 1, 1 x 16, 4096 x 1 and 4096 x 16 frames x rigs (a one-frame call is given again and again at growing times), and beside each the
smoother (ctag_rig_track_smooth_device, the default segment) on the same records.  Host clock around a synchronised call, median of 10
after 3 warm-ups, and the device's own time of the last filter call.  Then the time a step adds behind a one-frame detect + rig pose +
covariance chain on a rendered 1920 x 1080 frame.  Prints one JSON line per measurement.
usage (GPU): python tools/track_filter_rate.py"""
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
from dense_testlib import COLS, K_PLANTED, ROWS  # noqa: E402
from rig_rate import timed  # noqa: E402
import track_shapes as sh  # noqa: E402


def main():
    import torch
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    det.set_option(capi.OPT_TIMING, 1)
    rng = np.random.default_rng(3)
    for n_frames, n_rigs in ((1, 1), (1, 16), (4096, 1), (4096, 16)):
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
        stat = torch.zeros(n_rigs * capi.TRACK_STAT_DT.itemsize, dtype=torch.uint8, device="cuda")
        rigs = sh.RigSet(n_rigs)
        o = {k: v for k, v in b["opts"].items() if k != "max_gap"}
        F = det.track_filter(rigs, capi.track_filter_opts(max_gap=b["opts"]["max_gap"], **o))
        clock = [0.0]

        def step():
            t = clock[0] + np.arange(n_frames) / 30.0
            clock[0] = t[-1] + 1.0 / 30.0
            F.step_device(dP.data_ptr(), dQ.data_ptr(), out.data_ptr(), n_frames, times=t)

        tf = timed(step, det.sync)
        ms = F.track_filter_last_ms()
        ok = int((out.cpu().numpy().view(capi.TRACK_DT)["status"] == capi.TRACK_OK).sum())
        F.close()
        ts_ = timed(lambda: det.smooth_rig_track_device(rigs, dP.data_ptr(), dQ.data_ptr(), n_frames, out.data_ptr(), stat.data_ptr(),
                                                        opts=sh.track_opts(b)), det.sync)
        print(json.dumps({"n_frames": n_frames, "n_rigs": n_rigs, "filter_seconds": tf, "filter_device_ms": ms, "filter_us_per_frame": 1e6 * tf / n_frames,
                          "frames_ok": ok, "smoother_seconds": ts_, "smoother_device_ms": det.track_last_ms()["total"]}), flush=True)
    # the step behind a one-frame chain
    M, _ = tk.synth3d_model(state)
    K = K_PLANTED.copy()
    K[0, 2] -= 0.5
    K[1, 2] -= 0.5
    cam = ca.make_camera(K, np.zeros(5))
    nr = state.shape[0]
    rigs = ca.Rigs(M, np.arange(nr, dtype=np.int32))
    frame = torch.empty((1, ROWS, COLS), dtype=torch.uint8, device="cuda")
    det.synth3d_frames_device(frame.data_ptr(), 0, 1, ROWS, COLS, COLS, ROWS * COLS, K_PLANTED)
    res = torch.zeros(ca.RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    poses = torch.zeros(nr * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    covs = torch.zeros(nr * ca.POSE_COV_DT.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.zeros(nr * capi.TRACK_DT.itemsize, dtype=torch.uint8, device="cuda")
    F = det.track_filter(rigs, None)

    def chain(with_step):
        det.detect_batch_device(frame.data_ptr(), 1, ROWS, COLS, COLS, ROWS * COLS, res.data_ptr(), 5, True, 5)
        det.rig_pose_batch_device(res.data_ptr(), 1, M, rigs, cam, poses.data_ptr())
        det.rig_pose_cov_batch_device(res.data_ptr(), 1, M, rigs, cam, poses.data_ptr(), covs.data_ptr())
        if with_step:
            F.step_device(poses.data_ptr(), covs.data_ptr(), out.data_ptr())

    t0 = timed(lambda: chain(False), det.sync)
    t1 = timed(lambda: chain(True), det.sync)
    print(json.dumps({"chain": "detect + rig pose + cov, one 1920x1080 frame, %d rigs" % nr, "chain_seconds": t0, "chain_and_step_seconds": t1,
                      "step_adds_us": 1e6 * (t1 - t0)}), flush=True)
    F.close()
    det.close()


if __name__ == "__main__":
    main()
