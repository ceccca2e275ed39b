"""What track smoothing is worth, and which q to start from (needs the GPU).  A rig of three stacked copies of the
golden model (units: mm) is carried along smooth hand-held-like trajectories that are NOT drawn from the smoother's model: a base pose
plus sums of three sinusoids of 0.2 - 1.3 Hz, 0.12 rad and 25 / 25 / 50 mm in all, at 30 frames a second.  Every frame is planted as
tools/rig_study.py plants one (three consecutive features per marker, 0.2 px of pixel noise), every 25th frame starts a loss of 1, 2, 3
or 4 frames, and the records go through ctag_rig_pose_batch_device, ctag_rig_pose_cov_batch_device and ctag_rig_track_smooth_device.
Reported per (q_rot, q_trans): the rms rotation (degrees) and translation (mm) error of the raw and of the smoothed poses at the
measured frames, and of the bridged frames by length of the loss, over all trajectories.

    python tools/track_study.py [--tracks 6] [--frames 600]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import cylindertag_amd as ca  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from ctag_testlib import GOLDEN, RESULT_DT  # noqa: E402
from pose_testlib import golden_camera_and_model  # noqa: E402
from rig_testlib import add_marker, project, rot_err_deg, stacked_rig_model  # noqa: E402
from track_statement import so3_exp, so3_log  # noqa: E402

Q_ROT = (1e-4, 1e-3, 1e-2, 0.1, 1.0, 10.0)          # rad^2 / s^3
Q_TRANS = (1e2, 3e2, 1e3, 3e3, 1e4, 3e4, 1e5)          # mm^2 / s^3
FPS, FEATURES, NOISE_PX = 30.0, 3, 0.2


def trajectory(rng, centre, n):
    """(R [n, 3, 3], t [n, 3]): the rig frame's pose in the camera frame"""
    tt = np.arange(n) / FPS
    rot, tr = np.zeros((n, 3)), np.zeros((n, 3))
    for _ in range(3):
        f, ph = rng.uniform(0.2, 1.3, 6), rng.uniform(0, 2 * np.pi, 6)
        rot += 0.04 * np.sin(2 * np.pi * f[:3] * tt[:, None] + ph[:3])
        tr += np.array([25.0, 25.0, 50.0]) / 3 * np.sin(2 * np.pi * f[3:] * tt[:, None] + ph[3:])
    R0 = so3_exp(rng.normal(0, 0.2, 3))
    R = np.array([so3_exp(rot[k]) @ R0 for k in range(n)])
    t = np.array([centre - R[k] @ centre + tr[k] for k in range(n)])
    return R, t


def plant(rng, model, K, dist, R, t, lost):
    n = len(R)
    recs = np.zeros(n, RESULT_DT)
    for k in range(n):
        if lost[k]:
            recs[k]["status"] = 1
            continue
        r = np.zeros((), RESULT_DT)
        rv = so3_log(R[k])
        for mi in range(len(model["ids"])):
            X = model["corners"][mi].astype(np.float64)
            pts = project(K, dist, rv, t[k], X) + rng.normal(0, NOISE_PX, (X.shape[0], 2))
            p0 = int(rng.integers(0, model["size"] - FEATURES + 1))
            add_marker(r, int(model["ids"][mi]), mi, model, pts, p0, FEATURES, ((3, 4),), rng)
        recs[k] = r
    return recs


def errors(rvec, tvec, R, t):
    return np.array([rot_err_deg(rvec[k], so3_log(R[k])) for k in range(len(R))]), np.linalg.norm(tvec - t, axis=1)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tracks", type=int, default=6)
    ap.add_argument("--frames", type=int, default=600)
    a = ap.parse_args()
    K, dist, golden = golden_camera_and_model()
    model = stacked_rig_model(golden, 3, 70.0)
    centre = model["corners"].reshape(-1, 3).astype(np.float64).mean(0)
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = ca.Detector(state, fs, device=0)
    M = ca.Model(ids=model["ids"], corners=model["corners"], model_size=model["size"], base=model["base"], axis=model["axis"])
    cam = ca.load_camera(os.path.join(GOLDEN, "cameraParams.yml"))
    rigs = ca.Rigs(M, np.zeros(len(model["ids"]), np.int32))
    n = a.frames
    lost = np.zeros(n, bool)
    gap_of = np.zeros(n, np.int32)
    for i, f0 in enumerate(range(20, n - 10, 25)):
        g = 1 + i % 4
        lost[f0:f0 + g] = True
        gap_of[f0:f0 + g] = g
    acc = {}   # (q_rot, q_trans) -> lists of squared errors
    raw = {"rot": [], "tr": []}
    for track in range(a.tracks):
        rng = np.random.default_rng(4000 + track)
        R, t = trajectory(rng, centre, n)
        recs = plant(rng, model, K, dist, R, t, lost)
        d = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).cuda()
        poses = torch.zeros(n * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
        cov = torch.zeros(n * ca.POSE_COV_DT.itemsize, dtype=torch.uint8, device="cuda")
        out = torch.zeros(n * ca.TRACK_DT.itemsize, dtype=torch.uint8, device="cuda")
        stat = torch.zeros(capi.TRACK_STAT_DT.itemsize, dtype=torch.uint8, device="cuda")
        det.rig_pose_batch_device(d.data_ptr(), n, M, rigs, cam, poses.data_ptr())
        det.rig_pose_cov_batch_device(d.data_ptr(), n, M, rigs, cam, poses.data_ptr(), cov.data_ptr())
        det.sync()
        P = poses.cpu().numpy().view(ca.RIG_POSE_DT)
        ok = P["status"] == 0
        assert (ok == ~lost).all()
        er, et = errors(P["rvec"][ok], P["tvec"][ok], R[ok], t[ok])
        raw["rot"] += list(er ** 2)
        raw["tr"] += list(et ** 2)
        for qr in Q_ROT:
            for qt in Q_TRANS:
                opts = ca.track_opts(q_rot=qr, q_trans=qt, dt=1.0 / FPS, max_gap=5)
                det.smooth_rig_track_device(rigs, poses.data_ptr(), cov.data_ptr(), n, out.data_ptr(), stat.data_ptr(), opts=opts)
                det.sync()
                S = out.cpu().numpy().view(ca.TRACK_DT)
                assert (S["status"] == 0).all()
                er, et = errors(S["rvec"], S["tvec"], R, t)
                e = acc.setdefault((qr, qt), {"rot": [], "tr": [], "gap": {g: [[], []] for g in (1, 2, 3, 4)}})
                e["rot"] += list(er[ok] ** 2)
                e["tr"] += list(et[ok] ** 2)
                for g in (1, 2, 3, 4):
                    e["gap"][g][0] += list(er[gap_of == g] ** 2)
                    e["gap"][g][1] += list(et[gap_of == g] ** 2)
    rms = lambda v: float(np.sqrt(np.mean(v)))  # noqa: E731
    print(json.dumps({"raw": True, "frames": len(raw["rot"]), "rot_deg": round(rms(raw["rot"]), 4), "trans_mm": round(rms(raw["tr"]), 3)}), flush=True)
    for (qr, qt), e in sorted(acc.items()):
        print(json.dumps({"q_rot": qr, "q_trans": qt, "rot_deg": round(rms(e["rot"]), 4), "trans_mm": round(rms(e["tr"]), 3),
                          "bridged_rot_deg": {g: round(rms(e["gap"][g][0]), 4) for g in (1, 2, 3, 4)},
                          "bridged_trans_mm": {g: round(rms(e["gap"][g][1]), 3) for g in (1, 2, 3, 4)}}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
