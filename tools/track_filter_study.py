"""What the track filter is worth on a live sequence, and which gate to start from (needs the GPU).  The six
hand-held-like trajectories of tools/track_study.py (not drawn from the filter's model; a rig of three stacked golden models, units mm,
30 frames a second, three features a marker with 0.2 px of noise, every 25th frame a loss of 1 to 4 frames) go through
ctag_rig_pose_batch_device and ctag_rig_pose_cov_batch_device, and the records through the filter at its default options and through the
smoother at its own.  Reported over all trajectories:
    clean        rotation (degrees) and translation (mm) rms of the raw, filtered and smoothed poses at the measured frames; of the
                 filter's and the smoother's bridged frames by length of the loss; of `predict` one and two frames ahead against holding
                 the last filtered pose; per gate 3, 4, 5, 6, 8 how many of the (correctly decoded) frames the gate refuses; and the
                 filtered rms and the same counts with q_rot and q_trans 10, 100 and 1000 times the defaults
    wrong poses  the same records with one measured pose in fifty replaced by a grossly wrong one (20 to 125 degrees and 20 to 200 mm off),
                 filtered without protection, under each gate, under Huber and under Cauchy (loss_scale 4): the rms at the good measured
                 frames, how many wrong poses were refused or downweighted, how many good frames were
The default gate is the smallest listed value that refuses no good frame in either table.

    python tools/track_filter_study.py [--tracks 6] [--frames 600]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import cylindertag_amd as ca  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from ctag_testlib import GOLDEN  # noqa: E402
from pose_testlib import golden_camera_and_model  # noqa: E402
from rig_testlib import stacked_rig_model  # noqa: E402
from track_statement import so3_exp, so3_log  # noqa: E402
from track_study import FPS, errors, plant, trajectory  # noqa: E402

GATES = (3.0, 4.0, 5.0, 6.0, 8.0)
Q_SCALES = (10.0, 100.0, 1000.0)
MEASURED, DOWN, GATED = capi.TRACK_FLAG_MEASURED, capi.TRACK_FLAG_DOWNWEIGHTED, capi.TRACK_FLAG_GATED


def rms(v):
    return float(np.sqrt(np.mean(v))) if len(v) else None


class Acc:
    def __init__(self):
        self.d = {}

    def add(self, key, er, et):
        e = self.d.setdefault(key, [[], []])
        e[0] += list(np.asarray(er) ** 2)
        e[1] += list(np.asarray(et) ** 2)

    def report(self, key):
        e = self.d.get(key, [[], []])
        return {"frames": len(e[0]), "rot_deg": None if not e[0] else round(rms(e[0]), 4), "trans_mm": None if not e[1] else round(rms(e[1]), 3)}


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
    times = np.arange(n) / FPS
    lost = np.zeros(n, bool)
    gap_of = np.zeros(n, np.int32)
    for i, f0 in enumerate(range(20, n - 10, 25)):
        g = 1 + i % 4
        lost[f0:f0 + g] = True
        gap_of[f0:f0 + g] = g
    acc = Acc()
    counts = {}

    def count(key, k, v):
        counts.setdefault(key, {}).setdefault(k, 0)
        counts[key][k] += int(v)

    def run_filter(P, Q, **opts):
        F = det.track_filter(rigs, capi.track_filter_opts(dt=1.0 / FPS, **opts))
        try:
            return F.step(P, Q, n)[:, 0]
        finally:
            F.close()

    for track in range(a.tracks):
        rng = np.random.default_rng(4000 + track)
        R, t = trajectory(rng, centre, n)
        recs = plant(rng, model, K, dist, R, t, lost)
        d = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).cuda()
        poses = torch.zeros(n * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
        cov = torch.zeros(n * ca.POSE_COV_DT.itemsize, dtype=torch.uint8, device="cuda")
        det.rig_pose_batch_device(d.data_ptr(), n, M, rigs, cam, poses.data_ptr())
        det.rig_pose_cov_batch_device(d.data_ptr(), n, M, rigs, cam, poses.data_ptr(), cov.data_ptr())
        det.sync()
        P = poses.cpu().numpy().view(ca.RIG_POSE_DT).copy()
        Q = cov.cpu().numpy().view(ca.POSE_COV_DT).copy()
        ok = P["status"] == 0
        assert (ok == ~lost).all()
        acc.add("raw", *errors(P["rvec"][ok], P["tvec"][ok], R[ok], t[ok]))
        S, _ = det.smooth_rig_track(rigs, P, Q, n, opts=ca.track_opts(dt=1.0 / FPS))
        S = S[:, 0]
        er, et = errors(S["rvec"], S["tvec"], R, t)
        acc.add("smoothed", er[ok], et[ok])
        for g in (1, 2, 3, 4):
            acc.add(("smoothed bridged", g), er[gap_of == g], et[gap_of == g])
        Fr = run_filter(P, Q)
        assert (Fr["status"] == 0).all()
        er, et = errors(Fr["rvec"], Fr["tvec"], R, t)
        acc.add("filtered", er[ok], et[ok])
        for g in (1, 2, 3, 4):
            acc.add(("filtered bridged", g), er[gap_of == g], et[gap_of == g])
        # predict one and two frames ahead, one frame a call, against holding the last filtered pose
        P1 = P.copy()
        P1["frame"] = 0
        F = det.track_filter(rigs, capi.track_filter_opts(dt=1.0 / FPS))
        for f in range(n - 2):
            now = F.step(P1[f:f + 1], Q[f:f + 1], 1, times=[times[f]])[0, 0]
            if now["status"] != 0:
                continue
            for ahead in (1, 2):
                pr = F.predict(times[f + ahead])[0]
                e1 = errors(pr["rvec"][None], pr["tvec"][None], R[f + ahead:f + ahead + 1], t[f + ahead:f + ahead + 1])
                e0 = errors(now["rvec"][None], now["tvec"][None], R[f + ahead:f + ahead + 1], t[f + ahead:f + ahead + 1])
                acc.add(("predict", ahead), *e1)
                acc.add(("hold", ahead), *e0)
        F.close()
        # the gates on the clean records: every frame is correctly decoded
        for gate in GATES:
            G = run_filter(P, Q, gate=gate)
            count(("clean", gate), "good_refused", ((G["flags"] & GATED) != 0).sum())
            count(("clean", gate), "good", ok.sum())
        # the same with the motion model loosened: q_rot and q_trans times 10, 100, 1000 (the defaults are the smoother's, which sees the future)
        for scale in Q_SCALES:
            q = dict(q_rot=0.1 * scale, q_trans=3000.0 * scale)
            G = run_filter(P, Q, **q)
            er, et = errors(G["rvec"], G["tvec"], R, t)
            acc.add(("q", scale), er[ok], et[ok])
            for gate in GATES:
                G = run_filter(P, Q, gate=gate, **q)
                count(("q", scale), "good_refused_gate_%g" % gate, ((G["flags"] & GATED) != 0).sum())
        # one measured pose in fifty grossly wrong
        W = P.copy()
        measured = np.flatnonzero(ok)
        wrong = measured[25::50]
        for f in wrong:
            ax = rng.normal(0, 1, 3)
            ax /= np.linalg.norm(ax)
            W["rvec"][f] = so3_log(so3_exp(np.radians(rng.uniform(20, 125)) * ax) @ so3_exp(P["rvec"][f]))
            W["tvec"][f] = P["tvec"][f] + rng.normal(0, 1, 3) * rng.uniform(20, 200) / np.sqrt(3)
        is_wrong = np.zeros(n, bool)
        is_wrong[wrong] = True
        good = ok & ~is_wrong
        variants = [("none", {})] + [("gate %g" % g, dict(gate=g)) for g in GATES] + [("huber", dict(loss=capi.LOSS_HUBER)), ("cauchy", dict(loss=capi.LOSS_CAUCHY))]
        for name, o in variants:
            G = run_filter(W, Q, **o)
            tracked = G["status"] == 0
            er, et = errors(G["rvec"], G["tvec"], R, t)
            acc.add(("wrong", name), er[good & tracked], et[good & tracked])
            hit = (G["flags"] & (GATED | DOWN)) != 0
            count(("wrong", name), "wrong", is_wrong.sum())
            count(("wrong", name), "wrong_refused_or_downweighted", (hit & is_wrong).sum())
            count(("wrong", name), "good_refused", (((G["flags"] & GATED) != 0) & good).sum())
            count(("wrong", name), "good_downweighted", (((G["flags"] & DOWN) != 0) & good).sum())
            count(("wrong", name), "good_not_tracked", (good & ~tracked).sum())
    for key in ("raw", "filtered", "smoothed"):
        print(json.dumps(dict(clean=key, **acc.report(key))), flush=True)
    for kind in ("filtered bridged", "smoothed bridged"):
        for g in (1, 2, 3, 4):
            print(json.dumps(dict(clean=kind, loss_frames=g, **acc.report((kind, g)))), flush=True)
    for ahead in (1, 2):
        print(json.dumps(dict(clean="ahead", frames_ahead=ahead, predict=acc.report(("predict", ahead)), hold=acc.report(("hold", ahead)))), flush=True)
    for gate in GATES:
        print(json.dumps(dict(clean="gate", gate=gate, **counts[("clean", gate)])), flush=True)
    for scale in Q_SCALES:
        print(json.dumps(dict(clean="q x %g" % scale, **acc.report(("q", scale)), **counts[("q", scale)])), flush=True)
    for name in ["none"] + ["gate %g" % g for g in GATES] + ["huber", "cauchy"]:
        print(json.dumps(dict(wrong_poses=name, **acc.report(("wrong", name)), **counts[("wrong", name)])), flush=True)
    free = [g for g in GATES if counts[("clean", g)]["good_refused"] == 0 and counts[("wrong", "gate %g" % g)]["good_refused"] == 0]
    print(json.dumps({"default_gate": free[0] if free else None}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
