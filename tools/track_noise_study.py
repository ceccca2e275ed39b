"""What the track noise fit gives on the live sequences of tools/track_filter_study.py (needs the GPU).  The same six
hand-held-like trajectories and records (tools/track_study.py: a rig of three stacked golden models, units mm, 30 frames a second, 0.2 px
of noise, every 25th frame a loss of 1 to 4 frames) go through ctag_rig_track_noise_fit:
    per trajectory     the fitted q_rot, q_trans and cov_scale with their sigmas (octaves), mean_m2, and the same at the defaults
    leave one out      the pooled fit of the five other trajectories, applied to the sixth: the filtered rms against the raw poses'; the
                       good frames refused at gates 3 / 4 / 5 / 6 / 8, against the defaults'; and with one measured pose in fifty replaced
                       by a grossly wrong one, per gate, the rms at the good frames and the wrong / good poses refused
    surface            a 17 x 17 slice of L over (q_rot, q_trans), one octave a step around the fitted values at the fitted scale, of the
                       first trajectory, through the score call: the number of local minima of the slice and where the smallest lies
Prints one JSON line per row.

    python tools/track_noise_study.py [--tracks 6] [--frames 600]
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
GATED = capi.TRACK_FLAG_GATED


def rms(v):
    return round(float(np.sqrt(np.mean(np.asarray(v) ** 2))), 4) if len(v) else None


class CountRigs:
    """n one-model rigs: the calls only read n_rigs"""

    def __init__(self, n):
        self.model = ca.Model(ids=np.arange(n), corners=np.zeros((n, 8, 3)), model_size=1)
        self.rigs = ca.Rigs(self.model, np.arange(n, dtype=np.int32), n)
        self.r, self.n_rigs = self.rigs.r, n


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
    for i, f0 in enumerate(range(20, n - 10, 25)):
        lost[f0:f0 + 1 + i % 4] = True
    one = CountRigs(1)
    data = []
    for track in range(a.tracks):   # the records of tools/track_filter_study.py, seed for seed
        rng = np.random.default_rng(4000 + track)
        R, t = trajectory(rng, centre, n)
        recs = plant(rng, model, K, dist, R, t, lost)
        d = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).cuda()
        poses = torch.zeros(n * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
        cov = torch.zeros(n * ca.POSE_COV_DT.itemsize, dtype=torch.uint8, device="cuda")
        det.rig_pose_batch_device(d.data_ptr(), n, M, rigs, cam, poses.data_ptr())
        det.rig_pose_cov_batch_device(d.data_ptr(), n, M, rigs, cam, poses.data_ptr(), cov.data_ptr())
        det.sync()
        data.append(dict(P=poses.cpu().numpy().view(ca.RIG_POSE_DT).copy(), Q=cov.cpu().numpy().view(ca.POSE_COV_DT).copy(), R=R, t=t, rng=rng))
    nopts = dict(dt=1.0 / FPS)

    def run_filter(P, Q, s, **opts):
        F = det.track_filter(one, capi.track_filter_opts(dt=1.0 / FPS, **opts))
        try:
            F.set_cov_scale(s)
            return F.step(P, Q, n)[:, 0]
        finally:
            F.close()

    def row_of(rec):
        return dict(status=int(rec["status"]), q_rot=float(rec["q_rot"]), q_trans=float(rec["q_trans"]), cov_scale=float(rec["cov_scale"]),
                    log2_sigma=[round(float(v), 4) for v in rec["log2_sigma"]], mean_m2=round(float(rec["mean_m2"]), 3), flags=int(rec["flags"]),
                    score=float(rec["score"]), score_start=float(rec["score_start"]), n_terms=int(rec["n_terms"]))

    # ---- per trajectory ----
    own = []
    for k, D in enumerate(data):
        rec = det.fit_track_noise(one, D["P"], D["Q"], n, opts=capi.track_noise_opts(**nopts))[0]
        own.append(rec)
        at_default = det.fit_track_noise(one, D["P"], D["Q"], n, opts=capi.track_noise_opts(free_mask=0, rounds=1, **nopts))[0]
        print(json.dumps(dict(per_trajectory=k, default_mean_m2=round(float(at_default["mean_m2"]), 3), **row_of(rec))), flush=True)
    # ---- leave one out, pooled ----
    tot = {}

    def add(key, **kv):
        e = tot.setdefault(key, {})
        for name, v in kv.items():
            if isinstance(v, (list, np.ndarray)):
                e.setdefault(name, []).extend(list(v))
            else:
                e[name] = e.get(name, 0) + int(v)

    for k, D in enumerate(data):
        others = [j for j in range(len(data)) if j != k]
        if others:
            P = np.stack([data[j]["P"] for j in others], 1).copy()
            Q = np.stack([data[j]["Q"] for j in others], 1).copy()
            P["rig"] = np.arange(len(others))[None, :]
            rec = det.fit_track_noise(CountRigs(len(others)), P, Q, n, opts=capi.track_noise_opts(mode=capi.NOISE_POOLED, **nopts))[0]
        else:
            rec = own[k]
        print(json.dumps(dict(leave_out=k, **row_of(rec))), flush=True)
        fit = dict(q_rot=float(rec["q_rot"]), q_trans=float(rec["q_trans"]))
        s = float(rec["cov_scale"])
        P, Q, R, t, rng = D["P"], D["Q"], D["R"], D["t"], D["rng"]
        ok = P["status"] == 0
        er, et = errors(P["rvec"][ok], P["tvec"][ok], R[ok], t[ok])
        add("raw", rot=er, trans=et)
        for name, s_, o in (("default", 1.0, {}), ("fitted", s, fit)):
            G = run_filter(P, Q, s_, **o)
            er, et = errors(G["rvec"], G["tvec"], R, t)
            tr = ok & (G["status"] == 0)
            add(name, rot=er[tr], trans=et[tr], m2=G["mahalanobis2"][tr & ((G["flags"] & capi.TRACK_FLAG_STARTED) == 0)])
            for gate in GATES:
                G = run_filter(P, Q, s_, gate=gate, **o)
                add((name, gate), good=ok.sum(), good_refused=((G["flags"] & GATED) != 0).sum())
        W = P.copy()   # one measured pose in fifty grossly wrong, as tools/track_filter_study.py plants them
        wrong = np.flatnonzero(ok)[25::50]
        for f in wrong:
            ax = rng.normal(0, 1, 3)
            ax /= np.linalg.norm(ax)
            W["rvec"][f] = so3_log(so3_exp(np.radians(rng.uniform(20, 125)) * ax) @ so3_exp(P["rvec"][f]))
            W["tvec"][f] = P["tvec"][f] + rng.normal(0, 1, 3) * rng.uniform(20, 200) / np.sqrt(3)
        is_wrong = np.zeros(n, bool)
        is_wrong[wrong] = True
        good = ok & ~is_wrong
        for name, s_, o in (("default", 1.0, {}), ("fitted", s, fit)):
            for gate in (0.0,) + GATES:
                G = run_filter(W, Q, s_, gate=gate, **o)
                tr = G["status"] == 0
                er, et = errors(G["rvec"], G["tvec"], R, t)
                gated = (G["flags"] & GATED) != 0
                add(("wrong", name, gate), rot=er[good & tr], trans=et[good & tr], wrong=is_wrong.sum(), wrong_refused=(gated & is_wrong).sum(),
                    good_refused=(gated & good).sum(), good_not_tracked=(good & ~tr).sum())
    for key in ("raw", "default", "fitted"):
        e = tot[key]
        print(json.dumps(dict(clean=key, frames=len(e["rot"]), rot_deg=rms(e["rot"]), trans_mm=rms(e["trans"]),
                              mean_m2=None if "m2" not in e else round(float(np.mean(e["m2"])), 3))), flush=True)
    for name in ("default", "fitted"):
        for gate in GATES:
            print(json.dumps(dict(clean_gate=gate, values=name, **tot[(name, gate)])), flush=True)
    for name in ("default", "fitted"):
        for gate in (0.0,) + GATES:
            e = dict(tot[("wrong", name, gate)])
            print(json.dumps(dict(wrong_poses_gate=gate, values=name, rot_deg=rms(e.pop("rot")), trans_mm=rms(e.pop("trans")), **e)), flush=True)
    # ---- the surface around the first trajectory's own fit ----
    rec, D = own[0], data[0]
    u = np.arange(-8, 9, dtype=np.float64)
    cands = np.array([[rec["q_rot"] * 2.0 ** a_, rec["q_trans"] * 2.0 ** b_, rec["cov_scale"]] for a_ in u for b_ in u])
    Ls = np.concatenate([det.score_track_noise(one, D["P"], D["Q"], n, cands[i:i + 64], opts=capi.track_noise_opts(**nopts))[:, 0] for i in range(0, len(cands), 64)])
    L = np.where(Ls["n_singular"] == 0, Ls["L"], np.inf).reshape(17, 17)
    minima = []
    for i in range(17):
        for j in range(17):
            nb = [L[p, q] for p in range(max(i - 1, 0), min(i + 2, 17)) for q in range(max(j - 1, 0), min(j + 2, 17)) if (p, q) != (i, j)]
            if np.isfinite(L[i, j]) and all(L[i, j] < v for v in nb):
                minima.append((int(u[i]), int(u[j])))
    print(json.dumps(dict(surface="17x17 octaves around the fit of trajectory 0", local_minima=minima, singular_cells=int((Ls["n_singular"] != 0).sum()),
                          L_minus_min_along_q_rot=[round(float(v), 1) for v in L[:, 8] - L.min()],
                          L_minus_min_along_q_trans=[round(float(v), 1) for v in L[8, :] - L.min()])), flush=True)
    det.close()


if __name__ == "__main__":
    main()
