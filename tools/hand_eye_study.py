"""What the hand-eye fit does with the library's own records, and what the covariance weights and the losses are worth (DESIGN.md section
22; needs the GPU).  The ray-cast frames of tools/dense_study.py (cylinders with printed strips under planted rigid poses, 1920x1080,
f = 2600 px, four objects a frame) are rendered on the device and go through detect(img,5,true,5), ctag_rig_pose_batch_device (every
model a rig of its own) and ctag_rig_pose_cov_batch_device.  Object slot s of every frame is one hand-eye problem: transforms P and Q
are planted, and the arm is where the planted pose A_f of that object puts it, C_f = P^-1 o A_f o Q^-1, so that A_f = P o C_f o Q
holds exactly for the planted poses and the fit sees the detector's errors alone.  The link pose handed over is C_f (rig on the link) or
its inverse (camera on the link).  Reported per mode and variant, over the slots: the rotation (degrees) and translation (model units)
errors of P and Q against the planted transforms, sigma2_hat, and the frames flagged as downweighted:
    raw poses           the rig pose records themselves against the planted poses
    weighted            the covariance records as the library returns them; without a loss and under Cauchy
    W = I               every covariance replaced by the identity; without a loss and under Cauchy
    wrong links, loss   every tenth frame's link pose moved by 0.05 rad and 10 units; no loss, Huber, Cauchy (loss_scale 4)

    python tools/hand_eye_study.py [--frames 96]
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
import testkit as tk  # noqa: E402
from cylindertag_amd import capi  # noqa: E402
from ctag_testlib import GOLDEN  # noqa: E402
from dense_testlib import COLS, K_PLANTED, ROWS  # noqa: E402
from hand_eye_statement import so3_exp, so3_log  # noqa: E402
from track_shapes import RigSet  # noqa: E402

SLOTS = 4
WRONG_ROT, WRONG_TRANS = 0.05, 10.0


def compose(a, b):
    """a o b for (R, t) pairs"""
    return a[0] @ b[0], a[0] @ b[1] + a[1]


def inverse(a):
    return a[0].T, -(a[0].T @ a[1])


def rot_deg(R, Rt):
    return float(np.degrees(np.linalg.norm(so3_log(R @ Rt.T))))


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=96)
    a = ap.parse_args()
    n = a.frames
    state, fs = ca.load_marker_file(os.path.join(GOLDEN, "CTag_2f12c.marker"))
    det = tk.Detector(state, fs, device=0)
    M, _ = tk.synth3d_model(state)
    K = K_PLANTED.copy()
    K[0, 2] -= 0.5   # the renderer's pixel centres, as tools/dense_study.py
    K[1, 2] -= 0.5
    cam = ca.make_camera(K, np.zeros(5))
    n_models = state.shape[0]
    rigs = ca.Rigs(M, np.arange(n_models, dtype=np.int32))
    frames = torch.empty((n, ROWS, COLS), dtype=torch.uint8, device="cuda")
    det.synth3d_frames_device(frames.data_ptr(), 0, n, ROWS, COLS, COLS, ROWS * COLS, K_PLANTED)
    res = torch.zeros((n, ca.RESULT_DT.itemsize), dtype=torch.uint8, device="cuda")
    det.detect_batch_device(frames.data_ptr(), n, ROWS, COLS, COLS, ROWS * COLS, res.data_ptr(), 5, True, 5)
    poses = torch.zeros(n * n_models * ca.RIG_POSE_DT.itemsize, dtype=torch.uint8, device="cuda")
    covs = torch.zeros(n * n_models * ca.POSE_COV_DT.itemsize, dtype=torch.uint8, device="cuda")
    det.rig_pose_batch_device(res.data_ptr(), n, M, rigs, cam, poses.data_ptr())
    det.rig_pose_cov_batch_device(res.data_ptr(), n, M, rigs, cam, poses.data_ptr(), covs.data_ptr())
    det.sync()
    P_all = poses.cpu().numpy().view(ca.RIG_POSE_DT).reshape(n, n_models)
    Q_all = covs.cpu().numpy().view(ca.POSE_COV_DT).reshape(n, n_models)
    del frames
    truth = [tk.synth3d_frame_host(state, f, K_PLANTED, rows=ROWS, cols=COLS)[1] for f in range(n)]
    one = RigSet(1)
    rng = np.random.default_rng(77)
    acc = {}
    seen, raw = [], []
    for s in range(SLOTS):
        rec, cov = np.zeros((n, 1), ca.RIG_POSE_DT), np.zeros((n, 1), ca.POSE_COV_DT)
        A = []
        for f in range(n):
            t = truth[f]
            r = int(t["dict_row"][s]) if s < t["n_markers"] else 0
            rec[f, 0], cov[f, 0] = P_all[f, r], Q_all[f, r]
            if s >= t["n_markers"]:
                rec[f, 0]["status"] = capi.POSE_NOT_SEEN
            A.append((t["R"][s].reshape(3, 3).astype(np.float64), t["t"][s].astype(np.float64)))
        rec["rig"], rec["frame"][:, 0] = 0, np.arange(n)
        ok = (rec["status"][:, 0] == 0) & (cov["status"][:, 0] == 0)
        seen.append(int(ok.sum()))
        raw_rot = np.array([rot_deg(so3_exp(rec["rvec"][f, 0]), A[f][0]) for f in range(n) if ok[f]])
        raw_tr = np.array([np.linalg.norm(rec["tvec"][f, 0] - A[f][1]) for f in range(n) if ok[f]])
        raw.append({"slot": s, "frames": int(ok.sum()), "rot_deg_median": round(float(np.median(raw_rot)), 4), "rot_deg_max": round(float(raw_rot.max()), 3),
                    "frames_over_1_deg": int((raw_rot > 1.0).sum()), "trans_median": round(float(np.median(raw_tr)), 4), "trans_max": round(float(raw_tr.max()), 2)})
        Pt = (so3_exp(rng.normal(0, 0.8, 3)), rng.normal(0, 60.0, 3))
        Qt = (so3_exp(rng.normal(0, 0.8, 3)), rng.normal(0, 150.0, 3))
        Cf = [compose(compose(inverse(Pt), A[f]), inverse(Qt)) for f in range(n)]
        wrong = np.zeros(n, bool)
        wrong[5::10] = True
        for mode in (capi.HAND_EYE_CAMERA_ON_LINK, capi.HAND_EYE_RIG_ON_LINK):
            def links(spoiled):
                K_ = np.zeros(n, capi.LINK_POSE_DT)
                for f in range(n):
                    c = Cf[f]
                    if spoiled and wrong[f]:
                        c = compose((so3_exp(rng.normal(0, WRONG_ROT / np.sqrt(3), 3)), rng.normal(0, WRONG_TRANS / np.sqrt(3), 3)), c)
                    lk = inverse(c) if mode == capi.HAND_EYE_CAMERA_ON_LINK else c
                    K_[f]["rvec"], K_[f]["tvec"] = so3_log(lk[0]), lk[1]
                return K_
            unit = np.array(cov, copy=True)
            unit["cov"][unit["status"] == 0] = np.eye(6)
            clean, spoiled = links(False), links(True)
            for label, c_, k_, loss in (("weighted", cov, clean, capi.TRACK_LOSS_NONE), ("W = I", unit, clean, capi.TRACK_LOSS_NONE),
                                        ("weighted, Cauchy", cov, clean, capi.LOSS_CAUCHY), ("W = I, Cauchy", unit, clean, capi.LOSS_CAUCHY),
                                        ("wrong links, no loss", cov, spoiled, capi.TRACK_LOSS_NONE),
                                        ("wrong links, Huber", cov, spoiled, capi.LOSS_HUBER), ("wrong links, Cauchy", cov, spoiled, capi.LOSS_CAUCHY)):
                out, fr = det.fit_hand_eye(one, rec, c_, n, k_, opts=capi.hand_eye_opts(mode=mode, loss=loss, max_iterations=50))
                o = out[0]
                e = acc.setdefault((mode, label), {"P_rot": [], "P_tr": [], "Q_rot": [], "Q_tr": [], "s2": [], "down": [], "down_wrong": [], "status": []})
                e["status"].append(int(o["status"]))
                if o["status"] != capi.HE_OK:
                    continue
                e["P_rot"].append(rot_deg(so3_exp(o["P"]["rvec"]), Pt[0]))
                e["P_tr"].append(float(np.linalg.norm(o["P"]["tvec"] - Pt[1])))
                e["Q_rot"].append(rot_deg(so3_exp(o["Q"]["rvec"]), Qt[0]))
                e["Q_tr"].append(float(np.linalg.norm(o["Q"]["tvec"] - Qt[1])))
                e["s2"].append(float(o["sigma2_hat"]))
                d = (fr["flags"][:, 0] & capi.HE_FLAG_DOWNWEIGHTED) != 0
                e["down"].append(int(d.sum()))
                e["down_wrong"].append(int((d & wrong).sum()))
    print(json.dumps({"frames": n, "slots": SLOTS, "used_frames_per_slot": seen, "wrong_links_per_slot": int(wrong.sum())}), flush=True)
    for r in raw:
        print(json.dumps({"raw_poses": r}), flush=True)
    rms = lambda v: round(float(np.sqrt(np.mean(np.square(v)))), 5) if len(v) else None  # noqa: E731
    for (mode, label), e in acc.items():
        print(json.dumps({"mode": int(mode), "variant": label, "status": e["status"], "P_rot_deg": rms(e["P_rot"]), "P_trans": rms(e["P_tr"]),
                          "Q_rot_deg": rms(e["Q_rot"]), "Q_trans": rms(e["Q_tr"]), "sigma2_hat": [round(v, 2) for v in e["s2"]],
                          "downweighted": e["down"], "of_them_wrong_links": e["down_wrong"]}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
