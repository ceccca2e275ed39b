"""Model reconstruction end to end, with the detector in the loop (needs a GPU).

The ray-cast frames of tools/dense_study.py (cylinders of known radius with planted poses, 1920x1080, f = 2600 px) go through
detect().  The seed is cylindertag_amd.models.cylinder_model with every radius off by --radius-error (15 %): what a user who
wraps a printed strip round a tube and guesses its radius has.  Detector.fit_model reconstructs the models from the detections.
Reported: the 3-D position error of the markers' corners in the camera frame (mm; RMS over a marker, median / 90th percentile
over the markers), which does not depend on the model's own frame, with the seed, with the fitted model and with the true
model; the rounds taken; and the milliseconds per round of each kernel kind (CTAG_OPT_TIMING).

    python tools/model_fit_study.py --frames 96
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import cylindertag_amd as ca  # noqa: E402
import dense_testlib as dt  # noqa: E402
import testkit as tk  # noqa: E402
from cylindertag_amd import capi, models  # noqa: E402
from pose_statement import rodrigues  # noqa: E402

STRIP = 60.0  # the synthetic strips' height, mm


def corner_errors(det, recs, truths, model, corners, true_corners, cam):
    """Per posed marker: RMS distance, mm, between its corners placed by the estimated pose of `model` and by the planted pose of
    the true model, over the corners of the features the marker shows."""
    out = []
    for res, truth in zip(recs, truths):
        if res["status"] != 0:
            continue
        for p in det.estimate_pose(res, model, cam):
            ks = [i for i in range(truth["n_markers"]) if truth["dict_row"][i] == p["model_index"]] if p["status"] == 0 else []
            if not ks:
                continue
            M = res["markers"][p["marker"]]
            cols = sorted({int(res["features"][M["first_feature"] + j]["pos"]) for j in range(M["n_features"])})
            idx = np.concatenate([np.arange(8 * c, 8 * c + 8) for c in cols if 0 <= c < corners.shape[1] // 8])
            got = corners[p["model_index"]][idx].astype(np.float64) @ rodrigues(p["rvec"]).T + p["tvec"]
            want = true_corners[p["model_index"]][idx].astype(np.float64) @ truth["R"][ks[0]].reshape(3, 3).T + truth["t"][ks[0]]
            out.append(float(np.sqrt(((got - want) ** 2).sum(1).mean())))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--radius-error", type=float, default=0.15)
    a = ap.parse_args()
    state, fs, true_model, K = dt.synth_scene()
    det = ca.Detector(state, fs, device=0)
    det.set_option(capi.OPT_TIMING, 1)
    cam = ca.make_camera(K, np.zeros(5, np.float32))
    t0 = time.time()
    frames, truths = zip(*[tk.synth3d_frame_host(state, f, dt.K_PLANTED, rows=dt.ROWS, cols=dt.COLS) for f in range(a.frames)])
    recs = det.detect_batch(np.stack(frames), 5, True, 5)
    t_detect = time.time() - t0
    radii = np.array([models.default_radius(r, state.shape[1]) for r in range(state.shape[0])])
    sign = np.where(np.arange(len(radii)) % 2 == 0, 1.0 + a.radius_error, 1.0 - a.radius_error)
    seed_corners = models.cylinder_model(state, STRIP, radii * sign)
    ids = np.arange(state.shape[0], dtype=np.int32)
    seed = ca.Model(ids=ids, corners=seed_corners, model_size=state.shape[1])
    true = ca.Model(ids=ids, corners=true_model["corners"], model_size=state.shape[1])
    t0 = time.time()
    fitted, stats = det.fit_model(recs, seed, cam, ca.model_fit_opts(strip_height=STRIP))
    t_fit = time.time() - t0
    ms_kind = det.model_fit_last_ms()
    seen = stats["status"] == 0
    fit_corners = fitted.view()["corners"]
    keep_rows = set(np.nonzero(seen)[0].tolist())

    def summary(model, corners):
        e = corner_errors(det, recs, truths, model, corners, true_model["corners"], cam)
        return {"markers": int(len(e)), "median_mm": round(float(np.median(e)), 4), "p90_mm": round(float(np.percentile(e, 90)), 4)} if len(e) else {}

    rounds = stats["rounds"][seen]
    total_rounds = max(int(rounds.max()), 1) if len(rounds) else 1
    print(json.dumps({
        "frames": a.frames, "frames_ok": int((recs["status"] == 0).sum()), "radius_error": a.radius_error,
        "models_fitted": len(keep_rows), "records": int(stats["n_records"].sum()),
        "rounds": {"min": int(rounds.min()), "median": float(np.median(rounds)), "max": int(rounds.max())} if len(rounds) else {},
        "rms_px_fitted_median": round(float(np.median(stats["rms_px"][seen])), 4) if seen.any() else None,
        "corner_error_camera_frame": {"seed": summary(seed, seed_corners), "fitted": summary(fitted, fit_corners), "true": summary(true, true_model["corners"])},
        "ms_per_round": {k: round(v / total_rounds, 3) for k, v in ms_kind.items()}, "ms_total": {k: round(v, 2) for k, v in ms_kind.items()},
        "seconds": {"render_and_detect": round(t_detect, 1), "fit": round(t_fit, 2)}}))
    det.close()


if __name__ == "__main__":
    main()
