"""GPU test of the track noise fit through the C++ class (CylinderTag::calibrateTrackNoise and startRigTracking with the fitted values)
via cylindertag_amd/examples/ctag_tracknoisecheck.cpp: from the per-frame rig poses and covariances the class's own calls return, the
class gives the records of the C calls, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import track_filter_shapes as fsh
import track_filter_statement as fs
import track_noise_shapes as nsh
import track_noise_statement as ns
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_tracknoisecheck")


@pytest.mark.parametrize("name,mode", (("planted_times", ns.PER_RIG), ("gaps", ns.POOLED)))
def test_calibrate_track_noise_of_the_class_equals_the_c_calls(detector, tmp_path, name, mode):
    b = nsh.batch(name)
    nf, nr = b["n_frames"], b["n_rigs"]
    over = dict(free_mask=5, rounds=3, mode=mode)
    present = b["pose_status"] == 0
    item = np.zeros((nf, nr, 44))
    item[..., 0], item[..., 1] = present, b["cov_status"]
    item[..., 2:5], item[..., 5:8], item[..., 8:] = b["rvec"], b["tvec"], b["cov"].reshape(nf, nr, 36)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([nf, nr, b["times"] is not None, 0], np.int32).tobytes())
        if b["times"] is not None:
            f.write(np.asarray(b["times"], np.float64).tobytes())
        f.write(item.tobytes())
    fopts = capi.track_filter_opts(gate=6.0, max_gap=ns.noise_opts(b)["max_gap"])
    with open(tmp_path / "nopts.bin", "wb") as f:
        f.write(bytes(nsh.noise_opts_c(b, **over)))
    with open(tmp_path / "fopts.bin", "wb") as f:
        f.write(bytes(fopts))
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), str(tmp_path / "in.bin"), str(tmp_path / "nopts.bin"), str(tmp_path / "fopts.bin"),
                        str(tmp_path / "noise.bin"), str(tmp_path / "track.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    n_search = 1 if mode == ns.POOLED else nr
    assert "frames %d rigs %d searches %d\n" % (nf, nr, n_search) in p.stdout
    assert p.stdout.count("threw calibrateTrackNoise, ") == 1 and "no throw" not in p.stdout
    got = np.fromfile(str(tmp_path / "noise.bin"), capi.TRACK_NOISE_DT)
    track = np.fromfile(str(tmp_path / "track.bin"), capi.TRACK_DT).reshape(nf, nr)
    # the C calls on the records the class builds: a rig missing from a frame's list is CTAG_POSE_NOT_SEEN with CTAG_COV_NO_POSE
    c = dict(b, cov_status=np.where(present, b["cov_status"], 1).astype(np.int32), pose_status=np.where(present, 0, 5).astype(np.int32))
    want = nsh.device_fit(detector, c, trace=False, **over)
    assert got.tobytes() == want.tobytes() and (want["status"] == capi.NOISE_OK).all()
    o, s = capi.apply_track_noise(want[:1], gate=6.0, max_gap=ns.noise_opts(b)["max_gap"])
    F = detector.track_filter(fsh.sh.RigSet(nr), o)
    try:
        F.set_cov_scale(s)
        wt = np.concatenate([F.step(*fsh.sh.to_records(fs.frames_slice(c, k, k + 1)), 1, times=None if b["times"] is None else b["times"][k:k + 1])
                             for k in range(nf)])
    finally:
        F.close()
    wt["frame"] = 0   # the class gives one frame a call
    assert track.tobytes() == wt.tobytes() and (track["status"] == capi.TRACK_OK).any()
