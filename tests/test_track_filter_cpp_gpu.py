"""GPU test of live track filtering through the C++ class (CylinderTag::startRigTracking / trackRigs / predictRigs) via
cylindertag_amd/examples/ctag_trackfiltercheck.cpp: from the per-frame rig poses and covariances the class's own calls return, the class
gives the records of the C calls, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import track_filter_shapes as fsh
import track_filter_statement as fs
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_trackfiltercheck")


@pytest.mark.parametrize("name", ("gaps", "gate"))
def test_track_rigs_of_the_class_equals_the_c_calls(detector, tmp_path, name):
    b = fsh.batch(name)   # `gaps` has its own times, `gate` a gate and f * dt
    nf, nr = b["n_frames"], b["n_rigs"]
    present = b["pose_status"] == 0
    item = np.zeros((nf, nr, 44))
    item[..., 0], item[..., 1] = present, b["cov_status"]
    item[..., 2:5], item[..., 5:8], item[..., 8:] = b["rvec"], b["tvec"], b["cov"].reshape(nf, nr, 36)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([nf, nr, b["times"] is not None, 0], np.int32).tobytes())
        if b["times"] is not None:
            f.write(np.asarray(b["times"], np.float64).tobytes())
        f.write(item.tobytes())
    with open(tmp_path / "opts.bin", "wb") as f:
        f.write(bytes(fsh.filter_opts(b)))
    t_pred = (b["times"][-1] if b["times"] is not None else (nf - 1) * fs.filter_opts(b)["dt"]) + 0.01
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), str(tmp_path / "in.bin"), str(tmp_path / "opts.bin"), str(tmp_path / "out.bin"),
                        "%.17g" % t_pred, str(tmp_path / "pred.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "frames %d rigs %d\n" % (nf, nr) in p.stdout
    assert p.stdout.count("threw trackRigs, startRigTracking first") == 1 and p.stdout.count("threw trackRigs, ") == 2 and "no throw" not in p.stdout
    got = np.fromfile(str(tmp_path / "out.bin"), capi.TRACK_DT).reshape(nf, nr)
    pred = np.fromfile(str(tmp_path / "pred.bin"), capi.TRACK_DT)
    # the C calls on the records the class builds: a rig missing from a frame's list is CTAG_POSE_NOT_SEEN with CTAG_COV_NO_POSE
    c = dict(b, cov_status=np.where(present, b["cov_status"], 1).astype(np.int32), pose_status=np.where(present, 0, 5).astype(np.int32))
    with fsh.DeviceFilter(detector, c) as F:
        want = np.concatenate([F.run(fs.frames_slice(c, k, k + 1), times=None if b["times"] is None else b["times"][k:k + 1]) for k in range(nf)])
        want_pred = F.f.predict(t_pred)
    assert got.tobytes() == want.tobytes() and pred.tobytes() == want_pred.tobytes()
    assert (got["status"] == capi.TRACK_OK).any() and (got["flags"] & capi.TRACK_FLAG_STARTED).any()
    if name == "gate":
        assert (got["flags"] & capi.TRACK_FLAG_GATED).any()
