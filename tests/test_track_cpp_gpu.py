"""GPU test of track smoothing through the C++ class (CylinderTag::smoothRigTrack) via cylindertag_amd/examples/ctag_trackcheck.cpp: from
the per-frame rig poses and covariances the class's own calls return, the class gives the records of the C call, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import track_shapes as sh
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_trackcheck")


@pytest.mark.parametrize("name", ("gaps", "huber"))
def test_smooth_rig_track_of_the_class_equals_the_c_call(detector, tmp_path, name):
    b = sh.batch(name)   # `gaps` has its own times, `huber` a loss and f * dt
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
    opts = sh.track_opts(b)
    with open(tmp_path / "opts.bin", "wb") as f:
        f.write(bytes(opts))
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), str(tmp_path / "in.bin"), str(tmp_path / "opts.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "frames %d rigs %d\n" % (nf, nr) in p.stdout
    assert p.stdout.count("threw smoothRigTrack, no frames") == 1 and p.stdout.count("threw smoothRigTrack, one covariance list per frame") == 1
    assert p.stdout.count("threw smoothRigTrack, ") == 3 and "no throw" not in p.stdout
    got = np.fromfile(str(tmp_path / "out.bin"), capi.TRACK_DT).reshape(nf, nr)
    # the C call on the records the class builds: a rig missing from a frame's list is CTAG_POSE_NOT_SEEN with CTAG_COV_NO_POSE
    c = dict(b, cov_status=np.where(present, b["cov_status"], 1).astype(np.int32), pose_status=np.where(present, 0, 5).astype(np.int32))
    want, _ = sh.device_smooth(detector, c)
    assert got.tobytes() == want.tobytes()
    assert (got["status"] == capi.TRACK_OK).any() and (got["status"] == capi.TRACK_NOT_TRACKED).any()
