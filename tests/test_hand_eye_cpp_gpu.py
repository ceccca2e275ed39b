"""GPU test of hand-eye calibration through the C++ class (CylinderTag::calibrateHandEye) via
cylindertag_amd/examples/ctag_handeyecheck.cpp: from the per-frame rig poses and covariances the class's own calls return and a link pose
per frame, the class gives the records of the C call, byte for byte, and throws what it must."""
import os
import subprocess

import numpy as np
import pytest

import hand_eye_shapes as sh
from cylindertag_amd import capi
from ctag_testlib import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_handeyecheck")


@pytest.mark.parametrize("name", ("holes", "huber"))
def test_calibrate_hand_eye_of_the_class_equals_the_c_call(detector, tmp_path, name):
    b = sh.batch(name)   # `holes` has rigs missing from frames and dropped links, `huber` a loss
    nf, nr = b["n_frames"], b["n_rigs"]
    present = b["pose_status"] == 0
    item = np.zeros((nf, nr, 44))
    item[..., 0], item[..., 1] = present, b["cov_status"]
    item[..., 2:5], item[..., 5:8], item[..., 8:] = b["rvec"], b["tvec"], b["cov"].reshape(nf, nr, 36)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([nf, nr, 0, 0], np.int32).tobytes())
        f.write(np.concatenate([b["links_rvec"], b["links_tvec"]], 1).astype(np.float64).tobytes())
        f.write(item.tobytes())
    with open(tmp_path / "opts.bin", "wb") as f:
        f.write(bytes(sh.he_opts(b)))
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), str(tmp_path / "in.bin"), str(tmp_path / "opts.bin"), str(tmp_path / "out.bin"),
                        str(tmp_path / "frames.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "frames %d rigs %d\n" % (nf, nr) in p.stdout
    assert p.stdout.count("threw calibrateHandEye, no frames") == 1 and p.stdout.count("threw calibrateHandEye, one link pose per frame") == 1
    assert p.stdout.count("threw calibrateHandEye, ") == 3 and "no throw" not in p.stdout
    got = np.fromfile(str(tmp_path / "out.bin"), capi.HAND_EYE_DT)
    gfr = np.fromfile(str(tmp_path / "frames.bin"), capi.HAND_EYE_FRAME_DT).reshape(nf, nr)
    # the C call on the records the class builds: a rig missing from a frame's list is CTAG_POSE_NOT_SEEN with CTAG_COV_NO_POSE
    c = dict(b, cov_status=np.where(present, b["cov_status"], 1).astype(np.int32), pose_status=np.where(present, 0, 5).astype(np.int32))
    want, wfr = sh.device_fit(detector, c)
    assert got.tobytes() == want.tobytes() and gfr.tobytes() == wfr.tobytes()
    assert (got["status"] == capi.HE_OK).all() and (gfr["flags"] & capi.HE_FLAG_USED).any()
