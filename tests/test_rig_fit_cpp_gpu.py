"""GPU test of the rig assembly of the C++ class (CylinderTag::assembleRigModel) through cylindertag_amd/examples/ctag_rigcheck.cpp:
on batch (a) of tests/rig_fit_shapes.py the class returns what the C call returns, float for float."""
import os
import subprocess

import numpy as np
import pytest

import cylindertag_amd as ca
import rig_fit_shapes as sh
from ctag_testlib import GOLDEN, ROOT
from rig_fit_testlib import Detectors, input_of

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_rigcheck")


def _camera_file(path, K):
    """The pinhole camera of batch (a) as the OpenCV YAML loadCamera reads; five zero coefficients."""
    k = ", ".join("%.9g" % v for v in np.asarray(K, np.float32).ravel())
    with open(path, "w") as f:
        f.write("%%YAML:1.0\n---\n\ncameraMatrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: f\n   data: [ %s ]\n" % k)
        f.write("distCoeffs: !!opencv-matrix\n   rows: 5\n   cols: 1\n   dt: f\n   data: [ 0., 0., 0., 0., 0. ]\n")


def test_assemble_rig_model_of_the_class_equals_the_c_call(tmp_path):
    b = sh.batch(sh.NAMES[0])
    M, rigs = input_of(b)
    M.save(str(tmp_path / "in.model"))
    np.ascontiguousarray(b["recs"]).tofile(str(tmp_path / "records.bin"))
    _camera_file(str(tmp_path / "camera.yml"), b["K"])
    cam = ca.load_camera(str(tmp_path / "camera.yml"))
    assert np.asarray(cam.K[:], np.float32).tobytes() == np.asarray(b["K"], np.float32).ravel().tobytes() and not any(cam.dist[:])
    # the class's handle has the 12 columns of the shipped dictionary, as batch (a)'s models have
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), str(tmp_path / "records.bin"), str(tmp_path / "in.model"), str(tmp_path / "camera.yml"),
                        str(tmp_path / "out.model")] + [str(int(g)) for g in b["rig_of_model"]], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    dets = Detectors()
    try:
        R, rig_stats, model_stats, placed = dets.of(b).fit_rigs(b["recs"], M, rigs, cam)   # the defaults, as the class calls it
    finally:
        dets.close()
    assert "frames %d models %d placed %s\n" % (len(b["recs"]), len(placed), " ".join(str(int(g)) for g in placed)) in p.stdout
    assert p.stdout.count("threw assembleRigModel: assembleRigModel, no frames") == 1
    assert p.stdout.count("threw assembleRigModel: assembleRigModel, one rig entry per model") == 1
    got, want = ca.Model(str(tmp_path / "out.model")).view(), R.view()
    assert all(got[k].tobytes() == want[k].tobytes() for k in ("ids", "base", "axis", "corners"))
    assert got["corners"][1].tobytes() != b["model"]["corners"][1].tobytes() and rig_stats[0]["rounds"] >= 1
