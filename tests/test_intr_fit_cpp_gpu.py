"""GPU test of the intrinsics fit of the C++ class (CylinderTag::calibrateCamera) through cylindertag_amd/examples/ctag_intrinsicscheck.cpp:
on case (a) of tests/intr_fit_shapes.py the class returns what the C call returns, float for float and double for double."""
import os
import subprocess

import numpy as np
import pytest

import cylindertag_amd as ca
import intr_fit_shapes as sh
from ctag_testlib import ROOT
from intr_fit_testlib import Detectors, input_of

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_intrinsicscheck")


def _camera_file(path, K, dist):
    """A camera as the OpenCV YAML loadCamera reads."""
    k = ", ".join("%.9g" % v for v in np.asarray(K, np.float32).ravel())
    d = [float(v) for v in np.asarray(dist, np.float32).ravel()] or [0.0] * 5
    with open(path, "w") as f:
        f.write("%%YAML:1.0\n---\n\ncameraMatrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: f\n   data: [ %s ]\n" % k)
        f.write("distCoeffs: !!opencv-matrix\n   rows: %d\n   cols: 1\n   dt: f\n   data: [ %s ]\n" % (len(d), ", ".join("%.9g" % v for v in d)))


def test_calibrate_camera_of_the_class_equals_the_c_call(tmp_path):
    c = sh.case("a 0.1 px")
    M, rigs, _ = input_of(c)
    M.save(str(tmp_path / "in.model"))
    np.ascontiguousarray(c["recs"]).tofile(str(tmp_path / "records.bin"))
    _camera_file(str(tmp_path / "seed.yml"), *c["seed"])          # five zero coefficients: the file format has no empty list
    seed = ca.load_camera(str(tmp_path / "seed.yml"))
    assert np.asarray(seed.K[:], np.float32).tobytes() == np.asarray(c["seed"][0], np.float32).ravel().tobytes() and seed.n_dist == 5
    with open(str(tmp_path / "dict.marker"), "w") as f:           # the class's handle needs the 20 columns of case (a)'s model
        f.write("%d %d 2\n" % c["state"].shape + "\n".join("\t".join(str(int(v)) for v in row) for row in c["state"]) + "\n")
    p = subprocess.run([EXE, str(tmp_path / "dict.marker"), str(tmp_path / "records.bin"), str(tmp_path / "in.model"), str(tmp_path / "seed.yml"), "0xF", "0"] +
                       [str(int(g)) for g in c["rig_of_model"]], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    dets = Detectors()
    try:
        cam, stat, _ = dets.of(c).fit_intrinsics(c["recs"], M, rigs, seed, free_mask=0xF)   # the defaults otherwise, as the class calls it
    finally:
        dets.close()
    lines = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln.split()}
    assert "views %d fitted 1\n" % len(c["recs"]) in p.stdout and stat["status"] == 0 and stat["rounds"] >= 1
    assert np.array([float(v) for v in lines["K"]], np.float32).tobytes() == np.asarray(cam.K[:], np.float32).tobytes()
    assert np.array([float(v) for v in lines["dist"]], np.float32).tobytes() == np.asarray(cam.dist[:5], np.float32).tobytes()
    assert np.array([float(v) for v in lines["sigma"]]).tobytes() == np.asarray(stat["sigma"], np.float64).tobytes()
    assert cam.K[0] != seed.K[0] and stat["sigma"][0] > 0
    assert p.stdout.count("threw calibrateCamera: calibrateCamera, one rig entry per model") == 1
