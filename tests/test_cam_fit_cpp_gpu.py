"""GPU test of the camera set fit of the C++ class (CylinderTag::calibrateCameraSet) through cylindertag_amd/examples/ctag_camsetcheck.cpp:
on case (a) of tests/cam_fit_shapes.py the class returns what the C call returns, double for double."""
import os
import subprocess

import numpy as np
import pytest

import cam_fit_shapes as sh
import cylindertag_amd as ca
from cam_fit_testlib import Detectors, input_of
from ctag_testlib import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_camsetcheck")


def _camera_file(path, K, dist):
    """A camera as the OpenCV YAML loadCamera reads."""
    k = ", ".join("%.9g" % v for v in np.asarray(K, np.float32).ravel())
    d = [float(v) for v in np.asarray(dist, np.float32).ravel()] or [0.0] * 5
    with open(path, "w") as f:
        f.write("%%YAML:1.0\n---\n\ncameraMatrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: f\n   data: [ %s ]\n" % k)
        f.write("distCoeffs: !!opencv-matrix\n   rows: %d\n   cols: 1\n   dt: f\n   data: [ %s ]\n" % (len(d), ", ".join("%.9g" % v for v in d)))


def test_calibrate_camera_set_of_the_class_equals_the_c_call(tmp_path):
    b = sh.case("a 0.1 px")
    M, rigs, _ = input_of(b)
    M.save(str(tmp_path / "in.model"))
    np.ascontiguousarray(b["recs"]).tofile(str(tmp_path / "records.bin"))
    cams = []
    for c, (K, dist) in enumerate(b["cameras"]):
        _camera_file(str(tmp_path / ("camera%d.yml" % c)), K, dist)
        cams.append(ca.load_camera(str(tmp_path / ("camera%d.yml" % c))))
        assert np.asarray(cams[c].K[:], np.float32).tobytes() == np.asarray(K, np.float32).ravel().tobytes()
        assert np.asarray(cams[c].dist[:len(dist)], np.float32).tobytes() == np.asarray(dist, np.float32).tobytes()
    # the class's handle has the 12 columns of the shipped dictionary, as case (a)'s models have
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), str(tmp_path / "records.bin"), str(tmp_path / "in.model"), str(len(cams))] +
                       [str(tmp_path / ("camera%d.yml" % c)) for c in range(len(cams))] + [str(int(g)) for g in b["rig_of_model"]],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    dets = Detectors()
    try:
        cs, stat, cam_stats = dets.of(b).fit_camera_set(b["recs"], M, rigs, cams)   # the defaults, as the class calls it
    finally:
        dets.close()
    assert "cameras %d instants %d all 1\n" % (len(cams), b["recs"].shape[1]) in p.stdout and cs is not None and stat["rounds"] >= 1
    for c in range(len(cams)):
        line = next(ln for ln in p.stdout.splitlines() if ln.startswith("camera %d placed 1 pose " % c))
        got = np.array([float(v) for v in line.split()[5:]])
        assert got.tobytes() == np.concatenate([cam_stats[c]["rvec"], cam_stats[c]["tvec"]]).tobytes(), (c, got)
    assert cam_stats[1]["rvec"].any()
    assert p.stdout.count("threw calibrateCameraSet: calibrateCameraSet, 2 to 8 cameras") == 1
    assert p.stdout.count("threw calibrateCameraSet: calibrateCameraSet, one rig entry per model") == 1
