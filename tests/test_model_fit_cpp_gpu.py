"""GPU test of the model calls of the C++ class (CylinderTag::saveModel, CylinderTag::reconstructModel) through
cylindertag_amd/examples/ctag_modelcheck.cpp: the class needs a handle, so even the file round trip runs where a GPU is."""
import os
import re
import subprocess

import pytest

from ctag_testlib import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "cylindertag_amd", "_build", "ctag_modelcheck")


def test_save_model_and_reconstruct_model_of_the_class(tmp_path):
    p = subprocess.run([EXE, os.path.join(GOLDEN, "CTag_2f12c.marker"), os.path.join(GOLDEN, "test.bmp"), os.path.join(GOLDEN, "CTag_2f12c.model"),
                        os.path.join(GOLDEN, "cameraParams.yml"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, out + p.stderr
    assert "roundtrip same models 6" in out and "fitted roundtrip same" in out
    assert "threw saveModel: saveModel, could not write the model file" in out
    assert "threw reconstructModel: reconstructModel, no frames" in out
    assert "fitted models 6" in out
    rows = re.findall(r"model (\d+) id (-?\d+) seen (\d) finite (\d) moved (\S+)", out)
    assert len(rows) == 6 and all(r[3] == "1" for r in rows)
    seen = [r for r in rows if r[2] == "1"]
    assert len(seen) == 5   # test.bmp shows five of the six models
    for r in rows:
        if r[2] == "0":
            assert float(r[4]) == 0.0, "a model no frame shows must come back as the seed"
        else:
            assert float(r[4]) < 5.0   # mm: three identical records cannot say much, but nothing may run away from the seed's gauge
    # the file saveModel wrote is the text the C loader and the plain parser read alike
    from pose_testlib import read_model_file
    a, b = read_model_file(os.path.join(GOLDEN, "CTag_2f12c.model")), read_model_file(str(tmp_path / "copy.model"))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("ids", "base", "axis", "corners"))
