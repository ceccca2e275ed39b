"""bench.py --dump-outputs without a GPU: dump_outputs() on records built here.  Every field round-trips exactly, the files stay
within the 64 MB budget, and a list too large for it is sampled the same way on every run."""
import os
import sys

import numpy as np

from ctag_testlib import RESULT_DT, ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _records(n):
    rng = np.random.RandomState(7)
    res = np.zeros(n, RESULT_DT)
    res["status"] = rng.randint(-3, 1, n)
    res["n_markers"] = rng.randint(0, 5, n)
    res["flags"] = 0xFFFFFFF0
    res["markers"]["marker_id"] = rng.randint(0, 1 << 20, (n, 100))
    res["features"]["corners"] = rng.standard_normal((n, 100, 16)).astype(np.float32) * 1000
    return res


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_is_exact_and_whole_when_it_fits(tmp_path):
    res = _records(64)
    info = bench.dump_outputs(res, str(tmp_path))
    assert info["frames"] == 64 and _size(str(tmp_path)) <= bench.DUMP_BUDGET
    for f in os.listdir(tmp_path):
        assert np.load(os.path.join(tmp_path, f)).dtype in (np.float32, np.float64), f
    assert (np.load(os.path.join(tmp_path, "status.npy")) == res["status"]).all()
    assert (np.load(os.path.join(tmp_path, "flags.npy")) == res["flags"]).all()
    assert (np.load(os.path.join(tmp_path, "markers_marker_id.npy")) == res["markers"]["marker_id"]).all()
    assert np.load(os.path.join(tmp_path, "features_corners.npy")).tobytes() == res["features"]["corners"].tobytes()


def test_large_lists_are_a_fixed_sample_within_the_budget(tmp_path):
    res = _records(8192)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(res, a)
    bench.dump_outputs(res, b)
    assert _size(a) <= bench.DUMP_BUDGET
    idx = np.load(os.path.join(a, "frame_index.npy"))
    assert 0 < len(idx) < 8192 and (np.diff(idx) > 0).all()
    assert (idx == np.load(os.path.join(b, "frame_index.npy"))).all()
    got = np.load(os.path.join(a, "features_corners.npy"))
    assert got.tobytes() == res["features"]["corners"][idx.astype(np.int64)].tobytes()
