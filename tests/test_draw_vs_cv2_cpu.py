"""The sequential painter of tests/draw_testlib.py against real OpenCV, where cv2 imports: cv2.circle, cv2.arrowedLine and
cv2.projectPoints on random inputs must give exactly the painter's bytes / floats.  Skipped without cv2; a failure on a
host that has it is a finding about the painter (and hence the kernels), not a reason to loosen the bar."""
import numpy as np
import pytest

import draw_testlib as D

cv2 = pytest.importorskip("cv2")


def test_circles_equal_cv2():
    rng = np.random.default_rng(1)
    for _ in range(200):
        h, w = int(rng.integers(20, 120)), int(rng.integers(20, 120))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        c = (int(rng.integers(-15, w + 15)), int(rng.integers(-15, h + 15)))
        r = int(rng.choice([5, 8]))
        col = tuple(int(v) for v in rng.integers(0, 256, 3))
        want = cv2.circle(img.copy(), c, r, col, -1)
        got = img.copy()
        D.circle_filled(got, c, r, col)
        assert np.array_equal(got, want), (c, r)


def test_arrowed_lines_equal_cv2():
    rng = np.random.default_rng(2)
    for _ in range(300):
        h, w = int(rng.integers(30, 200)), int(rng.integers(30, 200))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p1 = (int(rng.integers(-60, w + 60)), int(rng.integers(-60, h + 60)))
        p2 = (int(rng.integers(-60, w + 60)), int(rng.integers(-60, h + 60)))
        col = tuple(int(v) for v in rng.integers(0, 256, 3))
        want = cv2.arrowedLine(img.copy(), p1, p2, col, 10, cv2.LINE_AA, 0, 0.2)
        got = img.copy()
        D.arrowed_line(got, p1, p2, col)
        assert np.array_equal(got, want), (p1, p2, (h, w))


@pytest.mark.parametrize("n_dist", [0, 4, 5, 8, 12, 14])
def test_project_points_equal_cv2(n_dist):
    rng = np.random.default_rng(n_dist)
    K = np.array([[1200, 0, 640], [0, 1150, 360], [0, 0, 1]], np.float32)
    d = np.concatenate([rng.normal(0, 0.1, 5), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 4), [0, 0]]).astype(np.float32)[:n_dist]
    for _ in range(20):
        X = rng.normal(0, 20, (40, 3)).astype(np.float32)
        rv, tv = rng.normal(0, 0.4, 3), np.array([0, 0, 300.0]) + rng.normal(0, 20, 3)
        want, _ = cv2.projectPoints(X, rv.reshape(3, 1), tv.reshape(3, 1), K, d if n_dist else None)
        got = D.project_points(X, rv, tv, K, d)
        assert np.array_equal(got, want.reshape(-1, 2).astype(np.float32))
