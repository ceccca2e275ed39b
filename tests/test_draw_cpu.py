"""CPU tests of the drawAxis overlay: the sequential painter of tests/draw_testlib.py on hand-checked cases, its 14-term
projection against the closed form, the new C ABI symbols, and the host entry points failing loudly without a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cylindertag_amd as ca
import draw_testlib as D
from cylindertag_amd import capi
from ctag_testlib import ROOT
from pose_testlib import rodrigues

RED = (255, 0, 0)


def blank(h=40, w=40):
    return np.zeros((h, w, 3), np.uint8)


def test_disk_radius_5_and_8_shapes():
    """Circle(fill) of the midpoint loop: half widths 5,4,4,4,3,0 (radius 5) and 8,7,7,7,6,6,5,3,0 (radius 8), centred."""
    for r, hw in ((5, [5, 4, 4, 4, 3, 0]), (8, [8, 7, 7, 7, 6, 6, 5, 3, 0])):
        img = blank()
        D.circle_filled(img, (20, 20), r, RED)
        m = img[:, :, 0] > 0
        for oy in range(-r, r + 1):
            row = np.nonzero(m[20 + oy])[0]
            h = hw[abs(oy)]
            assert list(row) == list(range(20 - h, 21 + h)), (r, oy)
        assert m.sum() == sum(2 * hw[abs(o)] + 1 for o in range(-r, r + 1))
        assert (img[m] == RED).all()


def test_disk_clipping_at_all_four_borders():
    ref = blank()
    D.circle_filled(ref, (20, 20), 5, RED)
    for (cx, cy) in ((1, 20), (38, 20), (20, 0), (20, 39), (-3, -3), (42, 41)):
        img = blank()
        D.circle_filled(img, (cx, cy), 5, RED)
        big = np.zeros((80, 80, 3), np.uint8)
        D.circle_filled(big, (cx + 20, cy + 20), 5, RED)
        assert np.array_equal(img, big[20:60, 20:60]), (cx, cy)
    img = blank()
    D.circle_filled(img, (60, 60), 5, RED)  # entirely outside
    assert not img.any()


def test_horizontal_thick_aa_line():
    """line(p0, p1, 10, LINE_AA) horizontal: a solid body 11 rows high between the caps, symmetric about its centre row,
    with anti-aliased (partial) pixels only on the rim; the rows far from the line untouched."""
    img = blank(40, 80)
    D.thick_line(img, (20, 20), (60, 20), RED)
    a = img[:, :, 0].astype(int)
    assert (a[15:26, 25:56] == 255).all()  # the polygon's interior
    assert not a[:12].any() and not a[29:].any()
    col = a[:, 40]
    assert np.array_equal(col[15:26], np.full(11, 255))
    assert ((col > 0) & (col < 255)).any()  # anti-aliased rim
    assert (img[:, :, 1] == 0).all() and (img[:, :, 2] == 0).all()
    # the round caps: nothing beyond 5 px (+ the 1 px AA rim) from the end points
    assert not a[:, :13].any() and not a[:, 68:].any()
    assert (a[20, 15:66] == 255).all()


def test_diagonal_thick_aa_line():
    img = blank(80, 80)
    D.thick_line(img, (20, 20), (60, 60), RED)
    a = img[:, :, 0].astype(int)
    # full coverage along the diagonal, nothing farther than 5 px + the AA rim from the segment
    assert all(a[t, t] == 255 for t in range(17, 64)) and a[16, 16] < 255 and not a[15, 15]
    ys, xs = np.nonzero(a)
    t = np.clip((xs + ys) / 2.0, 20, 60)
    assert (np.hypot(xs - t, ys - t) <= 7.0).all()
    assert ((a > 0) & (a < 255)).any()  # anti-aliased rim


def test_arrow_tip_points():
    """arrowedLine's tip: 0.2 * |p1 - p2| from p2 at +-45 degrees off the reversed direction, cvRound'ed."""
    assert D.arrow_tips((0, 0), (100, 0)) == [(86, -14), (86, 14)]  # tip 20 px: 14.14 px back and to each side
    assert D.arrow_tips((100, 0), (0, 0)) == [(14, 14), (14, -14)]
    assert D.arrow_tips((0, 0), (0, 50)) == [(7, 43), (-7, 43)]     # tip 10 px: 7.07
    assert D.arrow_tips((5, 5), (5, 5)) == [(5, 5), (5, 5)]
    q = D.arrow_tips((3, 4), (33, 44))
    L = 0.2 * 50
    ang = math.atan2(-40, -30)
    assert q[0] == (round(33 + L * math.cos(ang + math.pi / 4)), round(44 + L * math.sin(ang + math.pi / 4)))


def test_last_corner_is_not_drawn():
    """The reference's size()-5 bound: of 8 corners + base + 3 axis ends, corners 0..6 get a disk, corner 7 does not."""
    img = np.zeros((200, 400, 3), np.uint8)
    pts = [(20 + 40 * k, 30) for k in range(8)] + [(200, 150), (230, 150), (200, 120), (170, 150)]
    D.draw_marker(img, np.array(pts, np.float32))
    for k in range(7):
        assert tuple(img[30, 20 + 40 * k]) == D.CORNER_COLOR, k
    assert not img[30, 300].any()
    assert tuple(img[150, 200]) == D.BASE_COLOR


def test_non_finite_point_removes_its_primitives():
    img = np.zeros((200, 400, 3), np.uint8)
    pts = np.array([(20 + 40 * k, 30) for k in range(8)] + [(200, 150), (230, 150), (200, 120), (170, 150)], np.float32)
    pts[2, 0] = np.nan
    pts[9, 1] = np.inf  # the first axis end
    D.draw_marker(img, pts)
    assert not img[30, 100].any()
    assert not ((img[:, :, 0] > 0) & (img[:, :, 1] == 0) & (img[:, :, 2] == 0)).any()  # the red (255,0,0) axis is gone
    assert (img[:, :, 1] == 255).any() and (img[:, :, 2] == 255).any()
    img2 = np.zeros((200, 400, 3), np.uint8)
    pts[8, 0] = np.inf  # the base: no axes, no base disk
    D.draw_marker(img2, pts)
    assert not img2[100:200].any()


def closed_form(X, rvec, tvec, K, d):
    """The textbook model (Brown-Conrady + rational + thin prism) evaluated with numpy in whole-array form."""
    R = rodrigues(rvec)
    P = np.asarray(X, np.float64) @ R.T + np.asarray(tvec, np.float64)
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    k = np.zeros(12)
    k[:len(d)] = np.asarray(d, np.float64)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = k
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
    K = np.asarray(K, np.float64)
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1)


@pytest.mark.parametrize("n_dist", [0, 4, 5, 8, 12, 14])
def test_projection_14_terms_against_closed_form(n_dist):
    rng = np.random.default_rng(n_dist)
    K = np.array([[1200, 0, 640], [0, 1150, 360], [0, 0, 1]], np.float32)
    d = np.concatenate([rng.normal(0, 0.1, 5), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 4)]).astype(np.float32)[:n_dist]
    for _ in range(5):
        X = rng.normal(0, 20, (30, 3)).astype(np.float32)
        rv, tv = rng.normal(0, 0.4, 3), np.array([0, 0, 300.0]) + rng.normal(0, 20, 3)
        got = D.project_points(X, rv, tv, K, d)
        want = closed_form(X, rv, tv, K, d)
        assert got.dtype == np.float32
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()) + 1e-3


def test_overlay_symbols_exported_and_prototyped():
    hdr = open(os.path.join(ROOT, "include", "ctag_pose.h")).read()
    for s in ("ctag_draw_axis", "ctag_draw_axis_batch_device"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.POSE_EXPORTS and s in capi.EXPORTS
        L = capi.load_library()
        assert getattr(L, s).restype == C.c_int and getattr(L, s).argtypes
    assert len(capi.load_library().ctag_draw_axis.argtypes) == 13
    assert len(capi.load_library().ctag_draw_axis_batch_device.argtypes) == 17
    assert capi.load_library().ctag_version() >= 120
    assert hasattr(ca.Detector, "draw_axis") and hasattr(ca.Detector, "draw_axis_batch_device")


def test_host_entry_points_fail_loudly_without_gpu():
    """No handle can be created without a device, and the overlay entry points refuse a null handle / bad arguments with
    CTAG_ERR_ARG instead of drawing on the CPU."""
    L = capi.load_library()
    g = np.zeros((8, 8), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    res = np.zeros(1, ca.RESULT_DT)
    cam = capi.CameraC()
    assert L.ctag_draw_axis(None, g.ctypes.data, 8, 8, 8, res.ctypes.data, None, 0, None, C.byref(cam), 5, out.ctypes.data, 24) == -1
    assert L.ctag_draw_axis_batch_device(None, None, 1, 8, 8, 8, 64, None, None, None, 0, None, C.byref(cam), 5, None, 24, 192) == -1
    import testkit as tk
    state, fs = ca.load_marker_file(os.path.join(ROOT, "tests", "golden", "CTag_2f12c.marker"))
    if not _has_gpu():
        with pytest.raises(ca.CtagError):
            tk.Detector(state, fs, device=0)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False
