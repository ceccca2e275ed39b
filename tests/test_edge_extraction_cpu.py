"""Stage a4 (`edgeExtraction`, `corner_detector.cpp:125-463`) of the oracle against the independent statement in
`tests/edge_testlib.py`: the candidate list, every candidate's `has_quad` and `n_boundary` exactly, its corners within 1e-3 px in
the reference's types ("ref") and within 1e-2 px of float64 ("f64", plus the resolution of the reference's float32 line fits), on
test.bmp, the 64-frame sequence, the 8 golden synthetic frames, 16 random-shape frames and the frames of `tests/edge_shapes.py`.
No candidate may miss a bar against the oracle.  Between "f64" and "ref" a candidate may miss one only when one of its comparisons
lies within EXCUSE_MARGIN of its threshold; those are listed, at most F64_EXCUSE_SHARE of them (0.3 %: the regular pinch fields of
edge_shapes.py repeat a few float32 knife edges), and at most RESOLUTION_SHARE need the float32 fit resolution."""
import numpy as np
import pytest

import edge_shapes as es
import edge_testlib as et
from sequences import avi_substitute


def _frames(state, test_bmp):
    import testkit as tk
    yield "test.bmp", test_bmp
    for k, f in enumerate(avi_substitute(test_bmp)):
        yield "sequence %d" % k, f
    for f in range(8):  # the golden synthetic frames (tests/golden/make_golden.py)
        yield "synthetic %d" % f, tk.synth_frame_host(state, f)[0]
    for seed in range(16):  # the sizes of test_gpu_parity.test_random_shapes_fuzz
        rows, cols = ((720, 1152), (540, 960), (1080, 1920), (601, 1023))[seed % 4]
        yield "random shapes %d" % seed, et.random_shapes_frame(state, seed, rows, cols)
    for name, f, _ in es.shape_frames_tagged():
        yield "shapes " + name, f


@pytest.fixture(scope="module")
def statement_runs(oracle, dictionary, test_bmp):
    """Every frame through the oracle and the statement in both modes: {name: (oracle run, ref candidates, f64 candidates)}."""
    et.use_shared_math(oracle)
    state, fs = dictionary
    runs = {}
    for name, img in _frames(state, test_bmp):
        o = oracle.detect(img, state, fs)
        runs[name] = (o, et.extract_frame(o["labels"], "ref"), et.extract_frame(o["labels"], "f64"))
    return runs


def test_candidate_lists(statement_runs):
    """The candidates are the components of 30 .. round(0.01 rows cols) pixels in label order, with the oracle's areas and boxes."""
    for name, (o, ref, _) in statement_runs.items():
        oc = o["candidates"]
        assert [c.label for c in ref] == list(oc[:, 0]), name
        assert [c.area for c in ref] == list(oc[:, 1]), name
        assert [list(c.bbox) for c in ref] == oc[:, 2:6].tolist(), name


def test_edge_extraction_matches_independent_statement(statement_runs):
    tally = et.Tally()
    for name, (o, ref, f64) in statement_runs.items():
        oc = o["candidates"]
        tally.add(name, ref, f64, oc[:, 6], oc[:, 7], o["candidate_quads"])
    print("\nedgeExtraction, oracle vs statement: " + tally.report())
    tally.check()
    assert tally.compared >= 10000 and tally.compared - tally.with_quad >= 2000, tally.report()


def test_shape_frames_reach_their_topologies(statement_runs):
    """What tests/edge_shapes.py is for: every shape it draws for a topology (letters open to each side, rings, pinches, diagonal
    arms, symmetric shapes, triangles, pentagons, discs, rotated rectangles, wide bars, seams, frame edges and corners, the area
    limits) yields a candidate inside its box, the shapes past the area limits yield none, and between them the walk stops early,
    the loop runs out of points (isFailed) and the nearest-point sort meets ties."""
    shapes = {n[len("shapes "):]: v for n, v in statement_runs.items() if n.startswith("shapes ")}
    tagged = {name: tags for name, _, tags in es.shape_frames_tagged()}
    assert set(shapes) == set(es.FRAMES) == set(tagged)
    topologies = set()
    for name, (o, ref, _) in shapes.items():
        for tag, x0, y0, x1, y1 in tagged[name]:
            inside = [c for c in ref if x0 <= c.bbox[0] and y0 <= c.bbox[1] and c.bbox[2] <= x1 and c.bbox[3] <= y1]
            assert bool(inside) != (tag in es.ABSENT), (name, tag, (x0, y0, x1, y1))
            topologies.add(tag)
    assert {"U open right", "U open up", "U open left", "U open down", "C open right", "C open up", "C open left", "C open down",
            "E open right", "E open up", "E open left", "E open down", "ring", "pinch", "diagonal arm", "symmetric", "triangle",
            "pentagon", "disc", "small triangle", "rect 0", "rect 1", "rect 44.9", "rect 45", "rect 89", "bar", "edge top",
            "edge bottom", "edge left", "edge right", "corner top-left", "corner top-right", "corner bottom-left",
            "corner bottom-right", "seam x=0", "seam x=31", "seam x=32", "seam x=319", "seam x=320", "area 30", "area 29",
            "area limit", "area limit + 1", "pinch field"} <= topologies
    cands = [c for _, ref, _ in shapes.values() for c in ref]
    assert sum(c.n_boundary < c.n_ray_cast for c in cands) >= 10  # walks that stop before every boundary pixel
    assert sum(c.failed_short for c in cands) >= 10  # the RDP loop left with <= 2 points (isFailed)
    assert sum(not c.has_quad for c in cands) >= 50 and sum(c.has_quad for c in cands) >= 50
    ties = 0
    for c in cands:
        d = np.hypot(c.boundary[:, 0] - c.boundary[:, 0].mean(), c.boundary[:, 1] - c.boundary[:, 1].mean())
        ties += int(np.sum(np.isclose(d, d.min(), rtol=0, atol=1e-9)) > 1)
    assert ties >= 10
    areas = sorted(c.area for c in shapes["area_limits"][1])
    assert 30 in areas and es.AREA_LIMIT in areas and 29 not in areas and es.AREA_LIMIT + 1 not in areas
    xmins = {c.bbox[0] for c in shapes["seams_and_edges"][1]}
    assert {5, 31, 32, 319, 320} <= xmins  # (x = 0 lies in the background band: its boxes start at 5)
    assert max(c.bbox[2] - c.bbox[0] for c in shapes["rotations"][1]) > 128
