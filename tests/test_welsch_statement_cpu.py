"""The clusters of tests/welsch_shapes.py, qualified without a GPU: for every one of them the oracle's `ctago_fitline_welsch` against the
Python statement of fitLine2D (`edge_testlib.fitline_welsch`, "ref" mode, the shared exp32), the distance between the two lines over the
cluster's own extent at most `edge_testlib.SAME_LINE_PX`.  The only excuse is the one tests/test_edge_extraction_cpu.py applies: a comparison
of the statement's own (`.welsch_angle`, `.welsch_shift`, `.welsch_min`) within EXCUSE_MARGIN of its threshold.  No cluster of `size_edges` may be
excused, at most 1 % of any other batch.  The statement's trace then says which tier and which branch every cluster takes; the coverage the
kernels' test (tests/test_welsch_forms_gpu.py) relies on is asserted here.  Eight planted errors show what the comparison refuses."""
import inspect

import numpy as np
import pytest

import edge_testlib as et
import welsch_shapes as ws

EXCUSED_SHARE = 0.01


def line_distance(pts, a, b):
    """The largest distance between lines a and b (vx, vy, x0, y0) over the extent of the cluster along either of them."""
    p = np.asarray(pts, np.float64)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    worst = 0.0
    for u, v in ((a, b), (b, a)):
        t = (p[:, 0] - u[2]) * u[0] + (p[:, 1] - u[3]) * u[1]
        for s in (t.min(), t.max()):
            x, y = u[2] + u[0] * s, u[3] + u[1] * s
            d = abs(v[1] * (x - v[2]) - v[0] * (y - v[3]))
            worst = d if not d <= worst else worst  # (a NaN stays)
    return worst


def qualify(oracle, cluster, statement=et.fitline_welsch, pts=None):
    """One cluster through the oracle and a statement (the planted errors pass their own, or their own copy of the points)."""
    path, trace = et._Path("ref"), {}
    with np.errstate(all="ignore"):
        got = statement(np.asarray(cluster if pts is None else pts, np.int64), path, "fit", trace)
    want = oracle.fitline(cluster, True)
    return dict(n=len(cluster), want=want, got=np.asarray(got, np.float32), dist=line_distance(cluster, want, got), margin=path.margin, site=path.site,
                trace=trace)


def verdict(results, allow_excuses):
    """(accepted, text): the batch's acceptance rule over qualify() results in order."""
    missed = [(i, r) for i, r in enumerate(results) if not r["dist"] <= et.SAME_LINE_PX]
    unexcused = [(i, r) for i, r in missed if not r["margin"] < et.EXCUSE_MARGIN]
    allowed = int(EXCUSED_SHARE * len(results)) if allow_excuses else 0
    ok = not unexcused and len(missed) <= allowed
    first = (unexcused or missed or [(None, None)])[0]
    text = "%d clusters, %d beyond %.0e px (%d of them excused by a margin below %.0e, %d allowed)" % (
        len(results), len(missed), et.SAME_LINE_PX, len(missed) - len(unexcused), et.EXCUSE_MARGIN, allowed)
    if first[0] is not None:
        text += "; first: cluster %d of %d points, %.2e px, margin %.1e at %s" % (first[0], first[1]["n"], first[1]["dist"], first[1]["margin"], first[1]["site"])
    return ok, text, first[0]


def statement_indices(batch_name, frame):
    return ws.statement_sample(frame) if batch_name.startswith("sort_forms") else range(len(frame))


@pytest.fixture(scope="module")
def qualified(oracle):
    """{batch: [(frame name, {cluster index: qualify()})]}: every cluster once."""
    et.use_shared_math(oracle)
    out = {}
    for name, make in ws.BATCHES.items():
        out[name] = [(fname, {i: qualify(oracle, frame[i]) for i in statement_indices(name, frame)}) for fname, frame in make()["frames"]]
    return out


def _flat(qualified, name):
    return [r for _, per in qualified[name] for _, r in sorted(per.items())]


# ------------------------------------------------------------------------------------------------ the inputs are what they claim to be

def test_the_shapes_use_the_kernels_constants():
    """The library itself says at which sizes its kernels change form (ctag_testkit_welsch_limits) and which grid the plan gives k_welsch."""
    import testkit as tk
    lim, plan = tk.welsch_limits(), tk.chunk_plan(ws.HD[0], ws.HD[1], 32)
    found = {k: lim[k] for k in ws.K if k in lim}
    found.update(welsch_gx=plan["welsch_gx"], welsch_gs=plan["welsch_gs"], lat_rank_blocks=lim["kLatRankBlocks"], sort_top_bucket=lim["kLineSortBuckets"] - 1)
    assert found == ws.K


def test_batches_are_deterministic_and_in_range():
    for name, make in ws.BATCHES.items():
        b = make()
        make.cache_clear()
        again = make()
        assert [f[0] for f in b["frames"]] == [f[0] for f in again["frames"]]
        for (fname, f), (_, g) in zip(b["frames"], again["frames"]):
            assert len(f) == len(g) and all(np.array_equal(c, d) for c, d in zip(f, g)), (name, fname)
            for c in f:
                assert c.dtype == np.int32 and c.ndim == 2 and c.shape[1] == 2 and len(c) >= 2 and c.min() >= 0 and c.max() <= 65535, (name, fname)
            if name != "branch_batch":  # (the default geometry stays inside a 1080p / 4K frame)
                assert all(c[:, 0].max() < b["size"][1] and c[:, 1].max() < b["size"][0] for c in f), (name, fname)
        for call in b["calls"]:
            assert 1 <= len(call["frames"]) and (not call["latency"] or len(call["frames"]) <= ws.K["kLatencyFrames"])


def test_size_edges_has_every_tier_edge_in_every_position():
    b = ws.size_edges()
    frames = [f for _, f in b["frames"]]
    tail_frames = [frames[c["frames"][0]] for c in b["calls"] if c["tail"]]
    plain = [frames[i] for c in b["calls"] if not c["tail"] and not c["latency"] for i in c["frames"]]
    lat = [frames[i] for c in b["calls"] if c["latency"] for i in c["frames"]]
    for n in ws.SIZES:
        assert any(len(f) == 1 and len(f[0]) == n for f in plain), "%d alone" % n
        # (the other eleven are shorter wherever that means something: edges of at most kWShort points get a lane each, and 11 is the shortest edge a block takes)
        alone = 1 if n > ws.K["kWShort"] + 1 else 12
        assert any(len(f) == 12 and ws.longest(f) == n and sum(len(c) == n for c in f) <= alone for f in plain), "%d leading twelve" % n
        if ws.K["kWShort"] < n <= ws.K["kWPts"]:  # forced from float pairs to packed words
            assert any(len(f) == 12 and ws.K["kWPts"] < ws.longest(f) <= ws.K["kWPtsU"] and any(len(c) == n for c in f) and min(map(len, f)) > ws.K["kWShort"] for f in plain), n
        if ws.K["kWShort"] < n <= ws.K["kWPtsU"]:  # forced to global memory
            assert any(len(f) == 12 and ws.K["kWPtsU"] < ws.longest(f) < ws.K["kPickN2"] and any(len(c) == n for c in f) and min(map(len, f)) > ws.K["kWShort"] for f in plain), n
        assert any(len(f[-1]) == n for f in tail_frames), "%d at the end of the pool" % n
        if n <= ws.K["kLatPoints"]:
            assert any(len(f) == 1 and len(f[0]) == n for f in lat) and any(len(f) == 12 and ws.longest(f) == n for f in lat), "%d in the few-frame kernel" % n
    # the edges of every constant, both sides
    for k in ("kWShort", "kWCap", "kWPts", "kWPtsU", "kPickN", "kPickN2", "kLatPoints"):
        assert {ws.K[k], ws.K[k] + 1} <= set(ws.SIZES), k
    assert {ws.K["kLatChunk"] * q + d for q in (1, 2, 3, 4) for d in (-1, 0, 1)} - {ws.K["kLatPoints"] + 1} <= set(ws.SIZES) | {513}
    # the two frames the few-frame kernel must decline, in calls that also hold frames it takes
    assert any(ws.longest(f) == ws.K["kLatPoints"] + 1 for f in lat) and any(len(f) == ws.K["kLatLines"] + 1 and ws.longest(f) <= ws.K["kLatPoints"] for f in lat)
    assert all(ws.longest(f) <= ws.K["kLatPoints"] + 1 for f in lat)


def test_block_mix_loops_blocks_and_grids():
    b = ws.block_mix()
    frames = [f for _, f in b["frames"]]
    count = lambda f: (sum(len(c) > ws.K["kWShort"] for c in f), sum(len(c) <= ws.K["kWShort"] for c in f))
    seen_long, seen_short = set(), set()
    for call in b["calls"]:
        if call["latency"]:
            continue
        gx, gs = call["gx"] or ws.K["welsch_gx"], call["gs"] or ws.K["welsch_gs"]
        for i in call["frames"]:
            nl, ns = count(frames[i])
            seen_long.add((nl, (gx, gs) == (1, 1)))
            seen_short.add((ns, (gx, gs) == (1, 1)))
    for nl in (1, 11, 12, 13, 24, 25, 216, 217, 440):
        assert (nl, False) in seen_long and (nl, True) in seen_long, nl
    for ns in (0, 1, 255, 256, 257, 600):
        assert (ns, False) in seen_short and (ns, True) in seen_short, ns
    assert 216 == ws.K["welsch_gx"] * ws.K["kWE"] and 256 == ws.K["welsch_gs"] * ws.K["kWT"]  # the sizes at which a block starts to loop at the plan's grid
    assert any(len(c["frames"]) == 5 and not c["latency"] and any(not frames[i] for i in c["frames"][1:-1]) for c in b["calls"])
    assert any(count(f)[0] == 0 and count(f)[1] > 0 for f in frames) and any(count(f)[1] == 0 and count(f)[0] > 0 for f in frames)
    lat_sizes = {len(frames[i]) for c in b["calls"] if c["latency"] for i in c["frames"]}
    assert {511, 512, 513, 1024, 2047, 2048} <= lat_sizes and 4 * ws.K["lat_rank_blocks"] == ws.K["kLatLines"]
    assert all(ws.longest(frames[i]) <= ws.K["kLatPoints"] for c in b["calls"] if c["latency"] for i in c["frames"] if frames[i])


def test_sort_forms_reach_both_sorts():
    b, hd = ws.sort_forms(), ws.sort_forms_hd()
    sizes = [len(f) for _, f in b["frames"]]
    assert sizes == [ws.K["kLdsLines"] - 1, ws.K["kLdsLines"], ws.K["kLdsLines"] + 1, 20000] and [len(f) for _, f in hd["frames"]] == [ws.K["kLdsLines"]]
    for _, f in b["frames"] + hd["frames"]:
        n = np.array([len(c) for c in f])
        assert (n > ws.K["sort_top_bucket"]).sum() == 3 and ((n >= 12) & (n <= 300)).sum() >= 12 and (n <= 11).sum() == len(f) - 15
        assert n.sum() <= 262144  # either workspace's cluster pool
        sample = ws.statement_sample(f)
        assert len(sample) == 512 and set(np.nonzero(n > 11)[0]) <= set(sample)


# ------------------------------------------------------------------------------------------------ oracle against statement

@pytest.mark.parametrize("name", list(ws.BATCHES))
def test_oracle_and_statement_agree(qualified, oracle, name):
    results = _flat(qualified, name)
    ok, text, _ = verdict(results, allow_excuses=name != "size_edges")
    print("%s: %s" % (name, text))
    assert ok, "%s: %s" % (name, text)
    if name.startswith("sort_forms"):  # the oracle alone fits every cluster of these frames (the GPU test compares with all of them): no NaN, a unit direction
        for _, frame in ws.BATCHES[name]()["frames"]:
            lines = np.array([oracle.fitline(c, True) for c in frame])
            assert np.isfinite(lines).all() and np.abs(np.hypot(lines[:, 0], lines[:, 1]) - 1).max() < 1e-6


def test_the_oracle_alone_meets_the_excuse_conditions(qualified):
    """The seeds are chosen so that the batches meet the conditions with room: nothing is excused in size_edges, and what is excused elsewhere is listed."""
    for name in ws.BATCHES:
        results = _flat(qualified, name)
        missed = [r for r in results if not r["dist"] <= et.SAME_LINE_PX]
        print("%s: %d of %d clusters excused; largest distance %.2e px" % (name, len(missed), len(results), max(r["dist"] for r in results)))
        assert len(missed) <= (0 if name == "size_edges" else int(EXCUSED_SHARE * len(results)))
        assert all(np.isfinite(r["want"]).all() for r in results)


# ------------------------------------------------------------------------------------------------ coverage from the trace

def _past2(r):
    return int((r["trace"]["iters"] >= 3).sum())


def _block_counts(per, frame):
    """Per kernel block of the frame: (edges, restarts that go on past the regroup at iteration 2, the four waves' counts)."""
    out = []
    for blk in ws.kernel_blocks(frame):
        iters = [per[i]["trace"]["iters"] for i in blk]
        out.append((len(blk), sum(int((it >= 3).sum()) for it in iters), ws.wave_counts(iters)))
    return out


def test_branch_batch_takes_every_named_branch(qualified):
    per = dict(qualified["branch_batch"])
    frames = dict(ws.branch_batch()["frames"])
    rows = lambda prefix: [r for name, p in per.items() if name.startswith(prefix) for _, r in sorted(p.items())]
    # exactly collinear, horizontal: err < EPS at restart 0 ends the restart at its first error sum and the selection at its first restart.  (Vertical and
    # 45 degree runs are in the batch too; their direction is cos / sin of a float angle, not 0 / 1, so their error sums are ~1e-4, not 0 -- unless the sample
    # is symmetric: among them are edges whose selection ends early at a LATER restart, which is asserted as well.)
    col = rows("collinear horizontal") + rows("collinear, short")
    assert len(col) >= 8
    for r in col:
        t = r["trace"]
        assert t["chosen"] == 0 and t["stopped"] and t["end"][0] == "eps" and t["iters"][0] == 1, (r["n"], t["end"], t["iters"])
    other = rows("collinear vertical") + rows("collinear 45")
    assert len(other) == 8 and any(r["trace"]["stopped"] and r["trace"]["chosen"] > 0 for r in other) and any(not r["trace"]["stopped"] for r in other)
    # collinear but one point: no restart can end below EPS (the odd point's distance alone is above it); restarts whose sample holds the odd
    # point take more iterations than the others, so the restarts of one edge end at different iterations
    one = rows("collinear but one")
    assert all((r["trace"]["end"] == "converged").all() and not r["trace"]["stopped"] for r in one)
    assert sum(len(set(r["trace"]["iters"])) > 1 for r in one) >= len(one) // 2
    # parallel groups: the unweighted refit
    par = rows("parallel pairs")
    assert any(r["trace"]["unweighted"].any() and not r["trace"]["unweighted"].all() for r in par)  # both refits among the restarts of one edge
    sparse = rows("sparse pairs")
    assert [r["n"] for r in sparse] == [u[0] for u in ws.UNWEIGHTED_CHOSEN]
    assert all(r["trace"]["unweighted"][r["trace"]["chosen"]] for r in sparse)  # ... and the line the edge ends with comes out of the unweighted one
    tiers = [0, ws.K["kWShort"], ws.K["kWCap"], ws.K["kWPts"], ws.K["kWPtsU"], ws.K["kLatPoints"], ws.K["kPickN2"]]
    assert all(any(lo < r["n"] <= hi for r in sparse) for lo, hi in zip(tiers, tiers[1:]))
    assert {min(-(-r["n"] // ws.K["kLatChunk"]), 5) for r in sparse} == {1, 2, 3, 4, 5}  # chunks of the few-frame kernel (5: the frame it declines)
    # two restarts tie at the smallest error sum with different lines: the first must win
    for c, r in zip(frames["tied restarts"], rows("tied restarts")):
        t = r["trace"]
        tied = [k for k in range(20) if t["err"][k] == t["err"][t["chosen"]] and line_distance(c, t["lines"][k], t["lines"][t["chosen"]]) > 1e-2]
        assert tied and min(tied) > t["chosen"], (t["chosen"], tied)
    # degenerate clusters
    deg = per["degenerate"]
    assert [len(np.unique(c, axis=0)) for c in frames["degenerate"]] == [1, 1, 1, 2, 2, 2]
    assert all(deg[i]["trace"]["stopped"] and deg[i]["trace"]["chosen"] == 0 for i in range(3))  # all points equal: an error sum of exactly 0
    # far from the origin
    far = frames["far from the origin"]
    assert sum(3000 < c.max() < 4200 for c in far) >= 4 and sum(c.max() > 64000 for c in far) >= 4 and max(c.max() for c in far) == 65535
    # slow convergence
    slow = np.concatenate([r["trace"]["iters"] for r in rows("L shapes") + rows("arcs")])
    assert (slow == 3).any() and (slow == 4).any() and (slow >= 5).any(), np.bincount(slow)
    # the cap of 30 iterations, on the chosen restart
    cap = rows("the 30-iteration cap")
    assert len(cap) == len(ws.CAP_SEEDS) and all(r["trace"]["end"][r["trace"]["chosen"]] == "cap" and r["trace"]["iters"][r["trace"]["chosen"]] == 30 for r in cap)
    # the three designed blocks: 0 of 240, all 240, a different count from each of the four waves
    blocks = {name: _block_counts(per[name], frames[name]) for name in ws.DESIGNED_BLOCKS}
    print(blocks)
    none, full, uneven = (blocks[k] for k in ws.DESIGNED_BLOCKS)
    assert none == [(12, 0, [0, 0, 0, 0])]
    assert full == [(12, 240, [64, 64, 64, 48])]
    assert len(uneven) == 1 and uneven[0][0] == 12 and 0 < uneven[0][1] < 240
    assert len(set(uneven[0][2])) == 4 and min(uneven[0][2]) > 0 and all(c < 64 for c in uneven[0][2]), uneven
    ends = np.concatenate([r["trace"]["end"] for r in _flat(qualified, "branch_batch")])
    assert {"converged", "eps", "cap"} == set(ends)


def test_block_mix_blocks_regroup_some_restarts(qualified):
    """Every full block of the benign frames hands SOME of its 240 restarts on past iteration 2 -- between the none and the all of the two blocks of
    branch_batch built to those counts -- and the blocks differ in how many."""
    shares = []
    for (name, per), (_, frame) in zip(qualified["block_mix"], ws.block_mix()["frames"]):
        for edges, past, waves in _block_counts(per, frame):
            assert 0 <= past <= 20 * edges
            if edges == ws.K["kWE"]:
                assert 0 < past < 240, (name, past)
                shares.append(past)
    print("block_mix: %d full blocks, restarts past iteration 2 per block: min %d, median %d, max %d of 240" % (
        len(shares), min(shares), int(np.median(shares)), max(shares)))
    assert len(shares) >= 100 and len(set(shares)) > 20


def test_size_edges_are_benign(qualified):
    """What the default geometry is for: no unweighted refit -- the tiers are the only thing these clusters vary."""
    ends = {}
    for r in _flat(qualified, "size_edges"):
        t = r["trace"]
        assert not t["unweighted"].any(), r["n"]
        for e in t["end"]:
            ends[e] = ends.get(e, 0) + 1
    print("size_edges: how the restarts end:", ends)


# ------------------------------------------------------------------------------------------------ planted errors

def _mutant(old, new):
    """The statement with one piece of its text replaced."""
    src = inspect.getsource(et.fitline_welsch)
    assert src.count(old) == 1, old
    scope = dict(vars(et))
    exec(compile(src.replace(old, new), "<planted error>", "exec"), scope)
    return scope["fitline_welsch"]


PLANTED = {
    "a restart's picks shifted by one": dict(edit=("w = _rng_subsets(n).astype(dt)", "w = _rng_subsets(n).astype(dt); w[3] = np.roll(w[3], 1)")),
    "<= for < in the selection": dict(edit=("if err[k] < min_err:", "if err[k] <= min_err:")),
    "the cap at 29": dict(edit=("for it in range(30):", "for it in range(29):")),
    "the unweighted refit skipped": dict(edit=("big = np.abs(sw) > FLT_EPSILON\n", "big = np.abs(sw) > -1.0\n")),
    "the last point dropped": dict(pts=lambda c: c[:-1] if len(c) > 2 else c),
    "weights from the previous line": dict(edit=(
        "        ww = np.exp(-dist * dist * c * c) if f64 else MATH.expf(-dist * dist * c * c)\n",
        "        if it:\n"
        "            dist = np.abs(prev[:, 1:2] * (px[None, :] - prev[:, 2:3]) + (-prev[:, 0:1]) * (py[None, :] - prev[:, 3:4]))\n"
        "        ww = np.exp(-dist * dist * c * c) if f64 else MATH.expf(-dist * dist * c * c)\n")),
    "points in reversed order": dict(pts=lambda c: c[::-1]),
    "EPS without the factor n": dict(edit=("EPS = n * FLT_EPSILON", "EPS = FLT_EPSILON")),
}
# What the comparison at SAME_LINE_PX cannot see, by construction: an error sum below n * FLT_EPSILON puts every point within 1e-7 px of the line, so a
# restart that goes on instead of ending there refits to the same line within float rounding, and whichever restart the selection then takes lies within
# that of it too -- the planted error moves lines by ~1e-7 px, a thousandth of the bar.  (The kernels are held to the oracle byte for byte on the GPU.)
# Such an error is pinned by the trace instead: branch_batch must hold clusters whose restarts END differently under it (test below).
BELOW_THE_BAR = {"EPS without the factor n"}


@pytest.mark.parametrize("what", list(PLANTED))
def test_the_comparison_refuses_a_planted_error(qualified, oracle, what):
    plant = PLANTED[what]
    statement = _mutant(*plant["edit"]) if "edit" in plant else et.fitline_welsch
    noticed = []
    for name in ("branch_batch", "size_edges"):
        results, labels = [], []
        for fname, frame in ws.BATCHES[name]()["frames"]:
            if name == "size_edges" and not fname.startswith("only"):
                continue
            for i, c in enumerate(frame):
                results.append(qualify(oracle, c, statement, plant["pts"](c) if "pts" in plant else None))
                labels.append("%s / %s, cluster %d of %d points" % (name, fname, i, len(c)))
        ok, text, first = verdict(results, allow_excuses=name != "size_edges")
        if not ok:
            noticed.append("%s: %s [%s]" % (name, text, labels[first]))
    print("%s: %s" % (what, "; ".join(noticed) if noticed else "not noticed"))
    if what in BELOW_THE_BAR:
        assert not noticed, "the comparison sees %s after all: take it out of BELOW_THE_BAR" % what
        # ... so the trace has to: clusters of branch_batch whose error sum lies in [FLT_EPSILON, n * FLT_EPSILON) end a restart (and the selection) there in
        # the statement and go on under the planted error
        changed = []
        for (fname, per), (_, frame) in zip(qualified["branch_batch"], ws.branch_batch()["frames"]):
            for i, c in enumerate(frame):
                t, m = per[i]["trace"], qualify(oracle, c, statement)["trace"]
                if list(t["end"]) != list(m["end"]) or t["stopped"] != m["stopped"] or list(t["iters"]) != list(m["iters"]):
                    assert (t["end"] == "eps").sum() > (m["end"] == "eps").sum(), (fname, i)  # only ever: fewer restarts end below EPS
                    whole = t["stopped"] and not m["stopped"] and et.FLT_EPSILON <= t["err"][t["chosen"]] < len(c) * et.FLT_EPSILON
                    changed.append(("%s, cluster %d of %d points%s" % (fname, i, len(c), " (the selection no longer ends early)" if whole else ""), whole))
        print("%s: the trace changes on %s" % (what, "; ".join(c for c, _ in changed)))
        assert any(whole for _, whole in changed), what
    else:
        assert noticed, what
