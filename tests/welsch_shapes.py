"""Edge clusters for the Welsch line fit (`k_line_sort` + `k_welsch` + `k_welsch_lat`, cylindertag_amd/csrc/k_quad.hip), built so that every size
tier, pick source, staging mode, loop and data-dependent branch of the kernels runs under a test -- and so that the tests can SAY which one ran.
Deterministic (fixed seeds), small, no GPU.  tests/test_welsch_statement_cpu.py qualifies every cluster here (oracle against the Python
statement, coverage from the statement's trace); tests/test_welsch_forms_gpu.py feeds the same clusters to the kernels.

A batch is a dict: "size" (rows, cols of the workspace it is meant for), "frames" (a list of (name, [clusters]); a cluster is an (n, 2) int32
array of x, y in walk order) and "calls" (dicts: "frames" = indices into the list, "latency" 0 / 1, "gx" / "gs" = k_welsch's blocks per
frame, 0 for the plan's, "tail" = the frame's clusters end at the end of the cluster pool).

The default geometry is what a silhouette edge looks like: a straight segment in a random direction inside 0..1919 x 0..1079, rounded to the grid
in walk order, every point moved by -1..1 px, a few outliers.  It is benign for the fit; the clusters of `branch_batch` are not."""
import functools

import numpy as np

# the kernels' constants (cylindertag_amd/csrc/k_quad.hip, ctag_internal.h); tests/test_welsch_statement_cpu.py reads them back from the sources
K = dict(kWShort=10, kWCap=16, kWRes=10, kWPts=128, kWPtsU=240, kPickN=256, kPickN2=4096, kWE=12, kWT=256, kLatLines=2048, kLatPoints=512,
         kLatChunk=128, kLdsLines=8192, kLatencyFrames=4, welsch_gx=18, welsch_gs=1, lat_rank_blocks=512, sort_top_bucket=2047)
SIZES = (2, 3, 9, 10, 11, 12, 15, 16, 17, 18, 20, 63, 64, 65, 127, 128, 129, 130, 239, 240, 241, 255, 256, 257, 383, 384, 385, 511, 512, 513,
         1023, 1025, 4095, 4096, 4097, 5000)
HD, UHD = (1080, 1920), (2160, 3840)


def segment(rng, n, outliers=True, box=(1920, 1080)):
    """n points of a straight segment in a random direction, rounded in walk order, none, a third or all of them moved by -1..1 px (how rough an edge
    is decides how many of its restarts settle within two refits), a few outliers."""
    W, H = box
    half = min(max(n * rng.uniform(0.8, 1.4), 4.0), 900.0) / 2  # clusters of more points than pixels along them repeat grid points
    ang = rng.uniform(0, 2 * np.pi)
    cx, cy = rng.uniform(half + 16, W - 17 - half), rng.uniform(half + 16, H - 17 - half)
    t = np.linspace(-half, half, n)
    rough = (0.0, 1 / 3, 1.0)[int(rng.integers(0, 3))]
    p = np.rint(np.stack([cx + t * np.cos(ang), cy + t * np.sin(ang)], 1)) + rng.integers(-1, 2, (n, 2)) * (rng.uniform(size=(n, 1)) < rough)
    if outliers and n >= 8:
        k = min(1 + n // 40, 6)
        idx = rng.choice(n, k, replace=False)
        p[idx] += rng.integers(-12, 13, (k, 2))
    p[:, 0] = np.clip(p[:, 0], 0, W - 1)
    p[:, 1] = np.clip(p[:, 1], 0, H - 1)
    return p.astype(np.int32)


def longest(frame):
    return max((len(c) for c in frame), default=0)


def _chunks(idx, size):
    return [idx[i:i + size] for i in range(0, len(idx), size)]


def kernel_blocks(frame):
    """The groups of kWE edges k_welsch's blocks fit together: the frame's edges of more than kWShort points in k_line_sort's order (descending
    point count, input order among equals), twelve at a time.  Returns lists of indices into the frame."""
    order = sorted((i for i, c in enumerate(frame) if len(c) > K["kWShort"]), key=lambda i: (-len(frame[i]), i))
    return _chunks(order, K["kWE"])


# ------------------------------------------------------------------------------------------------ size_edges

@functools.lru_cache(None)
def size_edges():
    rng = np.random.default_rng(20240601)
    frames = []
    tails = []
    for n in SIZES:
        frames.append(("only %d" % n, [segment(rng, n)]))
        if n <= K["kWShort"]:
            others = [int(rng.integers(2, n + 1)) for _ in range(11)]
        else:  # shorter edges of more than kWShort points: the same block, the staging mode of its longest edge
            others = [int(rng.integers(11, max(12, min(n, 301)))) for _ in range(11)]
        led = [segment(rng, m) for m in others]
        led.insert(int(rng.integers(0, 12)), segment(rng, n))
        frames.append(("%d leads a block" % n, led))
        for leader, mode, top in ((200, "packed words", K["kWPts"]), (300, "global memory", K["kWPtsU"])):
            if K["kWShort"] < n <= top:  # a shorter member of a block whose longest edge forces a higher mode on it
                f = [segment(rng, int(rng.integers(11, 100))) for _ in range(10)] + [segment(rng, leader)]
                f.insert(int(rng.integers(0, 12)), segment(rng, n))
                frames.append(("%d under a %d-point edge (%s)" % (n, leader, mode), f))
        tails.append(("%d at the end of the pool" % n, [segment(rng, 5), segment(rng, 20), segment(rng, 60), segment(rng, n)]))
    # a frame the few-frame kernel must decline for its edge count (the one it declines for its longest edge is "only 513")
    many = [segment(rng, int(rng.integers(2, 11))) for _ in range(K["kLatLines"] + 1 - 6)] + [segment(rng, m) for m in (11, 40, 129, 300, 511, 512)]
    frames.append(("%d edges" % (K["kLatLines"] + 1), many))
    first_tail = len(frames)
    frames += tails
    plain = list(range(first_tail))
    lat = [i for i in plain if longest(frames[i][1]) <= K["kLatPoints"] + 1]
    calls = [dict(frames=c, latency=0, gx=0, gs=0, tail=False) for c in _chunks(plain, 32)]
    calls += [dict(frames=c, latency=1, gx=0, gs=0, tail=False) for c in _chunks(lat, K["kLatencyFrames"])]
    calls += [dict(frames=[i], latency=0, gx=0, gs=0, tail=True) for i in range(first_tail, len(frames))]
    return dict(size=HD, frames=frames, calls=calls)


# ------------------------------------------------------------------------------------------------ block_mix

def _mixed_frame(rng, n_long, n_short):
    """n_long edges of more than kWShort points (mostly float-pair sized, some packed-word and global-memory sized) and n_short shorter, shuffled."""
    sizes = []
    for _ in range(n_long):
        u = rng.uniform()
        sizes.append(int(rng.integers(11, 60)) if u < 0.8 else int(rng.integers(60, 129)) if u < 0.95 else int(rng.integers(129, 300)))
    sizes += [int(rng.integers(2, 11)) for _ in range(n_short)]
    rng.shuffle(sizes)
    return [segment(rng, m) for m in sizes]


@functools.lru_cache(None)
def block_mix():
    rng = np.random.default_rng(20240602)
    frames, calls = [], []
    # block and grid looping: a block loops above welsch_gx * 12 long or welsch_gs * 256 short edges (defaults 18 / 1: 216 / 256)
    mix = [(1, 0), (11, 1), (12, 255), (13, 256), (24, 257), (25, 600), (216, 0), (217, 256), (440, 600), (0, 257), (216, 1)]
    for nl, ns in mix:
        frames.append(("%d long + %d short" % (nl, ns), _mixed_frame(rng, nl, ns)))
    for gx, gs in ((0, 0), (1, 1)):
        calls += [dict(frames=c, latency=0, gx=gx, gs=gs, tail=False) for c in _chunks(list(range(len(mix))), 6)]
    # 5 frames in one call (blockIdx.x above the frame count of a few-frame call), an empty frame between two full ones
    first = len(frames)
    frames += [("five: 30 + 40", _mixed_frame(rng, 30, 40)), ("five: empty", []), ("five: 14 + 300", _mixed_frame(rng, 14, 300)),
               ("five: only short", _mixed_frame(rng, 0, 90)), ("five: only long", _mixed_frame(rng, 26, 0))]
    calls.append(dict(frames=list(range(first, first + 5)), latency=0, gx=0, gs=0, tail=False))
    calls.append(dict(frames=list(range(first, first + 4)), latency=1, gx=0, gs=0, tail=False))
    # the few-frame kernel's 512 rank blocks loop up to four times
    first = len(frames)
    for L in (511, 512, 513, 1024, 2047, 2048):
        nl = 40
        frames.append(("%d edges for the few-frame kernel" % L, _mixed_frame(rng, nl, L - nl)))
    calls += [dict(frames=c, latency=1, gx=0, gs=0, tail=False) for c in _chunks(list(range(first, first + 6)), 3)]
    calls.append(dict(frames=list(range(first, first + 6)), latency=0, gx=2, gs=1, tail=False))
    return dict(size=HD, frames=frames, calls=calls)


# ------------------------------------------------------------------------------------------------ sort_forms

def _sort_frame(rng, L, box):
    sizes = [int(rng.integers(2, 12)) for _ in range(L - 15)] + [int(rng.integers(12, 301)) for _ in range(12)] + [2048, 2300, 3000]
    rng.shuffle(sizes)
    return [segment(rng, m, box=box) for m in sizes]


@functools.lru_cache(None)
def sort_forms():
    """k_line_sort's rank sort in LDS up to kLdsLines edges, its counting sort above; three edges share the counting sort's top bucket."""
    rng = np.random.default_rng(20240603)
    frames = [("%d edges" % L, _sort_frame(rng, L, (3840, 2160))) for L in (8191, 8192, 8193, 20000)]
    return dict(size=UHD, frames=frames, calls=[dict(frames=[0, 1, 2, 3], latency=0, gx=0, gs=0, tail=False)])


@functools.lru_cache(None)
def sort_forms_hd():
    rng = np.random.default_rng(20240604)
    return dict(size=HD, frames=[("8192 edges, a full 1080p workspace", _sort_frame(rng, 8192, (1920, 1080)))],
                calls=[dict(frames=[0], latency=0, gx=0, gs=0, tail=False)])


def statement_sample(frame, count=512):
    """The clusters of a sort_forms frame the Python statement is run on: every one of more than 11 points and a fixed choice of the rest."""
    big = [i for i, c in enumerate(frame) if len(c) > 11]
    rest = [i for i, c in enumerate(frame) if len(c) <= 11]
    pick = np.random.default_rng(len(frame)).choice(len(rest), count - len(big), replace=False)
    return sorted(big + [rest[i] for i in pick])


# ------------------------------------------------------------------------------------------------ branch_batch

def collinear(n, x0, y0, dx, dy):
    return np.stack([x0 + dx * np.arange(n), y0 + dy * np.arange(n)], 1).astype(np.int32)


def but_one(pts, at, off):
    p = pts.copy()
    p[at] += np.asarray(off, np.int32)
    return p


def parallel_pair(n, x0, y0, gap, dx=1, dy=0):
    """Two parallel runs of n points each, `gap` px apart, interleaved in walk order: a first sample that mixes them puts every point
    ~gap / 2 from the line, where exp(-d^2 / 2.9846^2) leaves a weight sum below FLT_EPSILON."""
    a = collinear(n, x0, y0, dx, dy)
    nx, ny = (-dy, dx)
    b = a + np.array([nx * gap, ny * gap], np.int32)
    out = np.empty((2 * n, 2), np.int32)
    out[0::2], out[1::2] = a, b
    return out


def sparse_pair(n, x0, y0, gap, step, seed):
    """Two parallel runs `gap` px apart whose points alternate between them, `step` px from one to the next: few points lie near any line, and the
    restarts whose first line runs between the two find a weight sum below FLT_EPSILON."""
    rng = np.random.default_rng(seed)
    x = x0 + step * np.arange(n) + rng.integers(0, max(step // 3, 1), n)
    y = y0 + gap * (np.arange(n) % 2) + rng.integers(-1, 2, n)
    return np.stack([x, y], 1).astype(np.int32)


# (points, gap, step, seed) of sparse pairs in which the CHOSEN restart went through the unweighted refit: one per size tier (a lane each; weights all
# cached; float pairs; packed words; global memory; one to five chunks of the few-frame kernel), the first of a
# search over 3 gaps x 3 steps x 4 seeds per size with the statement's trace
UNWEIGHTED_CHOSEN = ((8, 40, 60, 0), (10, 40, 60, 0), (12, 200, 58, 0), (16, 200, 62, 0), (40, 200, 17, 0), (100, 200, 10, 0), (128, 200, 7, 0), (140, 200, 5, 0),
                     (200, 200, 5, 0), (260, 200, 1, 1), (400, 200, 2, 0), (513, 120, 1, 0))


def ell(n, x0, y0, arm):
    """An L: `arm` of the n points along x, the rest up along y."""
    a = collinear(arm, x0, y0, 1, 0)
    b = collinear(n - arm, x0 + arm - 1, y0 + 1, 0, 1)
    return np.concatenate([a, b])


def arc(n, cx, cy, radius, a0, a1):
    a = np.linspace(a0, a1, n)
    return np.rint(np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], 1)).astype(np.int32)


def wave_counts(block_iters):
    """Restarts per wave of k_welsch's block that go on past the regroup at iteration 2, from the statement's trace of the block's edges
    in rank order (item = 20 * edge + restart, 64 items per wave)."""
    flat = np.concatenate([np.asarray(it) >= 3 for it in block_iters]) if block_iters else np.zeros(0, bool)
    flat = np.concatenate([flat, np.zeros(K["kWT"] - len(flat), bool)])
    return [int(flat[64 * w:64 * w + 64].sum()) for w in range(4)]


@functools.lru_cache(None)
def branch_batch():
    frames = []
    add = lambda name, *clusters: frames.append((name, list(clusters)))
    # err < EPS at restart 0: the selection's early end
    for n in (11, 40, 150, 300):
        add("collinear horizontal %d" % n, collinear(n, 100, 200 + n, 1, 0))
        add("collinear vertical %d" % n, collinear(n, 300 + n, 50, 0, 1))
        add("collinear 45 degrees %d" % n, collinear(n, 400, 60, 1, 1))
    add("collinear, short", collinear(2, 10, 10, 1, 0), collinear(5, 10, 20, 0, 1), collinear(10, 30, 30, 1, 1), collinear(7, 50, 90, 2, -1))
    # collinear but for one point
    for n, at, off in ((11, 5, (0, 3)), (12, 0, (0, 2)), (30, 29, (0, 7)), (64, 20, (1, 1)), (140, 70, (0, 25)), (260, 3, (0, 4)), (24, 12, (0, 1))):
        add("collinear but one %d" % n, but_one(collinear(n, 500, 300, 1, 0), at, off), but_one(collinear(n, 700, 100, 1, 1), at, (off[1], 0)),
            but_one(collinear(n, 900, 200, 0, 1), at, (off[1], 0)))
    # two parallel groups: the unweighted refit
    add("parallel pairs", parallel_pair(8, 100, 500, 40), parallel_pair(20, 200, 600, 40), parallel_pair(70, 300, 700, 40), parallel_pair(130, 400, 800, 40),
        parallel_pair(8, 1000, 300, 40, 0, 1), parallel_pair(30, 1200, 300, 28, 1, 1), parallel_pair(5, 50, 900, 40), parallel_pair(300, 1000, 900, 44))
    add("sparse pairs", *[sparse_pair(n, 100, 100, gap, step, seed) for n, gap, step, seed in UNWEIGHTED_CHOSEN])
    # two restarts with the same smallest error sum and different lines (found among 162 small pairs): the selection's `<` keeps the first
    add("tied restarts", parallel_pair(6, 100, 200, 40, 3, 0), np.concatenate([collinear(6, 100, 200, 2, 0), collinear(6, 100, 240, 2, 0)]),
        parallel_pair(6, 100, 200, 36, 3, 0), np.concatenate([collinear(6, 100, 200, 3, 0), collinear(6, 100, 244, 3, 0)]))
    # degenerate
    add("degenerate", np.tile(np.array([[77, 88]], np.int32), (2, 1)), np.tile(np.array([[640, 360]], np.int32), (9, 1)),
        np.tile(np.array([[1900, 1000]], np.int32), (30, 1)), np.tile(np.array([[10, 20], [30, 25]], np.int32), (8, 1)),
        np.tile(np.array([[1500, 40], [1400, 640]], np.int32), (70, 1)), np.tile(np.array([[5, 5], [6, 5]], np.int32), (3, 1)))
    # large coordinates: float cancellation in the moments
    rng = np.random.default_rng(20240605)
    far = []
    for base in (3800, 65000):
        for n in (8, 30, 200):
            s = segment(rng, n)
            s = s - s.min(0) + np.array([base - 300, base - 300])
            far.append(np.clip(s, 0, 65535).astype(np.int32))
        far.append(collinear(50, base, base - 200, 1, 3) if base < 5000 else collinear(50, 65000, 65300, 1, -3))
        far.append(but_one(collinear(40, base - 100, base, 2, 1), 7, (0, 5)))
    far.append(np.array([[65535, 65535], [0, 0], [65535, 0], [0, 65535], [65535, 65534], [1, 0], [65534, 1], [3, 65535], [65535, 65535], [0, 0], [40000, 40000]],
                        np.int32))
    add("far from the origin", *far)
    # slow convergence: 3, 4 and more iterations
    add("L shapes", ell(40, 100, 100, 20), ell(90, 300, 100, 30), ell(200, 600, 100, 120), ell(23, 900, 100, 11), ell(300, 1200, 100, 150))
    add("arcs", arc(60, 500, 500, 300, 0.2, 0.5), arc(200, 500, 500, 400, 0.1, 0.9), arc(120, 900, 500, 150, 1.0, 2.2), arc(500, 960, 540, 500, 3.2, 4.6),
        arc(35, 300, 700, 60, 0.0, 1.2))
    add("the 30-iteration cap", *[_wiggle(n, 1000, 300, sd) for n, sd in CAP_SEEDS])
    for name, f in DESIGNED_BLOCKS.items():
        frames.append((name, f()))
    calls = [dict(frames=c, latency=0, gx=0, gs=0, tail=False) for c in _chunks(list(range(len(frames))), 32)]
    lat = [i for i in range(len(frames)) if longest(frames[i][1]) <= K["kLatPoints"]]
    calls += [dict(frames=c, latency=1, gx=0, gs=0, tail=False) for c in _chunks(lat, K["kLatencyFrames"])]
    return dict(size=HD, frames=frames, calls=calls)


def _block_none():
    """Twelve exactly collinear edges: every restart ends below EPS at iteration 0, none reaches the regroup."""
    return [collinear(60 - 4 * i, 100 + 10 * i, 100 + 30 * i, 1, (i % 3) - 1) for i in range(12)]


def _wiggle(n, x0, y0, seed):
    """A wide band of scattered points: no restart settles within two refits."""
    rng = np.random.default_rng(seed)
    x = x0 + np.arange(n) // 2
    y = y0 + rng.integers(-9, 10, n) + (np.arange(n) // 7)
    return np.stack([x, y], 1).astype(np.int32)


# (points, seed) of twelve bands in which all 20 restarts go on past iteration 2 -- the smallest seed per size that does, found with the statement's
# trace; tests/test_welsch_statement_cpu.py asserts it of every one
WIGGLE_SEEDS_ALL = ((120, 0), (114, 0), (108, 0), (102, 0), (96, 0), (90, 0), (84, 1), (78, 0), (72, 0), (66, 0), (60, 0), (54, 0))
# rank order of a block whose four waves (64 items = 3.2 edges each) hand on different counts: bands (seed >= 0), exactly collinear edges (-1: none of
# the 20 goes on) and plain segments (-2: some do)
WIGGLE_SEEDS_SOME = ((120, 0), (114, 0), (108, 0), (100, -1), (96, 0), (90, 0), (84, -2), (80, -1), (70, -2), (60, 0), (50, -1), (40, -2))
# bands whose CHOSEN restart runs into fitLine2D's cap of 30 iterations (a seed search over 100 seeds per size found two or more for each)
CAP_SEEDS = ((30, 16), (30, 19), (60, 6), (60, 10), (100, 0), (100, 5), (140, 0), (140, 2))


def _block_all():
    return [_wiggle(n, 100 + 5 * i, 100 + 60 * i, s) for i, (n, s) in enumerate(WIGGLE_SEEDS_ALL)]


def _block_uneven():
    rng = np.random.default_rng(20240606)
    return [_wiggle(n, 900 + 5 * i, 100 + 60 * i, s) if s >= 0 else collinear(n, 900 + 5 * i, 100 + 60 * i, 1, 0) if s == -1 else segment(rng, n)
            for i, (n, s) in enumerate(WIGGLE_SEEDS_SOME)]


DESIGNED_BLOCKS = {"block: no restart past iteration 2": _block_none, "block: all 240 restarts past iteration 2": _block_all,
                   "block: uneven survivors per wave": _block_uneven}

BATCHES = {"size_edges": size_edges, "block_mix": block_mix, "sort_forms": sort_forms, "sort_forms_hd": sort_forms_hd, "branch_batch": branch_batch}


def probe_mismatches(det, batch, fit, calls=None, cache=None):
    """Every call of the batch (or `calls`) through the test kit's probe of the stage (testkit.Detector.welsch_fit) on the workspace of det's last chunk;
    `fit(cluster)` is the reference line; `cache`: a dict of the caller's that keeps the lines of ONE `fit` between calls.  All 16 bytes of every line count.  Returns (lines compared, [text per line that differs])."""
    bad, compared = [], 0
    _cache = {} if cache is None else cache
    for call in batch["calls"] if calls is None else calls:
        names = [batch["frames"][i][0] for i in call["frames"]]
        frames = [batch["frames"][i][1] for i in call["frames"]]
        got = det.welsch_fit(frames, call["latency"], call["gx"], call["gs"], call["tail"])
        at = 0
        for name, frame in zip(names, frames):
            for j, c in enumerate(frame):
                key = c.tobytes()
                if key not in _cache:
                    _cache[key] = np.asarray(fit(c), np.float32)
                compared += 1
                if got[at].tobytes() != _cache[key].tobytes():
                    bad.append("%s, cluster %d of %d points (latency %d, gx %d, gs %d, tail %d): %s, want %s" % (
                        name, j, len(c), call["latency"], call["gx"], call["gs"], call["tail"], got[at], _cache[key]))
                at += 1
    return compared, bad
