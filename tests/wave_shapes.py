"""Fixed inputs for the wave primitives of cylindertag_amd/csrc/ctag_wave.h, shared by tests/test_wave_statement_cpu.py (which shows that they
discriminate) and tests/test_wave_primitives_gpu.py (which holds the device to tests/wave_statement.py on them).  A case is (label, masks uint64 [n],
a float64 [n, 64], ia int64 [n, 64]); every shape is a few dozen waves.  Nothing here is random between runs."""
import numpy as np

EDGES = (0, 15, 16, 31, 32, 47, 48, 63)  # the row and wave edges, where "a lane without a source gets 0" is decided
ALL = np.uint64(0xffffffffffffffff)
M64 = (1 << 64) - 1

MOVE_OPS = ("FROM_PREV", "FROM_NEXT", "SHR1_I32", "SHR2_I32", "SHR4_I32", "SHR1_F32", "SHR1_F64", "XOR1_I32", "XOR2_I32", "HALF_MIRROR_I32", "ROW_MIRROR_I32",
            "XOR1_I64", "XOR2_I64", "HALF_MIRROR_I64", "ROW_MIRROR_I64")
SUM_OPS = ("SG_SUM8_I32", "SG_SUM64_I32", "SG_SUM8_I64", "SG_SUM64_I64")
BEST_OPS = ("SG_BEST8_NEAREST", "SG_BEST8_FARTHEST", "SG_BEST64_NEAREST", "SG_BEST64_FARTHEST")
PK_OPS = ("PK_MIN_U16", "PK_MAX_U16")


def _i64(words):
    """unsigned 64-bit Python ints -> the int64 array with those bits"""
    return np.array([int(w) & M64 for w in np.ravel(words)], np.uint64).view(np.int64).reshape(np.shape(words))


def _bits(lanes):
    m = 0
    for l in lanes:
        m |= 1 << l
    return m


def _masks(words):
    return np.array([int(w) & M64 for w in words], np.uint64)


def lane_masks():
    """All on; alternate lanes; whole rows and whole sub-groups off; the edge lanes alone off and alone on; a lane's source alone off; fixed-seed ones."""
    rng = np.random.RandomState(101)
    m = [M64, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa, 0x0000ffff0000ffff, 0xffff0000ffff0000, 0x00ff00ff00ff00ff, 0xff00ff00ff00ff00,
         M64 ^ _bits(EDGES), _bits(EDGES), M64 ^ _bits((1, 14, 17, 30, 33, 46, 49, 62)), 1, 1 << 63]
    m += [int(rng.randint(0, 1 << 32)) | (int(rng.randint(0, 1 << 32)) << 32) for _ in range(8)]
    return _masks(m)


def subgroup_masks():
    """Masks whose 8-lane sub-groups are on or off as a whole."""
    rng = np.random.RandomState(102)
    bytes_on = [0xff, 0x55, 0xaa, 0x01, 0x80, 0x0f, 0xf0] + [int(b) for b in rng.randint(1, 256, 5)]
    return _masks([sum(0xff << (8 * g) for g in range(8) if (b >> g) & 1) for b in bytes_on])


def distinct_words(n_waves, seed):
    """Every lane a distinct nonzero 64-bit word whose halves differ and are nonzero: a wrong source lane, or a half that did not move, is visible."""
    out = np.zeros((n_waves, 64), np.uint64)
    for w in range(n_waves):
        for l in range(64):
            v = ((0x9e3779b97f4a7c15 * (seed * 4096 + 64 * w + l + 1)) ^ (0xd1b54a32d192ed03 * (l + 1))) & M64
            lo, hi = v & 0xffffffff, v >> 32
            lo, hi = lo or 0x1234567, hi or 0x7654321
            if lo == hi:
                hi ^= 0x10001
            out[w, l] = lo | (hi << 32)
    assert len(set(out.ravel() & np.uint64(0xffffffff))) == out.size and len(set(out.ravel() >> np.uint64(32))) == out.size
    return out


def move_cases():
    masks = lane_masks()
    n = len(masks)
    words = distinct_words(n, 1)
    rng = np.random.RandomState(103)
    dbl = rng.uniform(1.0, 2.0, (n, 64)) * 10.0 ** rng.randint(-200, 200, (n, 64)) * rng.choice([-1.0, 1.0], (n, 64))
    u = dbl.view(np.uint64)
    assert ((u >> np.uint64(32)) != (u & np.uint64(0xffffffff))).all() and len(set(u.ravel())) == u.size  # both halves of a double are told apart
    return [("distinct words under every mask", masks, dbl, words.view(np.int64))]


def scan_cases():
    rng = np.random.RandomState(104)
    rows = [np.ones(64, np.int64)]
    for l in EDGES:  # a single 1: the carries of row_bcast:15 (lanes 15, 47) and row_bcast:31 (lane 31) and every row's first and last lane
        r = np.zeros(64, np.int64)
        r[l] = 1
        rows.append(r)
    rows += [rng.randint(-2 ** 31, 2 ** 31, 64).astype(np.int64) for _ in range(8)]
    rows += [rng.randint(2 ** 29, 2 ** 31, 64).astype(np.int64) for _ in range(4)]  # the running sum wraps past 2^31 within a few lanes
    rows += [np.full(64, 2 ** 31 - 1, np.int64), np.full(64, -2 ** 31, np.int64), (np.int64(1) << (np.arange(64) % 32))]
    ia = np.stack(rows) & np.int64(0xffffffff)
    return [("ones, single ones, random, wrapping", np.full(len(ia), ALL), np.zeros(ia.shape), ia)]


def sum_cases(op):
    rng = np.random.RandomState(105)
    rows = [rng.randint(-2 ** 31, 2 ** 31, 64).astype(np.int64) for _ in range(6)]
    rows += [np.int64(1) << np.arange(64).astype(np.int64)]  # lane l holds bit l: every lane is counted exactly once
    if op.endswith("I64"):
        rows += [rng.randint(-2 ** 62, 2 ** 62, 64, dtype=np.int64) for _ in range(6)]                # above 2^32, and negative
        rows += [np.full(64, 0xffffffff, np.int64), np.full(64, -1, np.int64), np.full(64, 0x80000000, np.int64)]  # the carry between the two halves
        rows += [rng.randint(0, 2, 64).astype(np.int64) * np.int64(0xffffffff) + rng.randint(-4, 4, 64)]
    ia = np.stack(rows)
    if op.endswith("I32"):
        ia = ia & np.int64(0xffffffff)
    cases = [("all lanes on", np.full(len(ia), ALL), np.zeros(ia.shape), ia)]
    if "SUM8" in op:
        sm = subgroup_masks()
        pick = ia[np.arange(len(sm)) % len(ia)]
        cases.append(("whole sub-groups off", sm, np.zeros(pick.shape), pick))
    return cases


def tie_rows():
    """(d, index) waves on which the tie rule alone decides: all d equal; equal bests in different rows of the wave and in the two quads of every
    sub-group; -0 and +0, equal as numbers.  The indices are distinct within a wave, in lane order and against it."""
    d, idx = [], []
    lane = np.arange(64)
    for order in (lane, 63 - lane, (lane * 37 + 11) % 64 - 20):
        d.append(np.full(64, 2.5))                                        # all equal
        idx.append(order)
        for base, best in ((5.0, 9.0), (5.0, 1.0)):
            r = np.full(64, base)
            r[[3, 20, 37, 60]] = best                                         # equal bests in the four rows of the wave
            d.append(r)
            idx.append(order)
            r = np.full(64, base)
            r[(lane % 8 == 2) | (lane % 8 == 5)] = best                       # in the two quads of every sub-group
            d.append(r)
            idx.append(order)
        for k in range(3):
            d.append(np.where(lane % 3 == k, -0.0, 0.0))                   # +0 / -0
            idx.append(order)
    return np.stack(d), np.stack(idx).astype(np.int64)


def best_cases(op):
    rng = np.random.RandomState(106)
    lane = np.arange(64)
    td, ti = tie_rows()
    d, idx = list(td), list(ti)
    for win in (0, 7, 8, 15, 16, 63):  # the winner at a sub-group's, a row's and the wave's ends, for either order
        for base, best in ((5.0, 9.0), (5.0, 1.0)):
            r = np.full(64, base)
            r[win] = best
            d.append(r)
            idx.append((lane + 100) if best > base else (163 - lane))
    d.append(np.full(64, -np.inf))
    idx.append(lane)
    r = np.full(64, -np.inf)
    r[[9, 41]] = -3.0
    d.append(r)
    idx.append(63 - lane)
    r = rng.randint(0, 4, 64).astype(np.float64)
    r[rng.randint(0, 64, 9)] = -np.inf
    d.append(r)
    idx.append(rng.permutation(64))
    # the pairs the call sites start from on a lane without a point: (3.0e38, INT_MAX) for the nearest, (-1, -1) for the farthest, (-1, INT_MAX) for the maximum
    r, ix = rng.randint(0, 3, 64).astype(np.float64), rng.permutation(64).astype(np.int64)
    none = rng.rand(64) < 0.5
    d.append(np.where(none, float(np.float32(3.0e38)), r))
    idx.append(np.where(none, 2 ** 31 - 1, ix))
    d.append(np.where(none, -1.0, r))
    idx.append(np.where(none, -1, ix))
    d.append(np.where(none, -1.0, r))
    idx.append(np.where(none, 2 ** 31 - 1, ix))
    for _ in range(8):  # few distinct values: ties everywhere
        d.append(rng.randint(0, 4, 64).astype(np.float64))
        idx.append(rng.permutation(64) - rng.randint(0, 40))
    if op == "MAX_F64":  # doubles one ulp apart, which a comparison in float would call equal
        for _ in range(4):
            d.append(1.0 + rng.randint(0, 3, 64) * 2.0 ** -52)
            idx.append(rng.permutation(64))
    a, ia = np.stack(d), np.stack(idx).astype(np.int64) & np.int64(0xffffffff)
    cases = [("all lanes on", np.full(len(a), ALL), a, ia)]
    if "BEST8" in op:
        sm = subgroup_masks()
        k = np.arange(len(sm)) % len(a)
        cases.append(("whole sub-groups off", sm, a[k], ia[k]))
    return cases


def cancellation_rows(n_waves=32):
    """Mixed-sign magnitudes over 1e-8 .. 1e8: the sum in lane order and the tree sum differ in bits on most waves."""
    rng = np.random.RandomState(107)
    return 10.0 ** rng.uniform(-8, 8, (n_waves, 64)) * rng.choice([-1.0, 1.0], (n_waves, 64))


def sum_f64_cases():
    rows = [cancellation_rows(), np.full((1, 64), -0.0), np.zeros((1, 64)), np.ones((1, 64)), 2.0 ** np.arange(64)[None, :]]
    single = np.zeros((len(EDGES), 64))
    for k, l in enumerate(EDGES):
        single[k, l] = 1.0 + 2.0 ** -30 * (l + 1)  # one nonzero lane: every row's value reaches the result
    a = np.concatenate(rows + [single])
    return [("cancellation, zeros, single lanes", np.full(len(a), ALL), a, np.zeros(a.shape, np.int64))]


def all_cases():
    rng = np.random.RandomState(108)
    masks, ia = [M64], [np.ones(64, np.int64)]
    for l in (0, 31, 32, 63):
        p = np.ones(64, np.int64)
        p[l] = 0
        masks += [M64, M64 ^ (1 << l), M64 ^ (1 << l) ^ (1 << (l ^ 5)), 1 << l, 1 << (l ^ 1)]  # the false lane votes; is off; another lane is off; alone; another lane alone
        ia += [p] * 5
    p = np.zeros(64, np.int64)
    masks += [M64, 1]
    ia += [p, p]
    for _ in range(8):
        masks.append(int(rng.randint(0, 1 << 32)) | (int(rng.randint(0, 1 << 32)) << 32))
        ia.append((rng.rand(64) < 0.97).astype(np.int64) * rng.randint(1, 2 ** 40))
    ia = np.stack(ia)
    return [("votes under masks", _masks(masks), np.zeros(ia.shape), ia)]


def pk_cases():
    rng = np.random.RandomState(109)
    pairs = [(0x0001ffff, 0xffff0001), (0xffff0001, 0x0001ffff), (0x12341234, 0x12341234), (0, 0xffffffff), (0xffffffff, 0), (0xffff0000, 0x0000ffff),
             (0x7fff8000, 0x80007fff), (0, 0), (0xffffffff, 0xffffffff), (0x00010000, 0x0000ffff)]  # halves that order differently, equal halves, 0 and 0xffff
    pairs += [(int(rng.randint(0, 1 << 32)), int(rng.randint(0, 1 << 32))) for _ in range(128 - len(pairs))]
    ia = _i64([a | (b << 32) for a, b in pairs]).reshape(2, 64)
    ia = np.concatenate([ia, ia])
    masks = _masks([M64, M64, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa])
    return [("halves that order differently", masks, np.zeros(ia.shape), ia)]


def cases(op):
    if op in MOVE_OPS:
        return move_cases()
    if op == "INCL_SCAN":
        return scan_cases()
    if op in SUM_OPS:
        return sum_cases(op)
    if op in BEST_OPS or op == "MAX_F64":
        return best_cases(op)
    if op == "SUM_F64":
        return sum_f64_cases()
    if op == "ALL":
        return all_cases()
    if op in PK_OPS:
        return pk_cases()
    raise ValueError(op)
