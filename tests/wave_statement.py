"""A plain statement of the wave primitives of cylindertag_amd/csrc/ctag_wave.h, written from the header's words: per-lane Python loops over
64-element lists, sharing nothing with the kernels.  A wave is a list of 64 values; `act` is a list of 64 bools (the lanes that are on where the
primitive is called).  A result is a list of 64 values with None on the lanes that were off.  Words are Python ints (bit patterns: a float or a double
moves as its bits); only the FP64 tree sum and the two maxima compute with numbers.

What the header states about lanes that are off (the contract, tests/test_wave_primitives_gpu.py holds the device to it):
  lane moves            any mask; a source lane that is off counts as no source: the reader gets 0
  sg_sum<8>, sg_best<8> a sub-group of 8 lanes is on or off as a whole; each sub-group that is on reduces over its own 8 lanes
  wave_incl_scan, sg_sum<64>, sg_best<64>, wave_sum_f64, wave_max_f64      all 64 lanes on (the caller's duty)
  wave_all              any mask; lanes that are off do not vote"""
import struct

import numpy as np

LANES = 64
ALL_ON = [True] * LANES
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def mask_to_act(mask):
    return [bool((int(mask) >> l) & 1) for l in range(LANES)]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def bits_f64(u):
    return struct.unpack("<d", struct.pack("<Q", u & M64))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def as_i64(u):
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def as_i32(u):
    u &= M32
    return u - (1 << 32) if u >> 31 else u


# ---- lane moves: where lane i takes its word from (None: no source) ---------------------------------------------------------------------------------
def src_prev(i):
    return i - 1 if i > 0 else None  # across the whole wave: lane 0 has no source


def src_next(i):
    return i + 1 if i < 63 else None  # lane 63 has no source


def src_shr(d):
    return lambda i: i - d if i % 16 >= d else None  # within the row of 16 lanes


def src_xor1(i):
    return i ^ 1


def src_xor2(i):
    return i ^ 2


def src_half_mirror(i):
    return (i - i % 8) + (7 - i % 8)  # lane 7 - i of its half row


def src_row_mirror(i):
    return (i - i % 16) + (15 - i % 16)  # lane 15 - i of its row


def lane_move(words, src, act=ALL_ON):
    out = []
    for i in range(LANES):
        if not act[i]:
            out.append(None)
            continue
        s = src(i)
        out.append(words[s] if s is not None and act[s] else 0)
    return out


# ---- scan and sums -------------------------------------------------------------------------------------------------------------------------------------
def incl_scan(words):
    """Inclusive sum over the wave, lane i = v[0] + ... + v[i], modulo 2^32 (all 64 lanes on)."""
    out, run = [], 0
    for i in range(LANES):
        run = (run + words[i]) & M32
        out.append(run)
    return out


def sg_sum(words, sg, bits, act=ALL_ON):
    """Every lane of a sub-group of `sg` lanes gets the sum of the sub-group's words, modulo 2^bits."""
    out = [None] * LANES
    for g0 in range(0, LANES, sg):
        lanes = range(g0, g0 + sg)
        on = [act[l] for l in lanes]
        assert all(on) or not any(on), "a sub-group is on or off as a whole"
        if not on[0]:
            continue
        total = 0
        for l in lanes:
            total += words[l]
        for l in lanes:
            out[l] = total & ((1 << bits) - 1)
    return out


# ---- the best (d, index) pair ------------------------------------------------------------------------------------------------------------------------
def _beats(order, od, oi, d, i):
    if order == "nearest":  # the smallest d, ties to the lowest index
        return od < d or (od == d and oi < i)
    if order == "farthest":  # the largest d, ties to the highest index
        return od > d or (od == d and oi > i)
    if order == "max_first":  # wave_max_f64: the largest d, ties to the lowest index
        return od > d or (od == d and oi < i)
    raise ValueError(order)


def sg_best(d, idx, sg, order, act=ALL_ON):
    """Every lane of a sub-group gets the pair (d, index) no other pair of the sub-group beats: (lane whose d is returned, index) per lane.  d are
    numbers without NaN; -0 and +0 are equal, so the index decides between them and the winner's own d (its sign included) is what comes back."""
    out = [None] * LANES
    for g0 in range(0, LANES, sg):
        lanes = list(range(g0, g0 + sg))
        on = [act[l] for l in lanes]
        assert all(on) or not any(on), "a sub-group is on or off as a whole"
        if not on[0]:
            continue
        best = lanes[0]
        for l in lanes[1:]:
            if _beats(order, d[l], idx[l], d[best], idx[best]):
                best = l
        for l in lanes:
            out[l] = (d[best], idx[best])
    return out


# ---- FP64 over the wave ---------------------------------------------------------------------------------------------------------------------------------
def wave_sum_f64(v):
    """The fixed tree: lane ^ 1, then lane ^ 2, then the other quad of 8, then the other half of the row, then ((r0 + r16) + r32) + r48.  numpy float64
    is IEEE binary64 with round to nearest even: the same bits as the device's v_add_f64."""
    v = [np.float64(x) for x in v]
    for src in (src_xor1, src_xor2, src_half_mirror, src_row_mirror):
        v = [v[i] + v[src(i)] for i in range(LANES)]
    return [((v[0] + v[16]) + v[32]) + v[48]] * LANES


def lane_order_sum(v):
    s = np.float64(v[0])
    for x in v[1:]:
        s = s + np.float64(x)
    return s


def wave_all(p, act=ALL_ON):
    """True when p holds on every lane that is on; lanes that are off do not vote."""
    verdict = True
    for i in range(LANES):
        if act[i] and not p[i]:
            verdict = False
    return [verdict if act[i] else None for i in range(LANES)]


# ---- packed 16-bit min / max ---------------------------------------------------------------------------------------------------------------------------
def pk_u16(a, b, pick):
    lo = pick(a & 0xffff, b & 0xffff)
    hi = pick((a >> 16) & 0xffff, (b >> 16) & 0xffff)
    return lo | (hi << 16)


# ---- one op of the probe (testkit.WAVE_OPS names), as (out bits, iout) per lane; None where the probe's result is not the primitive's ---------------
_MOVES32 = {"FROM_PREV": src_prev, "FROM_NEXT": src_next, "SHR1_I32": src_shr(1), "SHR2_I32": src_shr(2), "SHR4_I32": src_shr(4), "SHR1_F32": src_shr(1),
            "XOR1_I32": src_xor1, "XOR2_I32": src_xor2, "HALF_MIRROR_I32": src_half_mirror, "ROW_MIRROR_I32": src_row_mirror}
_MOVES64 = {"XOR1_I64": src_xor1, "XOR2_I64": src_xor2, "HALF_MIRROR_I64": src_half_mirror, "ROW_MIRROR_I64": src_row_mirror}
_BEST = {"SG_BEST8_NEAREST": (8, "nearest"), "SG_BEST8_FARTHEST": (8, "farthest"), "SG_BEST64_NEAREST": (64, "nearest"),
         "SG_BEST64_FARTHEST": (64, "farthest")}


def probe(name, mask, a, ia):
    """What ctag_testkit_wave_probe returns for one wave: a = 64 floats, ia = 64 signed 64-bit ints -> (out, iout), each a list of 64 entries: out as
    the double's BITS, iout as a signed int, None for a lane that was off or a result the op does not produce."""
    act = mask_to_act(mask)
    a = [float(x) for x in a]
    ia = [int(x) for x in ia]
    lo = [x & M32 for x in ia]
    none = [None] * LANES
    if name in _MOVES32:
        return none, lane_move(lo, _MOVES32[name], act)
    if name in _MOVES64:
        r = lane_move([x & M64 for x in ia], _MOVES64[name], act)
        return none, [None if x is None else as_i64(x) for x in r]
    if name == "SHR1_F64":
        return lane_move([f64_bits(x) for x in a], src_shr(1), act), none
    if name == "INCL_SCAN":
        assert all(act)
        return none, incl_scan(lo)
    if name in ("SG_SUM8_I32", "SG_SUM64_I32"):
        return none, sg_sum(lo, 8 if "8" in name else 64, 32, act)
    if name in ("SG_SUM8_I64", "SG_SUM64_I64"):
        r = sg_sum(ia, 8 if "8" in name else 64, 64, act)
        return none, [None if x is None else as_i64(x) for x in r]
    if name in _BEST:
        sg, order = _BEST[name]
        d = [float(np.float32(x)) for x in a]
        r = sg_best(d, [as_i32(x) for x in lo], sg, order, act)
        return [None if p is None else f64_bits(p[0]) for p in r], [None if p is None else p[1] for p in r]
    if name == "SUM_F64":
        assert all(act)
        return [f64_bits(x) for x in wave_sum_f64(a)], none
    if name == "MAX_F64":
        assert all(act)
        r = sg_best(a, [as_i32(x) for x in lo], 64, "max_first")
        return [f64_bits(p[0]) for p in r], [p[1] for p in r]
    if name == "ALL":
        r = wave_all([x != 0 for x in ia], act)
        return none, [None if x is None else int(x) for x in r]
    if name in ("PK_MIN_U16", "PK_MAX_U16"):
        pick = min if name == "PK_MIN_U16" else max
        return none, [pk_u16(ia[i] & M32, (ia[i] >> 32) & M32, pick) if act[i] else None for i in range(LANES)]
    raise ValueError(name)
