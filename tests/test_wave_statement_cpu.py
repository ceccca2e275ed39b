"""tests/wave_statement.py held to numpy wherever numpy says the same thing, and tests/wave_shapes.py shown to discriminate: the conditions on
the shapes that tests/test_wave_primitives_gpu.py relies on are checked here, without a GPU."""
import math
import os
import re

import numpy as np

import testkit as tk
import wave_shapes as ws
import wave_statement as st

U = 2.0 ** -53
GAMMA7 = 7 * U / (1 - 7 * U)  # a value passes through at most seven additions of the tree (four in the row, three across the rows)


def test_op_codes_are_the_header_s():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctag_testkit.h")).read()
    codes = {n: int(v) for n, v in re.findall(r"#define CTAG_WAVE_([A-Z0-9_]+) (\d+)\n", hdr)}
    assert codes.pop("OPS") == len(tk.WAVE_OPS) and codes == {n: i for i, n in enumerate(tk.WAVE_OPS)}
    assert all(getattr(tk, "WAVE_" + n) == i for i, n in enumerate(tk.WAVE_OPS))
    assert "(%r)" % tk.WAVE_SENTINEL_F64 in hdr and "(-0x%xLL)" % -tk.WAVE_SENTINEL_I64 in hdr


def test_every_op_has_shapes_within_its_contract():
    n_waves = 0
    for op in tk.WAVE_OPS:
        for label, masks, a, ia in ws.cases(op):
            assert masks.dtype == np.uint64 and a.shape == ia.shape == (len(masks), 64) and ia.dtype == np.int64, (op, label)
            assert 1 <= len(masks) <= 96, (op, label)
            assert not np.isnan(a).any(), (op, label)  # NaN is out of contract for the bests and the maximum
            for w in range(len(masks)):
                st.probe(op, masks[w], a[w], ia[w])  # asserts the mask rules of the whole-wave and the 8-lane forms
            n_waves += len(masks)
    assert n_waves < 1200  # the whole GPU file stays a matter of seconds


def test_lane_moves_are_the_stated_permutations():
    w = list(range(100, 164))
    assert st.lane_move(w, st.src_prev) == [0] + w[:-1] and st.lane_move(w, st.src_next) == w[1:] + [0]
    lane = np.arange(64)
    for d in (1, 2, 4):
        want = np.where(lane % 16 >= d, np.array(w)[np.maximum(lane - d, 0)], 0)
        assert st.lane_move(w, st.src_shr(d)) == list(want)
    for src, perm in ((st.src_xor1, lane ^ 1), (st.src_xor2, lane ^ 2), (st.src_half_mirror, lane ^ 7), (st.src_row_mirror, lane ^ 15)):
        assert st.lane_move(w, src) == list(np.array(w)[perm])
    # a source that is off is no source; a reader that is off has no result
    act = [l not in (4, 15) for l in range(64)]
    got = st.lane_move(w, st.src_prev, act)
    assert got[5] == 0 and got[16] == 0 and got[4] is None and got[6] == w[5]
    # the shapes: every word distinct and nonzero in both halves, so each of these moves changes every lane that has a source
    _, masks, dbl, words = ws.move_cases()[0]
    u = words.view(np.uint64)
    assert (u & np.uint64(0xffffffff)).all() and (u >> np.uint64(32)).all() and len(set(u.ravel())) == u.size
    assert int(masks[0]) == st.M64 and all(any(not (int(m) >> l) & 1 for m in masks) for l in ws.EDGES)


def test_scan_is_cumsum_modulo_2_32():
    _, masks, _, ia = ws.scan_cases()[0]
    wrapped = 0
    for w in range(len(ia)):
        got = st.incl_scan([int(x) for x in ia[w]])
        want = np.cumsum(ia[w].astype(object)) % (1 << 32)
        assert got == [int(x) for x in want]
        wrapped += int(np.cumsum(ia[w].astype(object))[-1]) >= 1 << 31
    assert wrapped >= 8  # running sums that pass 2^31
    singles = [list(r).index(1) for r in ia[1:9]]
    assert tuple(singles) == ws.EDGES and all(r.sum() == 1 for r in ia[1:9])


def test_sg_sum_is_the_sum_of_its_lanes():
    for op in ws.SUM_OPS:
        sg, bits = (8 if "SUM8" in op else 64), (32 if op.endswith("I32") else 64)
        for label, masks, _, ia in ws.cases(op):
            for w in range(len(ia)):
                _, got = st.probe(op, masks[w], np.zeros(64), ia[w])
                for g0 in range(0, 64, sg):
                    on = (int(masks[w]) >> g0) & 1
                    want = int(ia[w, g0:g0 + sg].astype(object).sum()) % (1 << bits)
                    for l in range(g0, g0 + sg):
                        assert (got[l] is None) if not on else (got[l] % (1 << bits) == want), (op, label, w, l)
        _, masks, _, ia = ws.cases(op)[0]
        if sg == 8:  # eight different sums in one wave
            assert any(len({int(ia[w, g:g + 8].astype(object).sum()) for g in range(0, 64, 8)}) == 8 for w in range(len(ia)))
        if bits == 64:  # the carry between the two halves: the low words alone overflow 32 bits
            assert any(int((ia[w] & np.int64(0xffffffff)).astype(object).sum()) >= 1 << 32 for w in range(len(ia))) and (ia < 0).any() and (ia > 2 ** 32).any()


def _argbest(d, idx, order):
    """numpy's argmax / argmin over the lanes in index order: their first hit is the lowest index among equals"""
    by_index = np.argsort(idx, kind="stable")
    if order == "farthest":  # ties to the highest index: search from the top
        by_index = by_index[::-1]
    dd = d[by_index]
    return by_index[np.argmin(dd) if order == "nearest" else np.argmax(dd)]


def test_bests_are_argmax_with_the_stated_tie():
    for op in ws.BEST_OPS + ("MAX_F64",):
        sg = 8 if "BEST8" in op else 64
        order = "nearest" if "NEAREST" in op else "farthest" if "FARTHEST" in op else "max_first"
        for label, masks, a, ia in ws.cases(op):
            for w in range(len(a)):
                out, iout = st.probe(op, masks[w], a[w], ia[w])
                idx = np.array([st.as_i32(int(x)) for x in ia[w]])
                d = a[w] if op == "MAX_F64" else a[w].astype(np.float32).astype(np.float64)
                for g0 in range(0, 64, sg):
                    if not (int(masks[w]) >> g0) & 1:
                        assert out[g0] is None and iout[g0] is None
                        continue
                    k = g0 + _argbest(d[g0:g0 + sg], idx[g0:g0 + sg], order)
                    for l in range(g0, g0 + sg):  # every lane ends with the same pair, and its d is the winner's own bits
                        assert (out[l], iout[l]) == (st.f64_bits(d[k]), int(idx[k])), (op, label, w, l)


def test_tie_shapes_tell_first_from_last():
    d, idx = ws.tie_rows()
    signs = pairs8 = 0
    for w in range(len(d)):
        first = st.sg_best(list(d[w]), list(idx[w]), 64, "max_first")[0]
        last = st.sg_best(list(d[w]), list(idx[w]), 64, "farthest")[0]
        assert first[0] == last[0] and first[1] != last[1]  # the same d, another index: the tie rule alone decides
        for g in range(0, 64, 8):  # and so inside every sub-group of 8
            f8 = st.sg_best(list(d[w]), list(idx[w]), 8, "max_first")[g]
            l8 = st.sg_best(list(d[w]), list(idx[w]), 8, "farthest")[g]
            assert f8[0] == l8[0]
            pairs8 += f8[1] != l8[1]
        signs += math.copysign(1, first[0]) != math.copysign(1, last[0])
    assert pairs8 > 4 * len(d)  # more than half of the sub-groups hold a tie of their own (a single best in a row of the wave leaves seven without)
    assert signs >= 2  # +0 against -0: the returned bits are the winning lane's, and the two rules return different ones


def test_tree_sum_is_close_to_fsum_and_is_not_the_lane_order_sum():
    rows = ws.cancellation_rows()
    differ = 0
    for v in rows:
        tree = st.wave_sum_f64(v)
        assert len({st.f64_bits(x) for x in tree}) == 1
        assert abs(float(tree[0]) - math.fsum(v)) <= GAMMA7 * math.fsum(np.abs(v))
        differ += st.f64_bits(tree[0]) != st.f64_bits(st.lane_order_sum(v))
    assert differ > len(rows) // 2, differ  # the shape tells the tree from the sum in lane order on more than half of its waves
    # the association matters too: (r0 + r16) + (r32 + r48) gives other bits on some wave
    other = 0
    for v in rows:
        x = [np.float64(t) for t in v]
        for src in (st.src_xor1, st.src_xor2, st.src_half_mirror, st.src_row_mirror):
            x = [x[i] + x[src(i)] for i in range(64)]
        other += st.f64_bits((x[0] + x[16]) + (x[32] + x[48])) != st.f64_bits(st.wave_sum_f64(v)[0])
    assert other >= 4, other
    assert st.f64_bits(st.wave_sum_f64([-0.0] * 64)[0]) == st.f64_bits(-0.0) and st.f64_bits(st.wave_sum_f64([0.0] * 64)[0]) == 0


def test_wave_all_and_packed_min_max():
    _, masks, _, ia = ws.all_cases()[0]
    verdicts = set()
    for w in range(len(ia)):
        act = st.mask_to_act(masks[w])
        got = st.wave_all([x != 0 for x in ia[w]], act)
        want = bool(np.all(ia[w][np.array(act)] != 0))
        assert all((g is None) if not on else (g == want) for g, on in zip(got, act))
        verdicts.add((want, bool((ia[w] != 0).all())))
    assert verdicts == {(True, True), (True, False), (False, False)}  # a false lane that is off does not vote
    _, _, _, ia = ws.pk_cases()[0]
    a, b = (ia.view(np.uint64) & np.uint64(0xffffffff)).astype(np.uint32), (ia.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    for name, f in (("PK_MIN_U16", np.minimum), ("PK_MAX_U16", np.maximum)):
        want = f(a.view(np.uint16), b.view(np.uint16)).view(np.uint32)
        for w in range(len(ia)):
            got = st.probe(name, st.M64, np.zeros(64), ia[w])[1]
            assert got == [int(x) for x in want[w]]
    lo, hi = np.minimum(a, b), np.maximum(a, b)  # the packed result is not the word-wise one on these inputs
    assert (np.minimum(a.view(np.uint16), b.view(np.uint16)).view(np.uint32) != lo).any() and (np.maximum(a.view(np.uint16), b.view(np.uint16)).view(np.uint32) != hi).any()
