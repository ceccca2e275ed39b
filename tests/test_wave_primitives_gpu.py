"""Every value-returning primitive of cylindertag_amd/csrc/ctag_wave.h by itself on the device (ctag_testkit_wave_probe), at every instantiation the
product uses, against the plain statement of tests/wave_statement.py on the shapes of tests/wave_shapes.py -- in blocks of 64 threads and in blocks
of 256, whose waves 1-3 have other thread indices than lanes.  tests/test_wave_statement_cpu.py holds the statement to numpy and shows that the
shapes discriminate.  The ordering points (lds_barrier, lds_wait, wave_fence, vmem_wait) return nothing and are not probed."""
import math

import numpy as np
import pytest

import testkit as tk
import wave_shapes as ws
import wave_statement as st
from cylindertag_amd.capi import CtagError

pytestmark = pytest.mark.gpu
BLOCKS = (64, 256)
GAMMA7 = 7 * 2.0 ** -53 / (1 - 7 * 2.0 ** -53)


def _run(det, op, block):
    """The probe on every case of `op` -> per case (label, masks, a, ia, out, iout)"""
    got = []
    for label, masks, a, ia in ws.cases(op):
        out, iout = det.wave(getattr(tk, "WAVE_" + op), masks, a, ia, block_threads=block)
        got.append((label, masks, a, ia, out, iout))
    return got


def _hold_to_statement(det, op, block):
    for label, masks, a, ia, out, iout in _run(det, op, block):
        obits = out.view(np.uint64)
        for w in range(len(masks)):
            want_o, want_i = st.probe(op, masks[w], a[w], ia[w])
            for l in range(64):
                where = "%s, %s, block %d, wave %d lane %d" % (op, label, block, w, l)
                if not (int(masks[w]) >> l) & 1:  # a lane that was off: nothing but the sentinels
                    assert out[w, l] == tk.WAVE_SENTINEL_F64 and int(iout[w, l]) == tk.WAVE_SENTINEL_I64, where
                    continue
                if want_o[l] is not None:
                    assert int(obits[w, l]) == want_o[l], "%s: %r, stated %r" % (where, out[w, l], st.bits_f64(want_o[l]))
                if want_i[l] is not None:
                    assert int(iout[w, l]) == want_i[l], "%s: %#x, stated %#x" % (where, int(iout[w, l]), want_i[l])


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op", ["FROM_PREV", "FROM_NEXT"])
def test_wave_from_prev_and_next(detector, op, block):
    """lane i <- lane i -+ 1 across the whole wave; lane 0 / lane 63, and a lane whose source is off, get 0"""
    _hold_to_statement(detector, op, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op", ["SHR1_I32", "SHR2_I32", "SHR4_I32", "SHR1_F32", "SHR1_F64"])
def test_dpp_shr(detector, op, block):
    """lane i <- lane i - D within its row of 16; the int, float and double forms of sg_expand_line: both halves of a double move"""
    _hold_to_statement(detector, op, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op", [o for o in ws.MOVE_OPS if "XOR" in o or "MIRROR" in o])
def test_dpp_mov(detector, op, block):
    """kDppXor1, kDppXor2, kDppHalfMirror, kDppRowMirror on int and long long"""
    _hold_to_statement(detector, op, block)


@pytest.mark.parametrize("block", BLOCKS)
def test_wave_incl_scan(detector, block):
    """ones, a single 1 at every row edge (the carries of row_bcast:15 and row_bcast:31), random int32 and sums that wrap, modulo 2^32"""
    _hold_to_statement(detector, "INCL_SCAN", block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op", ws.SUM_OPS)
def test_sg_sum(detector, op, block):
    """sg_sum<8> and sg_sum<64> on int and long long: eight sums a wave, the carry between a long long's halves, whole sub-groups off"""
    _hold_to_statement(detector, op, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op", ws.BEST_OPS)
def test_sg_best(detector, op, block):
    """The two orders of k_quad.hip (nearest, ties to the first index; farthest, ties to the last) over 8 lanes and over the wave: the tie rule
    alone, winners at the edges, equal bests across rows and quads, -inf, +0 / -0; and every lane of a sub-group ends with the same pair."""
    _hold_to_statement(detector, op, block)
    for label, masks, a, ia, out, iout in _run(detector, op, block):
        sg = 8 if "BEST8" in op else 64
        for w in range(len(masks)):
            for g0 in range(0, 64, sg):
                if (int(masks[w]) >> g0) & 1:
                    assert len(set(out[w, g0:g0 + sg].view(np.uint64))) == 1 and len(set(iout[w, g0:g0 + sg])) == 1, (op, label, w, g0)


@pytest.mark.parametrize("block", BLOCKS)
def test_wave_max_f64(detector, block):
    """The largest d and the LOWEST index among equal d, the winner's own bits (+0 / -0), the same pair in all 64 lanes"""
    _hold_to_statement(detector, "MAX_F64", block)
    for label, masks, a, ia, out, iout in _run(detector, "MAX_F64", block):
        for w in range(len(masks)):
            assert len(set(out[w].view(np.uint64))) == 1 and len(set(iout[w])) == 1, (label, w)
            idx = np.array([st.as_i32(int(x)) for x in ia[w]])
            assert out[w, 0] == a[w].max() and int(iout[w, 0]) == idx[a[w] == a[w].max()].min(), (label, w)


@pytest.mark.parametrize("block", BLOCKS)
def test_wave_sum_f64(detector, block):
    """The bits of the stated tree -- not of the sum in lane order -- in all 64 lanes; within gamma_7 sum |v| of the exact sum (a value passes through
    at most seven additions); all -0.0 gives -0.0."""
    _hold_to_statement(detector, "SUM_F64", block)
    (label, masks, a, ia, out, iout), = _run(detector, "SUM_F64", block)
    differ = 0
    for w in range(len(a)):
        assert len(set(out[w].view(np.uint64))) == 1, w
        assert abs(out[w, 0] - math.fsum(a[w])) <= GAMMA7 * math.fsum(np.abs(a[w])), w
        differ += st.f64_bits(out[w, 0]) != st.f64_bits(st.lane_order_sum(a[w]))
    assert differ > 16  # (tests/test_wave_statement_cpu.py: the cancellation shape tells the two sums apart)
    minus = [w for w in range(len(a)) if (a[w].view(np.uint64) == np.uint64(1 << 63)).all()]
    assert minus and all(st.f64_bits(out[w, 0]) == 1 << 63 for w in minus)


@pytest.mark.parametrize("block", BLOCKS)
def test_wave_all(detector, block):
    """All true; one false lane at 0, 31, 32, 63; the false lane off (true: it does not vote); every active lane gets the same answer"""
    _hold_to_statement(detector, "ALL", block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op", ws.PK_OPS)
def test_pk_min_max_u16(detector, op, block):
    """pk_min_u16 / pk_max_u16: halves that order differently (0x0001ffff against 0xffff0001), equal halves, 0 and 0xffff"""
    _hold_to_statement(detector, op, block)


def test_wave_probe_refuses_masks_outside_the_contract(detector):
    """The whole-wave forms read lanes 0, 16, 32 and 48 with v_readlane, which returns a masked-off lane's stale register: the probe refuses a mask
    that is not all ones for them, and a split sub-group for the 8-lane forms, so that no test reads an undefined value."""
    part = np.array([0xffffffffffffff00], np.uint64)
    for op in ("SG_SUM64_I32", "SG_SUM64_I64", "SG_BEST64_NEAREST", "SG_BEST64_FARTHEST", "SUM_F64", "MAX_F64", "INCL_SCAN"):
        with pytest.raises(CtagError) as e:
            detector.wave(getattr(tk, "WAVE_" + op), part)
        assert e.value.status == -1, op  # CTAG_ERR_ARG
    split = np.array([0xfffffffffffffffe], np.uint64)
    for op in ("SG_SUM8_I32", "SG_SUM8_I64", "SG_BEST8_NEAREST", "SG_BEST8_FARTHEST"):
        with pytest.raises(CtagError) as e:
            detector.wave(getattr(tk, "WAVE_" + op), split)
        assert e.value.status == -1, op
        detector.wave(getattr(tk, "WAVE_" + op), part)  # a whole sub-group off is within the contract
    for bad in (dict(block_threads=128), dict(block_threads=0)):
        with pytest.raises(CtagError):
            detector.wave(tk.WAVE_ALL, part, **bad)
    with pytest.raises(CtagError):
        detector.wave(len(tk.WAVE_OPS), part)
