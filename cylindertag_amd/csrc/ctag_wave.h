// ctag_wave.h -- what the kernels say to the wave itself, each stated once: the ordering points that are cheaper than __syncthreads(), the vote, the DPP lane moves
// and the reductions / scans built from them, and the packed 16-bit min / max.  Device only (gfx9, 64-wide wavefronts); every function is one or a few
// instructions and is inlined.
//
// Lanes that are off (EXEC) where a primitive is called -- they left a loop, or sit in the other side of a divergent branch.  Each primitive below says which
// of three rules it follows; tests/test_wave_primitives_gpu.py holds each one by itself to tests/wave_statement.py under these rules, and
// ctag_testkit_wave_probe refuses the masks a rule excludes:
//   [any mask]     any lanes may be off.  A lane move reads a source that is off as NO source: the reader gets 0, as at the edge of a row (the instruction's
//                  `old` operand is 0 and a disabled source leaves it in place).  Lanes that are off get nothing and cost nothing.
//   [sub-groups]   every 8-lane sub-group (lanes 8g .. 8g+7) is on or off AS A WHOLE, the caller's duty: the steps read lane ^ 1, lane ^ 2 and lane 7 - i of the
//                  sub-group only, so a sub-group that is on never reads one that is off.  With a sub-group split, a lane that is off counts as 0 in
//                  SOME of the partial results -- not a sum or a best of anything.
//   [all 64]       every lane of the wave is on, the caller's duty: the rows are combined with v_readlane of lanes 0, 16, 32 and 48, which returns a
//                  lane's register whether the lane is on or not -- a stale value -- and the scan's carries come from lanes 15 and 31.  Call these from
//                  wave-uniform control flow only: never inside a branch on a per-lane value, nor in a loop whose trip count differs between lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__) && defined(__GFX9__) && defined(__AMDGCN_WAVEFRONT_SIZE__) && __AMDGCN_WAVEFRONT_SIZE__ != 64
#error "ctag_wave.h assumes 64-wide wavefronts"
#endif

namespace ctag {

// ---- ordering points ----------------------------------------------------------------------------------------------------------------------------
// Block barrier between phases that exchange data through LDS ONLY.  Waits for the wave's LDS traffic (lgkmcnt), then s_barrier; it does NOT wait for
// vector memory (vmcnt), which __syncthreads() does -- that would drain, at every phase boundary, the prefetch loads and the stores the block has in flight
// (the vector-memory counter counts stores on gfx9).  The caller guarantees that no phase hands data to another thread of the block through GLOBAL memory;
// a value a thread loaded itself is waited for where it is used, as always.  (tests/test_variant_builds_gpu.py holds edgeRefine's use of it against a build
// with plain barriers, EXTRA=-DCTAG_REFINE_PLAIN_SYNC=1.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// The same wait without the barrier, for phases of ONE wave: LDS serves a wave's accesses in order, so once the wave's LDS traffic is done its lanes see each
// other's writes.  Not for vector memory either (the rows or quads requested ahead stay in flight).  The caller guarantees that the threads exchanging data
// are one wavefront -- a block of more than 64 threads would race silently -- and that the exchange is through LDS only.
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// Ordering point for lanes of one wave that run in LOCKSTEP (the 8-lane sub-groups of k_quad_edges_packed, k_markers' wave 0): no instruction is issued and
// nothing is waited for -- neither LDS nor vector memory; it only stops the compiler from moving memory accesses across it.  The caller guarantees that
// producer and consumer lanes are in the same wave and not in divergent branches of it.
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"), __builtin_amdgcn_wave_barrier(); }
// Wait for every vector-memory access the wave has issued (vmcnt(0)) and for nothing else: placed by hand where the compiler's own wait would come later
// and in a worse place (k_edge_refine_sums).
__device__ __forceinline__ void vmem_wait() { __builtin_amdgcn_s_waitcnt(0x0f70); }

// ---- votes ----------------------------------------------------------------------------------------------------------------------------------------------
// True when `p` holds on EVERY ACTIVE lane of the wave: one v_cmp into a scalar pair (the ballot of !p has no bit set) and a scalar compare, so a branch on
// it is a scalar branch -- the whole wave takes one side.  Nothing is waited for.  Lanes that are inactive where it is called -- they left the loop, or sit in
// the other side of a divergent branch -- do not vote: a ballot carries no bit for them.  With no lane active it is true.  [any mask]; every lane that is
// on gets the same answer.
__device__ __forceinline__ bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }

// ---- DPP lane moves: a v_mov_b32 with a data-parallel-primitive control, one vector instruction, no LDS crossbar round trip -----------------------
// (A __shfl is a ds_bpermute_b32: address arithmetic, the instruction and ~100 cycles before the value can be used.)
constexpr int kDppXor1 = 0xB1;          // quad_perm [1,0,3,2]: lane i <- lane i ^ 1
constexpr int kDppXor2 = 0x4E;          // quad_perm [2,3,0,1]: lane i <- lane i ^ 2
constexpr int kDppRowShr = 0x110;       // + D (1..15), row_shr:D: lane i <- lane i - D within its row of 16 lanes
constexpr int kDppWaveShl1 = 0x130;     // wave_shl:1: lane i <- lane i + 1 across the whole wave
constexpr int kDppWaveShr1 = 0x138;     // wave_shr:1: lane i <- lane i - 1 across the whole wave
constexpr int kDppRowMirror = 0x140;    // row_mirror: lane i <- lane 15 - i of its row
constexpr int kDppHalfMirror = 0x141;   // row_half_mirror: lane i <- lane 7 - i of its half row
constexpr int kDppRowBcast15 = 0x142;   // row_bcast:15: lane 15 of every row to the row behind it
constexpr int kDppRowBcast31 = 0x143;   // row_bcast:31: lane 31 to rows 2 and 3
// The one call: lanes of the rows in ROW_MASK take their source lane's `v`; a lane without a source (and every lane of a row not in the mask) gets 0.
// [any mask]: so does a lane whose source lane is off.  A 64-bit value (long long, double) moves as its two halves, each by the same rule.
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, BOUND_CTRL); }
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) { return __int_as_float(dpp_mov<CTRL>(__float_as_int(v))); }
template <int CTRL>
__device__ __forceinline__ long long dpp_mov(long long v) {
    const unsigned lo = (unsigned)dpp_mov<CTRL>((int)(unsigned)((unsigned long long)v & 0xffffffffull)), hi = (unsigned)dpp_mov<CTRL>((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)((unsigned long long)lo | ((unsigned long long)hi << 32));
}
// lane i <- lane i - 1 / lane i + 1 across the whole wave; lane 0 / lane 63 get 0  [any mask]
__device__ __forceinline__ uint32_t wave_from_prev(uint32_t v) { return (uint32_t)dpp_mov<kDppWaveShr1>((int)v); }
__device__ __forceinline__ uint32_t wave_from_next(uint32_t v) { return (uint32_t)dpp_mov<kDppWaveShl1>((int)v); }
// lane i <- lane i - D within its row of 16 lanes; lanes without a source get 0.  The 8-lane sub-groups are halves of such rows: the lanes that would read
// across a sub-group's edge are the ones that ignore the value.  [any mask]: sg_expand_line calls it with whole sub-groups off, and lane 8g then reads 0 or
// the value of lane 8g - 1 -- it is the lane that ignores what it read (step 0 takes the committed prefix's line).
template <int D>
__device__ __forceinline__ int dpp_shr(int v) { return dpp_mov<kDppRowShr + D>(v); }
template <int D>
__device__ __forceinline__ double dpp_shr(double v) { return __hiloint2double(dpp_shr<D>(__double2hiint(v)), dpp_shr<D>(__double2loint(v))); }
template <int D>
__device__ __forceinline__ float dpp_shr(float v) { return __int_as_float(dpp_shr<D>(__float_as_int(v))); }
__device__ __forceinline__ long long readlane_ll(long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v & 0xffffffffull), l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
    return (long long)((unsigned long long)lo | ((unsigned long long)hi << 32));
}
// Inclusive scan (sum) over the wave: shifts by 1, 2, 4, 8 inside the rows of 16 lanes (a lane without a source adds 0), then lane 15 of every even row into
// the odd row behind it and lane 31 into rows 2 and 3 -- six vector instructions instead of six ds_bpermute round trips.  The sum is modulo 2^32.
// [all 64]: a lane that is off adds 0 AND cuts the chain of partial sums that pass through it.
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += dpp_mov<kDppRowShr + 1, 0xf, true>(v);
    v += dpp_mov<kDppRowShr + 2, 0xf, true>(v);
    v += dpp_mov<kDppRowShr + 4, 0xf, true>(v);
    v += dpp_mov<kDppRowShr + 8, 0xf, true>(v);
    v += dpp_mov<kDppRowBcast15, 0xa>(v);  // into rows 1 and 3
    v += dpp_mov<kDppRowBcast31, 0xc>(v);  // into rows 2 and 3
    return v;
}
// All-reduce over a sub-group of 8 lanes or over the wave: lane ^ 1 and lane ^ 2 by quad permutes, the other quad of the 8 lanes by row_half_mirror, the
// other half of a row of 16 by row_mirror, and the wave's four rows by four v_readlane.  The operations are exact (integer sums) or a total order (best
// distance, ties by index), so the order of combination does not matter.  (As __shfl_xor a wave's reduction has six ds_bpermute steps; the split loop of the
// RDP runs one per round.)
// sg_sum<8>, sg_best<8>: [sub-groups] -- k_quad_edges_packed's sub-groups leave its loops one by one.  sg_sum<64>, sg_best<64>: [all 64].  Integer sums are
// modulo 2^32 / 2^64.  sg_best: `better` is a strict total order on the pairs that occur (distinct indices); d is never NaN -- a NaN compares false either
// way and the lanes of a sub-group would end with different pairs: out of contract.  -0 and +0 are EQUAL d: the index decides, and the d that comes back is
// the winning lane's own, sign included.
template <int SG, class T>
__device__ __forceinline__ T sg_sum(T v) {  // T: int, long long
    v += dpp_mov<kDppXor1>(v);
    v += dpp_mov<kDppXor2>(v);
    v += dpp_mov<kDppHalfMirror>(v);
    if constexpr (SG == 64) {
        v += dpp_mov<kDppRowMirror>(v);
        if constexpr (sizeof(T) == 8) v = (T)(readlane_ll((long long)v, 0) + readlane_ll((long long)v, 16) + readlane_ll((long long)v, 32) + readlane_ll((long long)v, 48));
        else v = (T)(__builtin_amdgcn_readlane((int)v, 0) + __builtin_amdgcn_readlane((int)v, 16) + __builtin_amdgcn_readlane((int)v, 32) + __builtin_amdgcn_readlane((int)v, 48));
    }
    return v;
}
// the best (d, i) pair of the sub-group under `better(od, oi, d, i)` ("the other pair beats mine"): every lane ends with the same pair
template <int SG, class Better>
__device__ __forceinline__ void sg_best(float& bd, int& bi, Better better) {
    auto step = [&](float od, int oi) {
        if (better(od, oi, bd, bi)) {
            bd = od;
            bi = oi;
        }
    };
    step(dpp_mov<kDppXor1>(bd), dpp_mov<kDppXor1>(bi));
    step(dpp_mov<kDppXor2>(bd), dpp_mov<kDppXor2>(bi));
    step(dpp_mov<kDppHalfMirror>(bd), dpp_mov<kDppHalfMirror>(bi));
    if constexpr (SG == 64) {
        step(dpp_mov<kDppRowMirror>(bd), dpp_mov<kDppRowMirror>(bi));
        float rd[4];
        int ri[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            rd[r] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bd), 16 * r));
            ri[r] = __builtin_amdgcn_readlane(bi, 16 * r);
        }
        bd = rd[0];
        bi = ri[0];
#pragma unroll
        for (int r = 1; r < 4; r++) step(rd[r], ri[r]);
    }
}

// FP64 over the wave (k_pose_cov.hip).  A double moves as its two halves.  The sum is one fixed tree -- lane ^ 1, lane ^ 2, the other quad of 8, the other
// half of the row, then the four rows' values added in row order -- and every step adds the same two numbers in both lanes of a pair, so all 64 lanes end
// with the same bits, and the same inputs give the same bits wherever the wave runs.  It is NOT the sum in lane order.  A value passes through at most seven
// additions, so |result - exact sum| <= gamma_7 sum |v|, gamma_7 = 7u / (1 - 7u), u = 2^-53.  All -0.0 gives -0.0.  wave_sum_f64, wave_max_f64: [all 64] --
// a lane without a point adds 0.0 / offers (-1, INT_MAX), it does not leave.
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) { return __hiloint2double(dpp_mov<CTRL>(__double2hiint(v)), dpp_mov<CTRL>(__double2loint(v))); }
__device__ __forceinline__ double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_mov<kDppXor1>(v);
    v += dpp_mov<kDppXor2>(v);
    v += dpp_mov<kDppHalfMirror>(v);
    v += dpp_mov<kDppRowMirror>(v);
    return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}
// the largest d of the wave and its index, the lowest index among equal d (a total order: the tree's shape does not matter); every lane ends with the pair.
// NaN is out of contract (as for sg_best); -0 and +0 are equal d, and the d returned is the winning lane's own.
__device__ __forceinline__ void wave_max_f64(double& bd, int& bi) {
    auto step = [&](double od, int oi) {
        if (od > bd || (od == bd && oi < bi)) {
            bd = od;
            bi = oi;
        }
    };
    step(dpp_mov<kDppXor1>(bd), dpp_mov<kDppXor1>(bi));
    step(dpp_mov<kDppXor2>(bd), dpp_mov<kDppXor2>(bi));
    step(dpp_mov<kDppHalfMirror>(bd), dpp_mov<kDppHalfMirror>(bi));
    step(dpp_mov<kDppRowMirror>(bd), dpp_mov<kDppRowMirror>(bi));
    double rd[4];
    int ri[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        rd[r] = readlane_f64(bd, 16 * r);
        ri[r] = __builtin_amdgcn_readlane(bi, 16 * r);
    }
    bd = rd[0];
    bi = ri[0];
#pragma unroll
    for (int r = 1; r < 4; r++) step(rd[r], ri[r]);
}

// ---- packed 16-bit min / max (v_pk_min_u16 / v_pk_max_u16) on the two halves of a word: each half by itself, unsigned; no other lane is read ----------
typedef unsigned short ctag_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ctag_us2 as_us2(uint32_t a) { return __builtin_bit_cast(ctag_us2, a); }
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(as_us2(a), as_us2(b))); }
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(as_us2(a), as_us2(b))); }

}  // namespace ctag
