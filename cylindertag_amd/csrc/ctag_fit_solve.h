// ctag_fit_solve.h -- the two kernels behind the reduced system of a fit whose unknowns are 6-parameter slots (k_rig_fit.hip: a rig's
// member transforms, at most 96 rows, a group per rig; k_cam_fit.hip: a camera set's poses, at most 48 rows, one group).
// k_fit_assemble adds the slot blocks (ctag_schur6.h) a pass of records left in the workspace to S and g; k_fit_solve is the damped
// solve, one block per group: the packed lower triangle of S + lambda diag S in LDS,
// right-looking Cholesky, the dropped slot (the anchor's) as identity rows with a zero right-hand side, the two triangular solves,
// delta and a flag for a pivot that is not positive.  The arithmetic of neither depends on STRIDE: a group's result is the same bytes
// under any stride that holds it.
// Not here, on purpose: k_mfit_assemble and k_mfit_solve (k_model_fit.hip: 3x3 blocks of 27 doubles, a model's own system), and
// k_ifit_solve (k_intr_fit.hip): a 16 x 16 whose two triangular solves run row by row on lane 0, while k_fit_solve's run column by
// column -- the two subtract in a different order per element, so one kernel for both would change the intrinsics fit's bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "ctag_linalg.h"
#include "ctag_math.h"
#include "ctag_schur6.h"

namespace ctag {

constexpr int kFitSolveThreads = 256;
constexpr int kFitAssembleThreads = 256;

// Adds records r0 .. r1-1 to S and g of group slot_of.group().  Thread t < STRIDE x STRIDE: entry (i, j) = (t / STRIDE, t % STRIDE) of S,
// the threads with i <= j work and write both triangles; STRIDE x STRIDE <= t < STRIDE x STRIDE + STRIDE: entry t - STRIDE x STRIDE
// of g.  S: [n_groups][STRIDE][STRIDE], g: [n_groups][STRIDE]; slot a of the group owns rows 6a .. 6a + 5.  A record's workspace
// holds STRIDE / 6 slot blocks; slot_of(r, a, b, ka, kb) gives the ones of slots a and b of the group in record r, or is false when
// the record has not both (an entry of g asks with b = a); slot_of.group() is the group the block works for: blockIdx.y of a grid
// with a row of blocks per group, or plainly 0 for a fit of one group -- with the group's offsets read from blockIdx.y the one-group
// instance measured 1.4 % slower per record than with the constant (3.004 against 2.956 ms over a camera set fit of 572 records).
// The records are walked in record order and the running sums live in global memory between the passes.
template <int STRIDE, class SlotOf>
__global__ __launch_bounds__(kFitAssembleThreads) void k_fit_assemble(const double* __restrict__ ws, SlotOf slot_of, const int32_t* __restrict__ flags, int r0, int r1,
                                                                        double* __restrict__ S, double* __restrict__ g) {
    const int grp = slot_of.group();
    const int t = blockIdx.x * kFitAssembleThreads + threadIdx.x;
    constexpr int NN = STRIDE * STRIDE, SLOTS = STRIDE / 6;
    const int i = t < NN ? t / STRIDE : t - NN, j = t < NN ? t - i * STRIDE : 0;
    const bool is_s = t < NN && i <= j, is_g = t >= NN && t < NN + STRIDE;
    if (!is_s && !is_g) return;
    const int a = i / 6, p = i - 6 * a, bs = j / 6, q = j - 6 * bs;
    double* dst = is_s ? S + (size_t)grp * NN + (size_t)i * STRIDE + j : g + (size_t)grp * STRIDE + i;
    double acc = *dst;
    int ea = 0;  // index of (p, q) in the upper triangle's row order
    if (is_s && a == bs) ea = p * 6 - p * (p - 1) / 2 + (q - p);
    const int b = is_g ? a : bs;
    for (int r = r0; r < r1; r++) {
        int ka, kb;
        if (flags[r] != 0 || !slot_of(r, a, b, ka, kb)) continue;
        const double* za = ws + ((size_t)(r - r0) * SLOTS + ka) * kSlotDoubles;
        if (is_g) {
            acc += za[kSlotG + p];
            continue;
        }
        const double* zb = ws + ((size_t)(r - r0) * SLOTS + kb) * kSlotDoubles;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += za[kSlotZ + k * 6 + p] * zb[kSlotZ + k * 6 + q];
        acc -= s;
        if (a == bs) acc += za[kSlotA + ea];
    }
    *dst = acc;
    if (is_s && i != j) S[(size_t)grp * NN + (size_t)j * STRIDE + i] = acc;
}

// the blocks of a k_fit_assemble launch along x
template <int STRIDE>
constexpr int fit_assemble_blocks() { return (STRIDE * STRIDE + STRIDE + kFitAssembleThreads - 1) / kFitAssembleThreads; }

// (S + lambda diag S) delta = -g of group blockIdx.x by Cholesky over its first N = 6 n_slots[group] rows, the rows of slot
// drop[group] as identity rows with a zero right-hand side.  bad[group] = 1 and delta = 0 for a pivot that is not positive.
// STRIDE: the row stride of S, g and delta, 6 x the most slots a group can have.
template <int STRIDE>
__global__ __launch_bounds__(kFitSolveThreads) void k_fit_solve(const double* __restrict__ S, const double* __restrict__ g, const int32_t* __restrict__ n_slots,
                                                                  const int32_t* __restrict__ drop, const double* __restrict__ lambda,
                                                                  const int32_t* __restrict__ active, double* __restrict__ delta, int32_t* __restrict__ bad) {
    __shared__ double A[STRIDE * (STRIDE + 1) / 2], rhs[STRIDE], z[STRIDE], diag[STRIDE];
    const int grp = blockIdx.x, tid = threadIdx.x;
    if (!active[grp]) return;  // block-uniform
    const int N = 6 * min(max(n_slots[grp], 0), STRIDE / 6), dr = drop[grp];
    const double* Sm = S + (size_t)grp * STRIDE * STRIDE;
    const double lam = lambda[grp];
    auto at = [](int i, int k) { return i * (i + 1) / 2 + k; };  // k <= i
    for (int e = tid; e < N * N; e += kFitSolveThreads) {
        const int i = e / N, k = e - i * N;
        if (k > i) continue;
        double v;
        if (i / 6 == dr || k / 6 == dr) v = i == k ? 1.0 : 0.0;
        else {
            v = Sm[(size_t)i * STRIDE + k];
            if (i == k) v += lam * v;
        }
        A[at(i, k)] = v;
    }
    for (int i = tid; i < N; i += kFitSolveThreads) rhs[i] = i / 6 == dr ? 0.0 : -g[(size_t)grp * STRIDE + i];
    __syncthreads();
    bool ok = true;
    for (int j = 0; j < N; j++) {
        const double d = A[at(j, j)];           // written before the last barrier; not written again
        if (!(d > 0.0) || !ctl::finite64(d)) {  // the same in every thread
            ok = false;
            break;
        }
        const double sd = ctm::sqrt64(d);
        if (tid == 0) diag[j] = sd;
        for (int i = j + 1 + tid; i < N; i += kFitSolveThreads) A[at(i, j)] /= sd;
        __syncthreads();
        for (int i = j + 1 + (tid >> 4); i < N; i += kFitSolveThreads / 16) {  // row i of the trailing block, 16 threads along the row
            const double lij = A[at(i, j)];
            for (int k = j + 1 + (tid & 15); k <= i; k += 16) A[at(i, k)] -= lij * A[at(k, j)];
        }
        __syncthreads();
    }
    if (!ok) {
        for (int i = tid; i < STRIDE; i += kFitSolveThreads) delta[(size_t)grp * STRIDE + i] = 0.0;
        if (tid == 0) bad[grp] = 1;
        return;
    }
    for (int j = 0; j < N; j++) {  // L z = rhs, column by column
        const double zj = rhs[j] / diag[j];
        __syncthreads();  // every thread has read rhs[j]
        if (tid == 0) z[j] = zj;
        for (int i = j + 1 + tid; i < N; i += kFitSolveThreads) rhs[i] -= A[at(i, j)] * zj;
        __syncthreads();
    }
    for (int j = N - 1; j >= 0; j--) {  // L^T delta = z, row j of L is column j of L^T
        const double dj = z[j] / diag[j];
        __syncthreads();
        if (tid == 0) rhs[j] = dj;
        for (int k = tid; k < j; k += kFitSolveThreads) z[k] -= A[at(j, k)] * dj;
        __syncthreads();
    }
    for (int i = tid; i < STRIDE; i += kFitSolveThreads) delta[(size_t)grp * STRIDE + i] = (i < N && i / 6 != dr) ? rhs[i] : 0.0;
    if (tid == 0) bad[grp] = 0;
}

}  // namespace ctag
