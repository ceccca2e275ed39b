// ctag_fit_solve.h -- the damped solve of a fit's reduced system, one block per group (k_rig_fit.hip: a rig's member transforms, at
// most 96 rows; k_cam_fit.hip: a camera set's poses, at most 48 rows): the packed lower triangle of S + lambda diag S in LDS,
// right-looking Cholesky, the dropped slot (the anchor's) as identity rows with a zero right-hand side, the two triangular solves,
// delta and a flag for a pivot that is not positive.  The arithmetic does not depend on STRIDE: a group's result is the same bytes
// under any stride that holds it.
#pragma once
#include <hip/hip_runtime.h>

#include "ctag_linalg.h"
#include "ctag_math.h"

namespace ctag {

constexpr int kFitSolveThreads = 256;

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
