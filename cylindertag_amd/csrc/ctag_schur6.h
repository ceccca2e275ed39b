// ctag_schur6.h -- the 6x6 pose block of a Schur complement, as the record kernels that eliminate a record's pose use it
// (k_model_fit.hip: corners against marker poses; k_rig_fit.hip: member transforms against rig poses; k_cam_fit.hip: camera poses
// against multi-view rig poses; k_intr_fit.hip: a camera's intrinsics against its view poses, which sums U in LDS and takes chol6,
// forward6 and forward6_dot from here): the sums of U = sum Jp^T Jp
// and sum Jp^T r over a record's points (k_pose_cov.hip sums the same U), U = L L^T, y = L^-1 sum Jp^T r, a column through L^-1 and
// the point Jacobian.  Every accumulator sees its additions in the order written here: the fits' results are held byte for byte.
#pragma once
#include <hip/hip_runtime.h>

#include "ctag_linalg.h"
#include "ctag_math.h"
#include "ctag_wave.h"

namespace ctag {

constexpr int kRecLeftOut = 1;   // flags of a record: it is not an observation / does not describe its detection record
constexpr int kRecSingular = 2;  // flags of a record: its U has a pivot that is not positive at this state

// H (the 21 upper entries of a symmetric 6x6, in row order) += j0 j0^T + j1 j1^T
__device__ __forceinline__ void gram6_add(const double* j0, const double* j1, double* H) {
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = a; c < 6; c++) {
            H[e] += j0[a] * j0[c];
            H[e] += j1[a] * j1[c];
            e++;
        }
}

// b += j0 q0 + j1 q1
__device__ __forceinline__ void grad6_add(const double* j0, const double* j1, double q0, double q1, double* b) {
#pragma unroll
    for (int a = 0; a < 6; a++) {
        b[a] += j0[a] * q0;
        b[a] += j1[a] * q1;
    }
}

// U = L L^T of a symmetric 6x6 given as its 21 upper entries in row order; false on a pivot that is not positive (or not a number)
__device__ __forceinline__ bool chol6(const double* H, double* L) {
    double U[36];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) {
            U[a * 6 + b] = H[e];
            U[b * 6 + a] = H[e];
            e++;
        }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = U[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0.0) || !ctl::finite64(d)) ok = false;
        d = ctm::sqrt64(d);
        L[j * 6 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = U[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = s / d;
        }
    }
    return ok;
}

// x <- L^-1 x (forward substitution, lower triangle of the row-major 6x6 L)
__device__ __forceinline__ void forward6(const double* L, double* x) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i * 6 + k] * x[k];
        x[i] = s / L[i * 6 + i];
    }
}

// The pose block of a record from every lane's share of H (gram6_add) and b (grad6_add): the 21 + 6 sums over the wave, U = L L^T
// and, when every pivot is positive, b <- y = L^-1 b.  Returns that verdict, the same in every lane.
__device__ __forceinline__ bool pose_block6(double* H, double* b, double* L) {
#pragma unroll
    for (int e = 0; e < 21; e++) H[e] = wave_sum_f64(H[e]);
#pragma unroll
    for (int a = 0; a < 6; a++) b[a] = wave_sum_f64(b[a]);
    const bool pd = chol6(H, L);
    if (pd) forward6(L, b);
    return pd;
}

// z <- L^-1 z, one column of Z = L^-1 (Jp^T J); returns z . y, what the column takes from the reduced right-hand side
__device__ __forceinline__ double forward6_dot(const double* L, double* z, const double* y) {
    forward6(L, z);
    double zy = 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) zy += z[a] * y[a];
    return zy;
}

// d residual / d X = (a0 R0 - b0 R2, a1 R1 - b1 R2) with the a0, b0, a1, b1 of point_residual: j0[3] = a0, j0[5] = -b0, j1[4] = a1, j1[5] = -b1
__device__ __forceinline__ void point_dX(const double* R, const double* j0, const double* j1, double* x0, double* x1) {
#pragma unroll
    for (int m = 0; m < 3; m++) {
        x0[m] = j0[3] * R[m] + j0[5] * R[6 + m];
        x1[m] = j1[4] * R[3 + m] + j1[5] * R[6 + m];
    }
}

}  // namespace ctag
