// ctag_schur6.h -- the 6x6 pose block of a Schur complement, as the record kernels that eliminate a record's pose use it
// (k_model_fit.hip: corners against marker poses; k_rig_fit.hip: member transforms against rig poses; k_cam_fit.hip: camera poses
// against multi-view rig poses; k_intr_fit.hip: a camera's intrinsics against its view poses, which sums U in LDS and takes chol6,
// forward6, backward6 and forward6_dot from here): the sums of U = sum Jp^T Jp
// and sum Jp^T r over a record's points (k_pose_cov.hip sums the same U), U = L L^T, y = L^-1 sum Jp^T r, a column through L^-1, the
// point Jacobian, and the slot block: the 63 doubles a record leaves per 6-parameter slot (a member of a rig, a camera of a set), as
// k_rfit_record and k_cfit_record write it and k_fit_assemble (ctag_fit_solve.h) reads it.
// Every accumulator sees its additions in the order written here: the fits' results are held byte for byte.
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

// x <- L^-T x (back substitution with the transpose of the lower triangle of the row-major 6x6 L)
__device__ __forceinline__ void backward6(const double* L, double* x) {
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[k * 6 + i] * x[k];
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

// ---- the slot block: what a record leaves for one 6-parameter slot s with Jacobian rows Js of its points.  kSlotDoubles doubles:
// Z = L^-1 (Jp^T Js) row-major at kSlotZ, the 21 upper entries of Js^T Js in row order at kSlotA, g = Js^T r - Z^T y at kSlotG.
constexpr int kSlotZ = 0, kSlotA = 36, kSlotG = 57, kSlotDoubles = 63;

// The rows (m0, m1) of Js = (dr/dQ) [-[Q]x | I] for a slot that moves the point Q rigidly; x0, x1 are the rows of dr/dQ.  The rotation
// columns are Q x (dr/dQ).
__device__ __forceinline__ void slot_rows(const double* Q, const double* x0, const double* x1, double* m0, double* m1) {
    m0[0] = Q[1] * x0[2] - Q[2] * x0[1];
    m0[1] = Q[2] * x0[0] - Q[0] * x0[2];
    m0[2] = Q[0] * x0[1] - Q[1] * x0[0];
    m1[0] = Q[1] * x1[2] - Q[2] * x1[1];
    m1[1] = Q[2] * x1[0] - Q[0] * x1[2];
    m1[2] = Q[0] * x1[1] - Q[1] * x1[0];
#pragma unroll
    for (int m = 0; m < 3; m++) {
        m0[3 + m] = x0[m];
        m1[3 + m] = x1[m];
    }
}

// Z (row-major 6x6) += j0 m0^T + j1 m1^T.  With gram6_add(m0, m1, A) and grad6_add(m0, m1, q0, q1, g) a point's share of a slot block.
__device__ __forceinline__ void cross6_add(const double* j0, const double* j1, const double* m0, const double* m1, double* Z) {
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            Z[a * 6 + c] += j0[a] * m0[c];
            Z[a * 6 + c] += j1[a] * m1[c];
        }
}

// The slot block from every lane's share of Z, A and g: the 36 + 21 + 6 sums over the wave (a lane without a point of the slot adds
// zeros), column c of Z <- L^-1 (column c) and g_c -= Z_c . y, and lane 0's store to O.  Which lane holds which point decides the order
// of the wave sums: that assignment is the calling kernel's.
__device__ __forceinline__ void slot_finish(double* Z, double* A, double* g, const double* L, const double* y, int lane, double* __restrict__ O) {
#pragma unroll
    for (int e = 0; e < 36; e++) Z[e] = wave_sum_f64(Z[e]);
#pragma unroll
    for (int e = 0; e < 21; e++) A[e] = wave_sum_f64(A[e]);
#pragma unroll
    for (int e = 0; e < 6; e++) g[e] = wave_sum_f64(g[e]);
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double z[6];
#pragma unroll
        for (int a = 0; a < 6; a++) z[a] = Z[a * 6 + c];
        g[c] -= forward6_dot(L, z, y);
#pragma unroll
        for (int a = 0; a < 6; a++) Z[a * 6 + c] = z[a];
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 36; e++) O[kSlotZ + e] = Z[e];
#pragma unroll
        for (int e = 0; e < 21; e++) O[kSlotA + e] = A[e];
#pragma unroll
        for (int e = 0; e < 6; e++) O[kSlotG + e] = g[e];
    }
}

}  // namespace ctag
