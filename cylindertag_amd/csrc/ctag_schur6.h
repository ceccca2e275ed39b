// ctag_schur6.h -- the 6x6 pose block of a Schur complement, as the kernels that eliminate a record's pose use it
// (k_model_fit.hip: corners against marker poses; k_rig_fit.hip: member transforms against rig poses).
#pragma once
#include <hip/hip_runtime.h>

#include "ctag_linalg.h"
#include "ctag_math.h"

namespace ctag {

// U = L L^T of a symmetric 6x6 given as its 21 upper entries in row order; false on a pivot that is not positive (or not a number)
__device__ __forceinline__ bool mfit_chol6(const double* H, double* L) {
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
__device__ __forceinline__ void mfit_forward6(const double* L, double* x) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i * 6 + k] * x[k];
        x[i] = s / L[i * 6 + i];
    }
}

}  // namespace ctag
