// ctag_m12.h -- 12x12 blocks of doubles in LDS worked on by ONE wavefront, stated once for the kernels whose unknowns are the twelve of a
// frame of a track (theta, t, w, v): the track smoother (k_track.hip) and the track filter (k_track_filter.hip).  Entry e of a block
// belongs to lane e % 64; every entry has one owner lane and one order of summation, so the bytes of a result do not depend on where
// the wave runs.  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "ctag_math.h"

namespace ctag {

struct M12 {
    double v[144];
};
__device__ __forceinline__ void tsync() { __syncthreads(); }
__device__ __forceinline__ void m_load(M12& d, const double* __restrict__ s, int lane, double diag_scale = 1.0) {
    for (int e = lane; e < 144; e += 64) d.v[e] = (e / 12 == e % 12) ? s[e] * diag_scale : s[e];
}
__device__ __forceinline__ void m_load_t(M12& d, const double* __restrict__ s, int lane) {
    for (int e = lane; e < 144; e += 64) d.v[e] = s[(e % 12) * 12 + e / 12];
}
__device__ __forceinline__ void m_store(double* __restrict__ d, const M12& s, int lane) {
    for (int e = lane; e < 144; e += 64) d[e] = s.v[e];
}
__device__ __forceinline__ void m_zero(M12& d, int lane) {
    for (int e = lane; e < 144; e += 64) d.v[e] = 0.0;
}
// C = add + sg op(A) op(B), op = transpose when TA / TB; sums over k in order; C must not alias A or B
template <bool TA, bool TB>
__device__ __forceinline__ void m_mul(M12& C, const M12& A, const M12& B, double sg, const M12* add, int lane) {
    for (int e = lane; e < 144; e += 64) {
        const int i = e / 12, j = e % 12;
        double s = 0.0;
        for (int k = 0; k < 12; k++) s += (TA ? A.v[k * 12 + i] : A.v[i * 12 + k]) * (TB ? B.v[j * 12 + k] : B.v[k * 12 + j]);
        C.v[e] = add ? add->v[e] + sg * s : sg * s;
    }
}
// y = add + sg op(A) x for 12-vectors, lanes 0 .. 11
template <bool TA>
__device__ __forceinline__ void m_vec(double* y, const M12& A, const double* x, double sg, const double* add, int lane) {
    if (lane < 12) {
        double s = 0.0;
        for (int k = 0; k < 12; k++) s += (TA ? A.v[k * 12 + lane] : A.v[lane * 12 + k]) * x[k];
        y[lane] = add ? add[lane] + sg * s : sg * s;
    }
}
// In-place Cholesky of the lower triangle, A = L L^T; false (for the whole wave) when a pivot is not positive.  Right-looking: column j
// scaled, then every entry (i, k) of the trailing lower triangle updated by its owner lane, so each entry sees its terms in the order j = 0, 1, ...
__device__ __forceinline__ bool m_chol(M12& A, int lane) {
    bool ok = true;
    for (int j = 0; j < 12; j++) {
        tsync();
        const double p = A.v[j * 12 + j];
        ok = ok && p > 0.0;
        const double s = ctm::sqrt64(p);
        tsync();
        if (lane == j) A.v[j * 12 + j] = s;
        else if (lane > j && lane < 12) A.v[lane * 12 + j] = A.v[lane * 12 + j] / s;
        tsync();
        for (int e = lane; e < 144; e += 64) {
            const int i = e / 12, k = e % 12;
            if (k > j && i >= k) A.v[e] -= A.v[i * 12 + j] * A.v[k * 12 + j];
        }
    }
    tsync();
    return ok;
}
// one column (base col, stride) solved in place by its lane: L^-1 (forward) or L^-T (backward)
__device__ __forceinline__ void col_fwd(const M12& L, double* col, int stride) {
    for (int i = 0; i < 12; i++) {
        double s = col[i * stride];
        for (int k = 0; k < i; k++) s -= L.v[i * 12 + k] * col[k * stride];
        col[i * stride] = s / L.v[i * 12 + i];
    }
}
__device__ __forceinline__ void col_bwd(const M12& L, double* col, int stride) {
    for (int i = 11; i >= 0; i--) {
        double s = col[i * stride];
        for (int k = i + 1; k < 12; k++) s -= L.v[k * 12 + i] * col[k * stride];
        col[i * stride] = s / L.v[i * 12 + i];
    }
}
// lanes 0-11: the columns of A, 12-23: of B, 24: the vector v (any of them may be null)
template <bool FWD>
__device__ __forceinline__ void m_solve(const M12& L, M12* A, M12* B, double* v, int lane) {
    double* col = nullptr;
    int stride = 12;
    if (lane < 12) col = A ? A->v + lane : nullptr;
    else if (lane < 24) col = B ? B->v + (lane - 12) : nullptr;
    else if (lane == 24) col = v, stride = 1;
    if (col) {
        if (FWD) col_fwd(L, col, stride);
        else col_bwd(L, col, stride);
    }
}
__device__ __forceinline__ void m_identity(M12& d, int lane) {
    for (int e = lane; e < 144; e += 64) d.v[e] = (e / 12 == e % 12) ? 1.0 : 0.0;
}
// the marginal of one frame from its 12x12 block P: the pose block mirrored from its upper triangle, the square roots of the velocity diagonal
__device__ __forceinline__ void marg_store(double* __restrict__ out, const M12& P, int lane) {
    if (lane < 36) {
        const int r = lane / 6, c = lane % 6;
        out[lane] = P.v[min(r, c) * 12 + max(r, c)];
    } else if (lane < 42) {
        out[lane] = ctm::sqrt64(P.v[(lane - 30) * 12 + (lane - 30)]);
    }
}
// d = the symmetric matrix with the upper triangle of s
__device__ __forceinline__ void m_sym(M12& d, const M12& s, int lane) {
    for (int e = lane; e < 144; e += 64) {
        const int i = e / 12, j = e % 12;
        d.v[e] = s.v[min(i, j) * 12 + max(i, j)];
    }
}

}  // namespace ctag
