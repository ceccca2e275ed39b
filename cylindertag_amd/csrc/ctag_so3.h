// ctag_so3.h -- SO(3) on 3x3 row-major doubles and the "measured" rule that turns a rig pose record and its covariance record into a
// sample (R, t, W = cov^-1), stated once for the kernels that consume covariance records: the track smoother (k_track.hip), the track
// filter (k_track_filter.hip) and the hand-eye fit (k_hand_eye.hip).  Device only.
#pragma once
#include "../../include/ctag_pose.h"
#include "ctag_linalg.h"
#include "ctag_math.h"

namespace ctag {

__device__ __forceinline__ void mat3_mul_nt(const double* A, const double* B, double* C) {  // C = A B^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1] + A[i * 3 + 2] * B[j * 3 + 2];
}
__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C) {  // C = A B
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
// Log of a rotation matrix: r = theta * axis with sin(theta) axis = vee(R - R^T) / 2 and theta = atan2(|.|, (tr - 1) / 2); below
// sin(theta) = 1e-4 the series of asin(s) / s (cos > 0), or, next to a half turn, the axis from R + R^T.
__device__ __forceinline__ void so3_log(const double* R, double* r) {
    const double x = 0.5 * (R[7] - R[5]), y = 0.5 * (R[2] - R[6]), z = 0.5 * (R[3] - R[1]);
    const double s2 = x * x + y * y + z * z;
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    double k;
    if (s2 < 1e-8) {
        if (c < 0.0) {  // near a half turn: the axis from the symmetric part, R + R^T = 2 c I + 2 (1 - c) a a^T; its sign from the antisymmetric one
            const double d0 = (R[0] - c) / (1.0 - c), d1 = (R[4] - c) / (1.0 - c), d2 = (R[8] - c) / (1.0 - c);
            const int m = d0 >= d1 && d0 >= d2 ? 0 : (d1 >= d2 ? 1 : 2);
            const double am = ctm::sqrt64(m == 0 ? d0 : (m == 1 ? d1 : d2));
            double ax[3];
            for (int j = 0; j < 3; j++) ax[j] = j == m ? am : (R[m * 3 + j] + R[j * 3 + m]) / (2.0 * (1.0 - c)) / am;
            const double sg = x * ax[0] + y * ax[1] + z * ax[2] < 0.0 ? -1.0 : 1.0;
            const double th = ctm::atan2_64(ctm::sqrt64(s2), c);
            for (int j = 0; j < 3; j++) r[j] = sg * th * ax[j];
            return;
        }
        k = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0));
    } else {
        const double s = ctm::sqrt64(s2);
        k = ctm::atan2_64(s, c) / s;
    }
    r[0] = k * x;
    r[1] = k * y;
    r[2] = k * z;
}
// the inverse of the left Jacobian of SO(3): Log(Exp(d) Exp(p)) = p + J d + O(d^2), J = I - [p]x / 2 + c [p]x^2,
// c = 1 / th^2 - (1 + cos th) / (2 th sin th), its series below th^2 = 1e-4
__device__ __forceinline__ void so3_jlinv(const double* p, double* J) {
    const double t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    double c;
    if (t2 < 1e-4) {
        c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0));
    } else {
        const double th = ctm::sqrt64(t2);
        double sn, cs;
        ctm::sincos64(th, &sn, &cs);
        c = 1.0 / t2 - (1.0 + cs) / (2.0 * th * sn);
    }
    // [p]x^2 = p p^T - |p|^2 I
    J[0] = 1.0 + c * (p[0] * p[0] - t2);
    J[1] = 0.5 * p[2] + c * (p[0] * p[1]);
    J[2] = -0.5 * p[1] + c * (p[0] * p[2]);
    J[3] = -0.5 * p[2] + c * (p[1] * p[0]);
    J[4] = 1.0 + c * (p[1] * p[1] - t2);
    J[5] = 0.5 * p[0] + c * (p[1] * p[2]);
    J[6] = 0.5 * p[1] + c * (p[2] * p[0]);
    J[7] = -0.5 * p[0] + c * (p[2] * p[1]);
    J[8] = 1.0 + c * (p[2] * p[2] - t2);
}
// the left Jacobian of SO(3): Exp(p + d) = Exp(Jl d + O(d^2)) Exp(p), Jl = I + b [p]x + c [p]x^2, b = (1 - cos th) / th^2,
// c = (th - sin th) / th^3, their series below th^2 = 1e-2 (the closed forms cancel there)
__device__ __forceinline__ void so3_jl(const double* p, double* J) {
    const double t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    double b, c;
    if (t2 < 1e-2) {
        b = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0))));
        c = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (1.0 / 39916800.0))));
    } else {
        const double th = ctm::sqrt64(t2);
        double sn, cs;
        ctm::sincos64(th, &sn, &cs);
        b = (1.0 - cs) / t2;
        c = (th - sn) / (t2 * th);
    }
    J[0] = 1.0 + c * (p[0] * p[0] - t2);
    J[1] = -b * p[2] + c * (p[0] * p[1]);
    J[2] = b * p[1] + c * (p[0] * p[2]);
    J[3] = b * p[2] + c * (p[1] * p[0]);
    J[4] = 1.0 + c * (p[1] * p[1] - t2);
    J[5] = -b * p[0] + c * (p[1] * p[2]);
    J[6] = -b * p[1] + c * (p[2] * p[0]);
    J[7] = b * p[0] + c * (p[2] * p[1]);
    J[8] = 1.0 + c * (p[2] * p[2] - t2);
}

// Rule 1 of the track smoother (include/ctag_pose.h): the record pair is a measurement when the pose is CTAG_POSE_OK, the covariance
// CTAG_COV_OK in the tangent parameterisation, and cov, scaled to unit diagonal, factors with every pivot above min_pivot_allowed.
// On true R, t and the weight are written (9, 3, 36 doubles); on false nothing is.  The weight is W = cov^-1, or with WHITEN the
// whitening matrix of the same factorisation in its place: V = L^-1 D, lower triangular, W = V^T V, so that e^T W e = |V e|^2 is a sum
// of squares.
template <bool WHITEN = false, class Rec>
__device__ __forceinline__ bool measured_sample(const Rec& P, const ctag_pose_cov_rec& Q, double min_pivot_allowed, double* __restrict__ Rm,
                                                double* __restrict__ tm, double* __restrict__ W) {
    if (!(P.status == CTAG_POSE_OK && Q.status == CTAG_COV_OK && Q.param == CTAG_COV_PARAM_TANGENT)) return false;
    double d[6], Cm[36], inv[36], Linv[36], min_pivot = 0.0;
    bool good = true;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double h = Q.cov[a * 6 + a];
        good = good && ctl::finite64(h) && h > 0.0;
        d[a] = 1.0 / ctm::sqrt64(h);
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) Cm[a * 6 + b] = d[a] * Q.cov[a * 6 + b] * d[b];
    for (int k = 0; k < 3; k++) good = good && ctl::finite64(P.rvec[k]) && ctl::finite64(P.tvec[k]);
    good = good && ctl::chol6_inverse_factor(Cm, inv, WHITEN ? Linv : nullptr, min_pivot_allowed, min_pivot);
    if (!good) return false;
    double R[9];
    ctl::angle_axis_rot(P.rvec, R, nullptr);
    for (int k = 0; k < 9; k++) Rm[k] = R[k];
    for (int k = 0; k < 3; k++) tm[k] = P.tvec[k];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) W[a * 6 + b] = WHITEN ? Linv[a * 6 + b] * d[b] : d[a] * inv[a * 6 + b] * d[b];
    return true;
}

// rule 1's bad input: a tangent-less covariance that claims to be good, or a record that is not at its place
template <class Rec>
__device__ __forceinline__ bool misplaced_or_rvec(const Rec& P, const ctag_pose_cov_rec& Q, int f, int g) {
    return P.rig != g || P.frame != f || (Q.status == CTAG_COV_OK && Q.param == CTAG_COV_PARAM_RVEC);
}

}  // namespace ctag
