// ctag_pose_dev.h -- device side of the pose back end shared by k_pose.hip (one pose per marker), k_rig_pose.hip (one pose per
// rig of markers) and k_mv_pose.hip (one pose per rig from several cameras): the LDS image of one problem, PnPSolver's
// correspondence rule, and EPnP + PoseBA over n points in LDS (the arithmetic of the oracle's ctago_solve_pnp_epnp and
// ctago_pose_ba, see k_pose.hip's header for the mapping).  pose_epnp and pose_ba are the two halves; pose_ba takes the residual
// of a point as a policy (one camera: camera_residual; a camera per point: k_mv_pose.hip); pose_solve is the two in a row.
// Generic over the LDS capacity PTS and the block width NT: per-point loops stride over the NT lanes, while every sum over
// the points stays with its one owner lane (lane < 144 / 34), so the result is the sequential evaluation for any n <= PTS.
// k_pose_cov.hip (the covariance of a finished pose), k_model_fit.hip, k_rig_fit.hip, k_cam_fit.hip and k_intr_fit.hip read the
// correspondence rule, the corner loaders, the residuals, the point descriptor and load_state6 from here.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ctag_pose.h"
#include "ctag_linalg.h"

namespace ctag {

struct PoseCam {
    double fx, fy, cx, cy;
    double k[12];
};

// the camera as the kernels read it (host side; camera_ok() has accepted it)
inline PoseCam make_pose_cam(const ctag_camera* camera) {
    PoseCam cam;
    cam.fx = (double)camera->K[0];
    cam.fy = (double)camera->K[4];
    cam.cx = (double)camera->K[2];
    cam.cy = (double)camera->K[5];
    for (int i = 0; i < 12; i++) cam.k[i] = i < camera->n_dist ? (double)camera->dist[i] : 0.0;
    return cam;
}

struct PoseModelDev {
    int n_models, model_size;
    const int32_t* marker_id;
    const float* corners;
};

constexpr int kPoseMaxPts = CTAG_POSE_MAX_POINTS;
constexpr int kPoseSmallPts = 96;  // dictionaries of <= 12 columns (the reference's CTag_2f12c): 16 KB of LDS, two waves per SIMD
constexpr int kJStride = 15;  // 12 Jacobian entries + 2 residuals per point, odd stride: conflict-free lane-per-point writes

// LDS image of one marker's problem (doubles)
template <int kPoseMaxPts>
struct PoseLds {
    double X[kPoseMaxPts * 3];    // world points
    double OBS[kPoseMaxPts * 2];  // BA observations (undistorted, through K, rounded to float)
    union {
        struct {
            double US[kPoseMaxPts * 2];  // EPnP pixel coordinates
            double AL[kPoseMaxPts * 4];  // barycentric coordinates
            double PC[kPoseMaxPts * 3];  // camera-frame points
            double A[144], V[144];       // M^T M and its eigenvectors
            double E[kPoseMaxPts];       // per-point reprojection error
        } e;
        struct {
            double JR[kPoseMaxPts * kJStride];  // per point: 2 x 6 column-scaled Jacobian entries, 2 residuals
        } b;
    } u;
    double cws[12], ccs[12], ci[9];
    double vv[48];  // the four null-space vectors
    double L[60], rho[6];
    double betas[16];
    double Rs[36], ts[12], rep[4];
    double s9[9], s3a[3], s3b[3];
    double red[34];
    double x[6];
    double rot[18];
    int rflag[6];
    int jac_flag;
};

__device__ __forceinline__ void wave_sync() { __syncthreads(); }  // the whole block (one wave in k_pose)

#ifdef CTAG_POSE_PROF
static __device__ unsigned long long g_pose_prof[16];  // per translation unit: k_pose.hip reads its own (ctag_pose_debug_prof)
#define PROF_MARK(i)                                                                    \
    do {                                                                                \
        const unsigned long long now__ = __builtin_readcyclecounter();                  \
        if (lane == 0) atomicAdd(&g_pose_prof[i], now__ - prof_t);                      \
        prof_t = now__;                                                                 \
    } while (0)
#else
#define PROF_MARK(i)
#endif

// cvUndistortPointsInternal, 5 iterations (same statement as the oracle's)
__device__ __forceinline__ void undistort_normalised(const PoseCam& c, double u, double v, double& xo, double& yo) {
    double x = (u - c.cx) / c.fx, y = (v - c.cy) / c.fy;
    const double x0 = x, y0 = y;
    const double* k = c.k;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) {
            x = x0;
            y = y0;
            break;
        }
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    xo = x;
    yo = y;
}

// epnp::gauss_newton on one lane
__device__ void gauss_newton(const double* L, const double* rho, double* b) {
    for (int it = 0; it < 5; it++) {
        double A[24], B[6], X[4];
        for (int i = 0; i < 6; i++) {
            const double* l = L + 10 * i;
            A[4 * i] = 2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3];
            A[4 * i + 1] = l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3];
            A[4 * i + 2] = l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3];
            A[4 * i + 3] = l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3];
            B[i] = rho[i] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] +
                             l[5] * b[2] * b[2] + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] * b[3]);
        }
        ctl::qr_solve<6, 4>(A, B, X);
        for (int i = 0; i < 4; i++) b[i] += X[i];
    }
}

// residual and Jacobian rows of point p under pose (R, dR, t): the arithmetic of the oracle's BA::eval
__device__ __forceinline__ void point_residual(const double* R, const double* dR, const double* x, double fx, double fy, double cx,
                                               double cy, const double* p, const double* ob, double& r0, double& r1, double* j0,
                                               double* j1, bool with_j) {
    const double P0 = (R[0] * p[0] + R[1] * p[1] + R[2] * p[2]) + x[3];
    const double P1 = (R[3] * p[0] + R[4] * p[1] + R[5] * p[2]) + x[4];
    const double P2 = (R[6] * p[0] + R[7] * p[1] + R[8] * p[2]) + x[5];
    const double iz = 1.0 / P2;
    r0 = (fx * (P0 * iz) + cx) - ob[0];
    r1 = (fy * (P1 * iz) + cy) - ob[1];
    if (with_j) {
        const double a0 = fx * iz, a1 = fy * iz;
        const double b0 = fx * P0 * iz * iz, b1 = fy * P1 * iz * iz;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double* D = dR + 9 * k;
            const double d0 = D[0] * p[0] + D[1] * p[1] + D[2] * p[2];
            const double d1 = D[3] * p[0] + D[4] * p[1] + D[5] * p[2];
            const double d2 = D[6] * p[0] + D[7] * p[1] + D[8] * p[2];
            j0[k] = a0 * d0 - b0 * d2;
            j1[k] = a1 * d1 - b1 * d2;
        }
        j0[3] = a0;
        j0[4] = 0.0;
        j0[5] = -b0;
        j1[3] = 0.0;
        j1[4] = a1;
        j1[5] = -b1;
    }
}

// PnPSolver's correspondences of marker M (pose_estimation.cpp:72-95, the oracle's ctago_build_correspondences): for every
// feature that contributes, emit(F, pos, cnt, i0) with its cnt (4 or 8) points going to i0 .. i0+cnt-1, i0 counted from the
// incoming n; n is advanced.  Returns CTAG_POSE_BAD_POS for a marker whose features lie outside the record, a position outside
// the model, or more points than min(model_size*8, cap); CTAG_POSE_OK otherwise.
template <class Emit>
__device__ __forceinline__ int marker_points(const ctag_frame_result& FR, const ctag_marker_rec& M, int model_size, int cap, int& n, Emit&& emit) {
    const int nf = M.n_features;
    // a marker that points outside the frame's feature array (hand-built or corrupted record) is rejected, never read
    if (M.first_feature < 0 || nf < 0 || M.first_feature > CTAG_MAX_FEATURES - nf) return CTAG_POSE_BAD_POS;
    for (int j = 0; j < nf; j++) {
        const ctag_feature_rec& F = FR.features[M.first_feature + j];
        const int idl = F.id_left, idr = F.id_right, pos = F.pos;
        const int d = idl - idr;
        const int ad = d < 0 ? -d : d;
        if (nf > 3 && (j == 0 || j == nf - 1) && (ad > 1 || idr == -1)) continue;
        if (j >= M.n_pos || pos < 0 || pos >= model_size) return CTAG_POSE_BAD_POS;
        const int cnt = (ad < 3 && idr != -1) ? 8 : 4;
        if (n + cnt > model_size * 8 || n + cnt > cap) return CTAG_POSE_BAD_POS;  // repeated positions: more points than the model has
        emit(F, pos, cnt, n);
        n += cnt;
    }
    return CTAG_POSE_OK;
}

// the first model with this marker id (pose_estimation.cpp:57-70), -1 if none
__device__ __forceinline__ int model_lookup(const PoseModelDev& model, int marker_id) {
    for (int j = 0; j < model.n_models; j++)
        if (model.marker_id[j] == marker_id) return j;
    return -1;
}

// corner q of an emit (order 0 1 4 5 2 3 6 7) of feature F at model position pos: its pixel undistorted to normalised
// coordinates (xn, yn), the BA observation ob[2] (through K, rounded to float) and the model point X[3]; `corners` is the model's
// corner list
__device__ __forceinline__ void corner_point(const PoseCam& cam, const float* __restrict__ corners, const ctag_feature_rec& F, int pos, int q,
                                             double& xn, double& yn, double* ob, double* X) {
    const int k = q < 2 ? q : q < 4 ? q + 2 : q < 6 ? q - 2 : q;  // 0 1 4 5 2 3 6 7
    const double u = (double)F.corners[2 * k], v = (double)F.corners[2 * k + 1];
    undistort_normalised(cam, u, v, xn, yn);
    ob[0] = (double)(float)(cam.fx * xn + cam.cx);
    ob[1] = (double)(float)(cam.fy * yn + cam.cy);
    const float* cp = corners + (pos * 8 + k) * 3;
    X[0] = (double)cp[0];
    X[1] = (double)cp[1];
    X[2] = (double)cp[2];
}

// the same corner as detected: its raw pixel uv[2], never undistorted, and the model point X[3] (the intrinsics fit, k_intr_fit.hip)
__device__ __forceinline__ void corner_pixel(const float* __restrict__ corners, const ctag_feature_rec& F, int pos, int q, double* uv, double* X) {
    const int k = q < 2 ? q : q < 4 ? q + 2 : q < 6 ? q - 2 : q;  // 0 1 4 5 2 3 6 7
    uv[0] = (double)F.corners[2 * k];
    uv[1] = (double)F.corners[2 * k + 1];
    const float* cp = corners + (pos * 8 + k) * 3;
    X[0] = (double)cp[0];
    X[1] = (double)cp[1];
    X[2] = (double)cp[2];
}

// Where a point of a record comes from, in one word, for the kernels that walk a record once and visit its points afterwards
// (k_pose_cov.hip, k_model_fit.hip, k_rig_fit.hip, k_cam_fit.hip, k_intr_fit.hip): feature index in its frame record (7 bits) | corner q of the emit << 7 (3 bits) |
// camera << 10 (3 bits) | model position << 13 (positions are below 2^16)
static_assert(CTAG_MAX_FEATURES <= 128 && CTAG_MV_MAX_CAMERAS <= 8, "the point descriptor's bit fields");
__device__ __forceinline__ int32_t point_desc(int feature, int q, int cam, int pos) { return feature | (q << 7) | (cam << 10) | (pos << 13); }
__device__ __forceinline__ int desc_feature(int32_t s) { return s & 127; }
__device__ __forceinline__ int desc_q(int32_t s) { return (s >> 7) & 7; }
__device__ __forceinline__ int desc_cam(int32_t s) { return (s >> 10) & 7; }
__device__ __forceinline__ int desc_pos(int32_t s) { return s >> 13; }

constexpr int kFitMaxPts = CTAG_RIG_MAX_POINTS;  // points of an observation record of a fit at most

// The member walk of the fits' record kernels (k_rfit_record; k_cfit_record, once per camera; k_ifit_pose and k_ifit_record): the
// markers k < min(max(n_markers, 0), CTAG_MAX_MARKERS) of FR whose bit is set in mask[4], in marker order, each with the model
// model_lookup gives it and its points in the builder's order (marker_points).  member(mi, base) is called for a member of model mi
// whose points start at n = base, before them, and may turn it down; point(i, desc, mi) is called in lane q < cnt of an emit for the
// lane's point i with its point_desc under camera `cam`.  n is advanced.  False -- the record does not describe its detection record
// -- for a member without a model or turned down, a marker marker_points rejects, or more than kFitMaxPts points; what member and
// point have written by then is not to be used.  A mask bit at or above the frame's marker count is ignored (k_pose_cov.hip's
// cov_add_members rejects it, and k_rig_count and k_mv_count load points as they walk: those walks are their own).  Wave-uniform.
template <class Member, class Point>
__device__ __forceinline__ bool fit_member_walk(const ctag_frame_result& FR, const uint32_t* mask, const PoseModelDev& model, int lane, int cam, int& n,
                                                Member&& member, Point&& point) {
    const int nm = min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
    const ctag_feature_rec* F0 = FR.features;
    for (int k = 0; k < nm; k++) {
        if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
        const int mi = model_lookup(model, FR.markers[k].marker_id);
        if (mi < 0 || !member(mi, n)) return false;
        const int base = n;
        int nl = 0;
        const int st = marker_points(FR, FR.markers[k], model.model_size, kPoseMaxPts, nl, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
            if (lane < cnt && base + i0 + cnt <= kFitMaxPts) point(base + i0 + lane, point_desc((int)(&F - F0), lane, cam, pos), mi);
        });
        if (st != CTAG_POSE_OK || base + nl > kFitMaxPts) return false;
        n += nl;
    }
    return true;
}

// x = (rvec, tvec) of a pose record of any kind; false when one of the six is not finite
template <class Rec>
__device__ __forceinline__ bool load_state6(const Rec& P, double* x) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        x[i] = P.rvec[i];
        x[3 + i] = P.tvec[i];
        ok = ok && ctl::finite64(x[i]) && ctl::finite64(x[3 + i]);
    }
    return ok;
}

// lane q < cnt of an emit: that corner as point i of the problem
template <int PTS>
__device__ __forceinline__ void load_point(PoseLds<PTS>& S, const PoseCam& cam, const float* __restrict__ corners, const ctag_feature_rec& F,
                                           int pos, int q, int i) {
    double xn, yn;
    corner_point(cam, corners, F, pos, q, xn, yn, S.OBS + 2 * i, S.X + 3 * i);
    S.u.e.US[2 * i] = (double)(float)xn * cam.fx + cam.cx;
    S.u.e.US[2 * i + 1] = (double)(float)yn * cam.fy + cam.cy;
}

// EPnP (solvePnP SOLVEPNP_EPNP) over the n >= 4 points the block has loaded into S (X, u.e.US), by the NT threads of the
// block (lane = threadIdx.x).  True: S.x holds the pose (rvec, tvec).  False: the result is not finite.  Every thread of the
// block calls it and gets the same answer; it synchronises the block.
template <int PTS, int NT>
__device__ __forceinline__ bool pose_epnp(PoseLds<PTS>& S, const int lane, const int n, const PoseCam& cam) {
#ifdef CTAG_POSE_PROF
    unsigned long long prof_t = __builtin_readcyclecounter();
#endif
    // =========================================== EPnP ===========================================
    const double dn = (double)n;
    // choose_control_points: centroid (lane j sums coordinate j in point order)
    if (lane < 3) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s += S.X[3 * i + lane];
        S.cws[lane] = s / dn;
    }
    wave_sync();
    if (lane < 9) {  // PW0^T PW0, lane = entry (a,b)
        const int a = lane / 3, b = lane % 3;
        const double ca = S.cws[a], cb = S.cws[b];
        double s = 0.0;
        for (int i = 0; i < n; i++) s += (S.X[3 * i + a] - ca) * (S.X[3 * i + b] - cb);
        S.s9[lane] = s;
    }
    wave_sync();
    if (lane == 0) {
        double C[9], V[9], w3[3];
        for (int i = 0; i < 9; i++) C[i] = S.s9[i];
        ctl::jacobi_eig<3>(C, V, w3);
        int ord[3];
        ctl::sort_desc<3>(w3, ord);
        for (int i = 1; i < 4; i++) {
            const double dc = w3[ord[i - 1]];
            const double k = ctm::sqrt64((dc > 0 ? dc : 0.0) / dn);
            for (int j = 0; j < 3; j++) S.cws[3 * i + j] = S.cws[j] + k * V[j * 3 + ord[i - 1]];
        }
        // compute_barycentric_coordinates: CC^-1
        double cc[9], ci[9];
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = S.cws[3 * j + i] - S.cws[i];
        const bool ok = ctl::inv3(cc, ci);
        for (int i = 0; i < 9; i++) S.ci[i] = ok ? ci[i] : 0.0;
        S.jac_flag = ok ? 1 : 0;
        // compute_rho
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        for (int i = 0; i < 6; i++) {
            double d2 = 0.0;
            for (int k = 0; k < 3; k++) d2 += (S.cws[3 * pa[i] + k] - S.cws[3 * pb[i] + k]) * (S.cws[3 * pa[i] + k] - S.cws[3 * pb[i] + k]);
            S.rho[i] = d2;
        }
    }
    wave_sync();
    if (!S.jac_flag) return false;
    for (int i = lane; i < n; i += NT) {  // alphas
        const double p0 = S.X[3 * i] - S.cws[0], p1 = S.X[3 * i + 1] - S.cws[1], p2 = S.X[3 * i + 2] - S.cws[2];
        double a[4];
#pragma unroll
        for (int j = 0; j < 3; j++) a[1 + j] = S.ci[3 * j] * p0 + S.ci[3 * j + 1] * p1 + S.ci[3 * j + 2] * p2;
        a[0] = 1.0 - a[1] - a[2] - a[3];
#pragma unroll
        for (int j = 0; j < 4; j++) S.u.e.AL[4 * i + j] = a[j];
    }
    wave_sync();
    PROF_MARK(1);
    // M^T M: lane = entry (r,c), rows of M in point order (fill_M + cvMulTransposed)
    for (int e = lane; e < 144; e += NT) {
        const int r = e / 12, c = e % 12;
        const int rj = r / 3, rk = r % 3, cj = c / 3, ck = c % 3;
        double acc = 0.0;
        for (int i = 0; i < n; i++) {
            const double ar = S.u.e.AL[4 * i + rj], ac = S.u.e.AL[4 * i + cj];
            const double u = S.u.e.US[2 * i], v = S.u.e.US[2 * i + 1];
            const double m1r = rk == 0 ? ar * cam.fx : (rk == 1 ? 0.0 : ar * (cam.cx - u));
            const double m2r = rk == 0 ? 0.0 : (rk == 1 ? ar * cam.fy : ar * (cam.cy - v));
            const double m1c = ck == 0 ? ac * cam.fx : (ck == 1 ? 0.0 : ac * (cam.cx - u));
            const double m2c = ck == 0 ? 0.0 : (ck == 1 ? ac * cam.fy : ac * (cam.cy - v));
            acc += m1r * m1c;
            acc += m2r * m2c;
        }
        S.u.e.A[e] = acc;
        S.u.e.V[e] = (r == c) ? 1.0 : 0.0;
    }
    wave_sync();
    PROF_MARK(2);
    // cyclic Jacobi with the round-robin pair order of ctl::jacobi_eig_rr12: the six rotations of a round are computed
    // by six lanes and applied side by side (15 lanes own the 2x2 blocks between two pairs, 6 the pairs' own entries,
    // 72 lane-tasks the eigenvector columns); bit-identical to the sequential sweep, see ctl::rr12_pair
    for (int sweep = 0; sweep < 60; sweep++) {
        double sm = 0.0;
        for (int p = 0; p < 11; p++)
            for (int q = p + 1; q < 12; q++) sm += ctm::fabs64(S.u.e.A[p * 12 + q]);
        if (sm == 0.0) break;  // uniform
        for (int round = 0; round < 11; round++) {
            if (lane < 6) {
                int p, q;
                ctl::rr12_pair(round, lane, p, q);
                const ctl::JacobiRot r = ctl::jacobi_rot(S.u.e.A[p * 12 + p], S.u.e.A[q * 12 + q], S.u.e.A[p * 12 + q], sweep);
                S.rot[3 * lane] = r.s;
                S.rot[3 * lane + 1] = r.tau;
                S.rot[3 * lane + 2] = r.h;
                S.rflag[lane] = r.zero ? 2 : (r.rotate ? 1 : 0);
            }
            wave_sync();
            if (lane < 15) {  // block between pair i and pair j, i < j (processing order)
                int i = 0, e = lane;
                while (e >= 5 - i) {
                    e -= 5 - i;
                    i++;
                }
                const int j = i + 1 + e;
                const int fi = S.rflag[i], fj = S.rflag[j];
                if (fi == 1 || fj == 1) {
                    int pi, qi, pj, qj;
                    ctl::rr12_pair(round, i, pi, qi);
                    ctl::rr12_pair(round, j, pj, qj);
                    double b00 = S.u.e.A[pi * 12 + pj], b01 = S.u.e.A[pi * 12 + qj], b10 = S.u.e.A[qi * 12 + pj], b11 = S.u.e.A[qi * 12 + qj];
                    if (fi == 1) {
                        const double s_ = S.rot[3 * i], t_ = S.rot[3 * i + 1];
                        ctl::jacobi_apply(b00, b10, s_, t_);
                        ctl::jacobi_apply(b01, b11, s_, t_);
                    }
                    if (fj == 1) {
                        const double s_ = S.rot[3 * j], t_ = S.rot[3 * j + 1];
                        ctl::jacobi_apply(b00, b01, s_, t_);
                        ctl::jacobi_apply(b10, b11, s_, t_);
                    }
                    S.u.e.A[pi * 12 + pj] = b00;
                    S.u.e.A[pj * 12 + pi] = b00;
                    S.u.e.A[pi * 12 + qj] = b01;
                    S.u.e.A[qj * 12 + pi] = b01;
                    S.u.e.A[qi * 12 + pj] = b10;
                    S.u.e.A[pj * 12 + qi] = b10;
                    S.u.e.A[qi * 12 + qj] = b11;
                    S.u.e.A[qj * 12 + qi] = b11;
                }
            } else if (lane < 21) {  // the pair's own entries
                const int i = lane - 15;
                const int f = S.rflag[i];
                if (f) {
                    int p, q;
                    ctl::rr12_pair(round, i, p, q);
                    if (f == 1) {
                        const double h = S.rot[3 * i + 2];
                        S.u.e.A[p * 12 + p] -= h;
                        S.u.e.A[q * 12 + q] += h;
                    }
                    S.u.e.A[p * 12 + q] = 0.0;
                    S.u.e.A[q * 12 + p] = 0.0;
                }
            }
            for (int t = lane - 21; t < 72; t += NT) {  // eigenvector columns: task = (pair, row k)
                if (t < 0) continue;
                const int i = t / 12, k = t % 12;
                if (S.rflag[i] == 1) {
                    int p, q;
                    ctl::rr12_pair(round, i, p, q);
                    double vx = S.u.e.V[k * 12 + p], vy = S.u.e.V[k * 12 + q];
                    ctl::jacobi_apply(vx, vy, S.rot[3 * i], S.rot[3 * i + 1]);
                    S.u.e.V[k * 12 + p] = vx;
                    S.u.e.V[k * 12 + q] = vy;
                }
            }
            wave_sync();
        }
    }
    wave_sync();
    PROF_MARK(3);
    if (lane == 0) {  // the four smallest eigenvalues' vectors = rows 11, 10, 9, 8 of cvSVD's U^T
        double w12[12];
        for (int i = 0; i < 12; i++) w12[i] = S.u.e.A[i * 12 + i];
        int ord[12];
        ctl::sort_desc<12>(w12, ord);
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 12; k++) S.vv[12 * j + k] = S.u.e.V[k * 12 + ord[11 - j]];
    }
    wave_sync();
    if (lane < 6) {  // compute_L_6x10, lane = control-point pair
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        const int a = pa[lane], b = pb[lane];
        double dv[4][3];
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 3; k++) dv[i][k] = S.vv[12 * i + 3 * a + k] - S.vv[12 * i + 3 * b + k];
        auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
        double* row = S.L + 10 * lane;
        row[0] = dot(dv[0], dv[0]);
        row[1] = 2.0 * dot(dv[0], dv[1]);
        row[2] = dot(dv[1], dv[1]);
        row[3] = 2.0 * dot(dv[0], dv[2]);
        row[4] = 2.0 * dot(dv[1], dv[2]);
        row[5] = dot(dv[2], dv[2]);
        row[6] = 2.0 * dot(dv[0], dv[3]);
        row[7] = 2.0 * dot(dv[1], dv[3]);
        row[8] = 2.0 * dot(dv[2], dv[3]);
        row[9] = dot(dv[3], dv[3]);
    }
    wave_sync();
    PROF_MARK(4);
    if (lane >= 1 && lane <= 3) {  // find_betas_approx_{1,2,3} + gauss_newton, lane = N
        double L[60], rho[6], be[4];
        for (int i = 0; i < 60; i++) L[i] = S.L[i];
        for (int i = 0; i < 6; i++) rho[i] = S.rho[i];
        if (lane == 1) {
            double A[24], B[6], b4[4];
            for (int i = 0; i < 6; i++) {
                A[4 * i] = L[10 * i];
                A[4 * i + 1] = L[10 * i + 1];
                A[4 * i + 2] = L[10 * i + 3];
                A[4 * i + 3] = L[10 * i + 6];
                B[i] = rho[i];
            }
            ctl::qr_solve<6, 4>(A, B, b4);
            if (b4[0] < 0) {
                be[0] = ctm::sqrt64(-b4[0]);
                be[1] = -b4[1] / be[0];
                be[2] = -b4[2] / be[0];
                be[3] = -b4[3] / be[0];
            } else {
                be[0] = ctm::sqrt64(b4[0]);
                be[1] = b4[1] / be[0];
                be[2] = b4[2] / be[0];
                be[3] = b4[3] / be[0];
            }
        } else if (lane == 2) {
            double A[18], B[6], b3[3];
            for (int i = 0; i < 6; i++) {
                A[3 * i] = L[10 * i];
                A[3 * i + 1] = L[10 * i + 1];
                A[3 * i + 2] = L[10 * i + 2];
                B[i] = rho[i];
            }
            ctl::qr_solve<6, 3>(A, B, b3);
            if (b3[0] < 0) {
                be[0] = ctm::sqrt64(-b3[0]);
                be[1] = (b3[2] < 0) ? ctm::sqrt64(-b3[2]) : 0.0;
            } else {
                be[0] = ctm::sqrt64(b3[0]);
                be[1] = (b3[2] > 0) ? ctm::sqrt64(b3[2]) : 0.0;
            }
            if (b3[1] < 0) be[0] = -be[0];
            be[2] = 0.0;
            be[3] = 0.0;
        } else {
            double A[30], B[6], b5[5];
            for (int i = 0; i < 6; i++) {
                for (int j = 0; j < 5; j++) A[5 * i + j] = L[10 * i + j];
                B[i] = rho[i];
            }
            ctl::qr_solve<6, 5>(A, B, b5);
            if (b5[0] < 0) {
                be[0] = ctm::sqrt64(-b5[0]);
                be[1] = (b5[2] < 0) ? ctm::sqrt64(-b5[2]) : 0.0;
            } else {
                be[0] = ctm::sqrt64(b5[0]);
                be[1] = (b5[2] > 0) ? ctm::sqrt64(b5[2]) : 0.0;
            }
            if (b5[1] < 0) be[0] = -be[0];
            be[2] = b5[3] / be[0];
            be[3] = 0.0;
        }
        gauss_newton(L, rho, be);
        for (int i = 0; i < 4; i++) S.betas[4 * lane + i] = be[i];
    }
    wave_sync();
    PROF_MARK(5);
    for (int N = 1; N <= 3; N++) {  // compute_R_and_t + reprojection_error
        if (lane < 12) {  // compute_ccs: ccs[j][k] = sum_i betas[i] * v[i][3j+k], i ascending from 0
            double s = 0.0;
            for (int i = 0; i < 4; i++) s += S.betas[4 * N + i] * S.vv[12 * i + lane];
            S.ccs[lane] = s;
        }
        wave_sync();
        {
            // solve_for_sign looks at pcs[2] of point 0
            const double* a0 = S.u.e.AL;
            const double z0 = a0[0] * S.ccs[2] + a0[1] * S.ccs[5] + a0[2] * S.ccs[8] + a0[3] * S.ccs[11];
            const bool neg = z0 < 0.0;
            for (int i = lane; i < n; i += NT) {
                const double* a = S.u.e.AL + 4 * i;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const double v = a[0] * S.ccs[j] + a[1] * S.ccs[3 + j] + a[2] * S.ccs[6 + j] + a[3] * S.ccs[9 + j];
                    S.u.e.PC[3 * i + j] = neg ? -v : v;
                }
            }
        }
        wave_sync();
        if (lane < 6) {  // centroids pc0 (lanes 0-2) and pw0 (lanes 3-5)
            const double* src = lane < 3 ? S.u.e.PC : S.X;
            const int j = lane % 3;
            double s = 0.0;
            for (int i = 0; i < n; i++) s += src[3 * i + j];
            (lane < 3 ? S.s3a : S.s3b)[j] = s / dn;
        }
        wave_sync();
        if (lane < 9) {
            const int j = lane / 3, k = lane % 3;
            const double cj = S.s3a[j], wk = S.s3b[k];
            double s = 0.0;
            for (int i = 0; i < n; i++) s += (S.u.e.PC[3 * i + j] - cj) * (S.X[3 * i + k] - wk);
            S.s9[lane] = s;
        }
        wave_sync();
        if (lane == 0) {
            double abt[9], U[9], sv[3], V[9], R[9];
            for (int i = 0; i < 9; i++) abt[i] = S.s9[i];
            ctl::svd3(abt, U, sv, V);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                               R[0] * R[5] * R[7];
            if (det < 0) {
                R[6] = -R[6];
                R[7] = -R[7];
                R[8] = -R[8];
            }
            for (int i = 0; i < 9; i++) S.Rs[9 * N + i] = R[i];
            for (int j = 0; j < 3; j++)
                S.ts[3 * N + j] = S.s3a[j] - (R[3 * j] * S.s3b[0] + R[3 * j + 1] * S.s3b[1] + R[3 * j + 2] * S.s3b[2]);
        }
        wave_sync();
        for (int i = lane; i < n; i += NT) {
            const double* R = S.Rs + 9 * N;
            const double* t = S.ts + 3 * N;
            const double* pw = S.X + 3 * i;
            const double Xc = R[0] * pw[0] + R[1] * pw[1] + R[2] * pw[2] + t[0];
            const double Yc = R[3] * pw[0] + R[4] * pw[1] + R[5] * pw[2] + t[1];
            const double inv_Zc = 1.0 / (R[6] * pw[0] + R[7] * pw[1] + R[8] * pw[2] + t[2]);
            const double ue = cam.cx + cam.fx * Xc * inv_Zc, ve = cam.cy + cam.fy * Yc * inv_Zc;
            const double u = S.u.e.US[2 * i], v = S.u.e.US[2 * i + 1];
            S.u.e.E[i] = ctm::sqrt64((u - ue) * (u - ue) + (v - ve) * (v - ve));
        }
        wave_sync();
        if (lane == 0) {
            double s = 0.0;
            for (int i = 0; i < n; i++) s += S.u.e.E[i];
            S.rep[N] = s / dn;
        }
        wave_sync();
    }
    PROF_MARK(6);
    if (lane == 0) {
        int N = 1;
        if (S.rep[2] < S.rep[1]) N = 2;
        if (S.rep[3] < S.rep[N]) N = 3;
        bool fin = true;
        for (int i = 0; i < 9; i++) fin = fin && ctl::finite64(S.Rs[9 * N + i]);
        for (int i = 0; i < 3; i++) fin = fin && ctl::finite64(S.ts[3 * N + i]);
        double rv[3] = {0, 0, 0};
        if (fin) {
            double R[9];
            for (int i = 0; i < 9; i++) R[i] = S.Rs[9 * N + i];
            ctl::rodrigues_from_matrix(R, rv);
            for (int i = 0; i < 3; i++) fin = fin && ctl::finite64(rv[i]);
        }
        S.jac_flag = fin ? 1 : 0;
        for (int i = 0; i < 3; i++) {
            S.x[i] = rv[i];
            S.x[3 + i] = S.ts[3 * N + i];
        }
    }
    wave_sync();
    if (!S.jac_flag) return false;
    PROF_MARK(7);
    return true;
}

// PoseBA from the pose x over the n points of S (X, OBS), by the NT threads of the block; x is the same in every thread and
// comes back refined.  residual(i, R, dR, y, r0, r1, j0, j1) gives point i's residuals and Jacobian rows at pose y (R, dR =
// angle_axis_rot(y)).  Every thread of the block calls it; it synchronises the block.
// Ceres TrustRegionMinimizer + LevenbergMarquardtStrategy (see the oracle for the statement of the loop).
// All lanes carry the same x / radius / cost.  Lane = point writes its two (column-scaled) Jacobian rows and
// residuals to LDS; lane e < 34 owns one sequentially accumulated sum over those rows: e < 21 an entry of
// J^T J, 21..26 of J^T r, 27 the cost, 28..33 a squared column norm.  Every owner runs the same loop
// (acc += o[i0]*o[i1]; acc += o[i2]*o[i3]) with its own four offsets, so the 34 sums advance together.  The
// candidate point is evaluated WITH its Jacobian and normal equations, which an accepted step then keeps.
template <int PTS, int NT, class Residual>
__device__ __forceinline__ void pose_ba(PoseLds<PTS>& S, const int lane, const int n, double (&x)[6], Residual&& residual, int& iterations,
                                        double& cost_start, double& cost_end) {
#ifdef CTAG_POSE_PROF
    unsigned long long prof_t = __builtin_readcyclecounter();
#endif
    double xc[6];
    int i0 = 12, i1 = 12, i2 = 13, i3 = 13;  // lane 27 (and the idle lanes): the cost
    {
        int e = lane, a = 0;
        if (e < 21) {
            while (e >= 6 - a) {
                e -= 6 - a;
                a++;
            }
            i0 = a;
            i1 = a + e;
            i2 = 6 + a;
            i3 = 6 + a + e;
        } else if (e < 27) {
            i0 = e - 21;
            i1 = 12;
            i2 = 6 + e - 21;
            i3 = 13;
        } else if (e >= 28 && e < 34) {
            i0 = i1 = e - 28;
            i2 = i3 = 6 + e - 28;
        }
    }
    double scale[6] = {1, 1, 1, 1, 1, 1};
    auto eval_points = [&](const double* y) {  // rows of every point at pose y -> S.u.b.JR
        double R[9], dR[27];
        ctl::angle_axis_rot(y, R, dR);
        wave_sync();
        for (int i = lane; i < n; i += NT) {
            double r0, r1, j0[6], j1[6];
            residual(i, R, dR, y, r0, r1, j0, j1);
            double* o = S.u.b.JR + i * kJStride;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                o[a] = j0[a] * scale[a];
                o[6 + a] = j1[a] * scale[a];
            }
            o[12] = r0;
            o[13] = r1;
        }
        wave_sync();
    };
    auto accumulate = [&]() -> double {
        double acc = 0.0;
        if (lane < 34) {
            for (int q = 0; q < n; q++) {
                const double* o = S.u.b.JR + q * kJStride;
                acc += o[i0] * o[i1];
                acc += o[i2] * o[i3];
            }
        }
        return acc;
    };
    double H[36], g[6];
    auto publish = [&](double v) {  // the owners' sums to LDS
        wave_sync();
        if (lane < 34) S.red[lane] = v;
        wave_sync();
    };
    auto take = [&](double* Ho, double* go) {  // ... and from there to every lane
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                Ho[a * 6 + b] = S.red[e];
                Ho[b * 6 + a] = S.red[e];
                e++;
            }
#pragma unroll
        for (int a = 0; a < 6; a++) go[a] = S.red[21 + a];
    };
    auto gradient_max = [&]() {
        double m = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double v = ctm::fabs64(g[a] / scale[a]);
            if (v > m) m = v;
        }
        return m;
    };
    // first evaluation with unit scaling: cost and the Jacobi scaling (column norms); then the rows are scaled in place
    eval_points(x);
    publish(accumulate());
    double cost = 0.5 * S.red[27];
#pragma unroll
    for (int a = 0; a < 6; a++) scale[a] = 1.0 / (1.0 + ctm::sqrt64(S.red[28 + a]));
    const double cost0 = cost;
    int iter = 0;
    bool live = ctl::finite64(cost);
    if (live) {
        for (int i = lane; i < n; i += NT) {
            double* o = S.u.b.JR + i * kJStride;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                o[a] = o[a] * scale[a];
                o[6 + a] = o[6 + a] * scale[a];
            }
        }
        wave_sync();
        publish(accumulate());
        take(H, g);
        if (gradient_max() <= 1e-15) live = false;
    }
    double radius = 1e4, decrease_factor = 2.0;
    while (live && iter < 50) {
        iter++;
        if (radius < 1e-32) break;
        double A[36], rhs[6], delta[6];
#pragma unroll
        for (int i = 0; i < 36; i++) A[i] = H[i];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double d = H[a * 6 + a];
            d = d < 1e-6 ? 1e-6 : (d > 1e32 ? 1e32 : d);
            A[a * 6 + a] += d / radius;
            rhs[a] = -g[a];
        }
        bool ok = ctl::chol6_solve(A, rhs, delta);
        double model_cost_change = 0.0;
        if (ok) {
            double dg = 0.0, dHd = 0.0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                dg += delta[a] * g[a];
                double hd = 0.0;
#pragma unroll
                for (int b = 0; b < 6; b++) hd += H[a * 6 + b] * delta[b];
                dHd += delta[a] * hd;
            }
            model_cost_change = -(dg + 0.5 * dHd);
#pragma unroll
            for (int a = 0; a < 6; a++) ok = ok && ctl::finite64(delta[a]);
        }
        if (!ok || !(model_cost_change > 0.0)) {
            radius = radius / decrease_factor;
            decrease_factor *= 2.0;
            continue;
        }
        double step2 = 0.0, x2 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double du = delta[a] * scale[a];
            xc[a] = x[a] + du;
            step2 += du * du;
            x2 += x[a] * x[a];
        }
        eval_points(xc);
        publish(accumulate());
        const double cost_c = 0.5 * S.red[27];
        const bool finite = ctl::finite64(cost_c);
        if (ctm::sqrt64(step2) <= 1e-10 * (ctm::sqrt64(x2) + 1e-10)) break;
        const double cost_change = cost - cost_c;
        if (finite && ctm::fabs64(cost_change) <= 1e-15 * cost) break;
        const double rho = cost_change / model_cost_change;
        if (finite && rho > 1e-3) {
#pragma unroll
            for (int a = 0; a < 6; a++) x[a] = xc[a];
            take(H, g);
            cost = cost_c;
            const double t = 2.0 * rho - 1.0;
            double f = 1.0 - t * t * t;
            if (f < 1.0 / 3.0) f = 1.0 / 3.0;
            radius = radius / f;
            if (radius > 1e16) radius = 1e16;
            decrease_factor = 2.0;
            if (gradient_max() <= 1e-15) break;
        } else {
            radius = radius / decrease_factor;
            decrease_factor *= 2.0;
        }
    }
    PROF_MARK(8);
    iterations = iter;
    cost_start = cost0;
    cost_end = cost;
}

// the residual of one camera: what PoseBA fits in the per-marker and the rig pose
template <int PTS>
__device__ __forceinline__ auto camera_residual(const PoseLds<PTS>& S, const PoseCam& cam) {
    return [&S, &cam](int i, const double* R, const double* dR, const double* y, double& r0, double& r1, double* j0, double* j1) {
        point_residual(R, dR, y, cam.fx, cam.fy, cam.cx, cam.cy, S.X + 3 * i, S.OBS + 2 * i, r0, r1, j0, j1, true);
    };
}

// EPnP, then PoseBA.  Lane 0 writes the pose fields of *P: rvec0 tvec0 rvec tvec iterations cost0 cost, or status =
// CTAG_POSE_DEGENERATE (the other fields untouched) for a non-finite EPnP result.  Rec is ctag_pose_rec or ctag_rig_pose_rec.
// Every thread of the block calls it; it synchronises the block.
template <int PTS, int NT, class Rec>
__device__ __forceinline__ void pose_solve(PoseLds<PTS>& S, const int lane, const int n, const PoseCam& cam, Rec* __restrict__ P) {
    if (!pose_epnp<PTS, NT>(S, lane, n, cam)) {
        if (lane == 0) P->status = CTAG_POSE_DEGENERATE;
        return;
    }
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = S.x[i];
    if (lane == 0)
        for (int i = 0; i < 3; i++) {
            P->rvec0[i] = x[i];
            P->tvec0[i] = x[3 + i];
        }
    int iter;
    double cost0, cost;
    pose_ba<PTS, NT>(S, lane, n, x, camera_residual(S, cam), iter, cost0, cost);
    if (lane == 0) {
        for (int i = 0; i < 3; i++) {
            P->rvec[i] = x[i];
            P->tvec[i] = x[3 + i];
        }
        P->iterations = iter;
        P->cost0 = cost0;
        P->cost = cost;
    }
}

// ---- several cameras (k_mv_pose.hip, k_pose_cov.hip) --------------------------------------------------------------------------
constexpr int kMvCams = CTAG_MV_MAX_CAMERAS;

// the camera set as the kernels take it, by value
struct MvCams {
    int n;
    int at_reference[kMvCams];  // the camera's pose is exactly zero: its frame is the reference frame
    PoseCam cam[kMvCams];
    double R[kMvCams][9];  // Rc = R(rvec), row-major
    double t[kMvCams][3];  // tc
};

struct MvResults {
    const ctag_frame_result* p[kMvCams];  // device pointers, n_frames records each
};

// residual and Jacobian rows of point p seen by a camera at (Rc, tc) in the reference frame, under the rig pose (R, dR, x):
// Q = Rc (R p + t) + tc, the projection of point_residual on Q, and Rc applied to the rows point_residual forms
__device__ __forceinline__ void mv_point_residual(const double* R, const double* dR, const double* x, const PoseCam& cam, const double* Rc,
                                                  const double* tc, const double* p, const double* ob, double& r0, double& r1, double* j0,
                                                  double* j1) {
    const double P0 = (R[0] * p[0] + R[1] * p[1] + R[2] * p[2]) + x[3];
    const double P1 = (R[3] * p[0] + R[4] * p[1] + R[5] * p[2]) + x[4];
    const double P2 = (R[6] * p[0] + R[7] * p[1] + R[8] * p[2]) + x[5];
    const double Q0 = (Rc[0] * P0 + Rc[1] * P1 + Rc[2] * P2) + tc[0];
    const double Q1 = (Rc[3] * P0 + Rc[4] * P1 + Rc[5] * P2) + tc[1];
    const double Q2 = (Rc[6] * P0 + Rc[7] * P1 + Rc[8] * P2) + tc[2];
    const double iz = 1.0 / Q2;
    r0 = (cam.fx * (Q0 * iz) + cam.cx) - ob[0];
    r1 = (cam.fy * (Q1 * iz) + cam.cy) - ob[1];
    const double a0 = cam.fx * iz, a1 = cam.fy * iz;
    const double b0 = cam.fx * Q0 * iz * iz, b1 = cam.fy * Q1 * iz * iz;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double* D = dR + 9 * k;
        const double d0 = D[0] * p[0] + D[1] * p[1] + D[2] * p[2];
        const double d1 = D[3] * p[0] + D[4] * p[1] + D[5] * p[2];
        const double d2 = D[6] * p[0] + D[7] * p[1] + D[8] * p[2];
        const double e0 = Rc[0] * d0 + Rc[1] * d1 + Rc[2] * d2;
        const double e1 = Rc[3] * d0 + Rc[4] * d1 + Rc[5] * d2;
        const double e2 = Rc[6] * d0 + Rc[7] * d1 + Rc[8] * d2;
        j0[k] = a0 * e0 - b0 * e2;
        j1[k] = a1 * e1 - b1 * e2;
    }
#pragma unroll
    for (int m = 0; m < 3; m++) {  // dQ/dt = Rc
        j0[3 + m] = a0 * Rc[m] - b0 * Rc[6 + m];
        j1[3 + m] = a1 * Rc[3 + m] - b1 * Rc[6 + m];
    }
}

}  // namespace ctag

// ctag_camera_set (opaque in include/ctag_pose.h)
struct ctag_camera_set {
    ctag::MvCams dev;
    ctag_camera cameras[CTAG_MV_MAX_CAMERAS];  // what the set was created from, for ctag_camera_set_get: entries 0 .. dev.n - 1
    ctag_camera_pose poses[CTAG_MV_MAX_CAMERAS];
};
