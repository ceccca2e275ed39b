// k_intr_fit.hip -- the intrinsics of one camera (fx fy cx cy and up to twelve distortion coefficients) from the detection records of
// views of rigs whose models are known, on the device.  The semantics are stated in include/ctag_pose.h (intrinsics fit, rules 1-8).
//
// Mapping.  The forward reprojection problem over the camera and every view's rig pose separates: given the
// camera a view's pose is a six-parameter minimisation of its own, so a round is
//   pose      k_ifit_pose: one wavefront per observation record, grid-stride.  Damped Gauss-Newton on the record's (rvec, tvec) from
//             its accepted pose; lane l owns the points l, l + 64, ... and the 21 + 6 + 1 sums of a step go through wave_sum_f64
//             (pose_block6's shape).  The record is updated in place: rvec, tvec, cost;
//   record    k_ifit_record: one wavefront per observation record, grid-stride.  Tiles of 64 points: every lane writes its point's two
//             rows (r | Jp | Jc, 23 columns each) to LDS at an odd stride, then every lane adds, point after point, the products of
//             the at most five entries it owns of the 23 x 23 Gram matrix of those rows (276 upper entries: 2 cost, Jp^T r, U,
//             Jc^T r, Jp^T Jc, Jc^T Jc).  No wave reduction: the order of every sum is the point order by construction.  Then every lane
//             factors U = L L^T (chol6), lanes 0-15 take a column of Z = L^-1 Jp^T Jc each (forward6_dot), and the 136 + 16 reduced
//             entries S_r = Jc^T Jc - Z^T Z, g_r = Jc^T r - Z^T y go to the workspace;
//   assemble  k_ifit_assemble: one thread per entry, records in record order, the running sums in global memory between the passes
//             of the workspace, so the result does not depend on the pass size;
//   solve     k_ifit_solve: one wavefront, (S + lambda diag S) over the free rows as a 16 x 16 in LDS, fixed parameters as identity
//             rows with a zero right-hand side, right-looking Cholesky, the two triangular solves on lane 0.
// The host decides (accept / reject, lambda, stop: fit::Lm) between the launches and forms the float32 trial camera.  FP64 VALU like the
// pose kernels; nothing here is MFMA-shaped.  The walk is the one of the rig assembly and the camera set fit (fit_member_walk,
// ctag_pose_dev.h, as are point_desc and load_state6);
// corner_pixel (ctag_pose_dev.h) gives the raw pixel; chol6, forward6, backward6 and forward6_dot are ctag_schur6.h's, the host side of a fit
// (timed state, call context, systems with their pass loop, the accept / reject rule) is ctag_fit_host.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_fit_host.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"
#include "ctag_schur6.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_intrinsics_fit_opts) == 40, "ctag_intrinsics_fit_opts layout");
static_assert(sizeof(ctag_intrinsics_fit_stat) == 200, "ctag_intrinsics_fit_stat layout");
static_assert(CTAG_INTR_PARAMS == 16, "the record kernel's column layout");

namespace ctag {

constexpr int kIfitGrid = 256;          // wavefronts of one k_ifit_pose / k_ifit_record launch at most
constexpr int kIfitPassRecords = 512;   // observation records one pass of the workspace holds
constexpr int kIfitN = CTAG_INTR_PARAMS;
constexpr int kIfitCols = 1 + 6 + kIfitN;                  // a row of a point: r | Jp | Jc
constexpr int kIfitStride = 2 * kIfitCols + 1;             // 47 doubles a point: odd, lane-per-point writes without bank conflicts
constexpr int kIfitGram = kIfitCols * (kIfitCols + 1) / 2; // 276: the upper triangle of the rows' Gram matrix, in row order
constexpr int kIfitOwned = (kIfitGram + 63) / 64;          // 5 entries a lane at most
constexpr int kIfitUpper = kIfitN * (kIfitN + 1) / 2;      // 136: the upper triangle of S_r in row order
constexpr int kIfitDoubles = kIfitUpper + kIfitN;          // per record of a pass: S_r, then g_r
constexpr int kRecUnusable = 4;  // flags of a record beside kRecLeftOut / kRecSingular: a point of it is unusable under this state (rule 2)
// rule 4's constants
constexpr double kIfitMu0 = 1e-4, kIfitMuMax = 1e8, kIfitPoseTol = 1e-15;
constexpr int kIfitPoseSteps = 40;

struct IfitWalk {
    int32_t src[kFitMaxPts];  // point i: its descriptor (point_desc, ctag_pose_dev.h; camera 0)
    int16_t mdl[kFitMaxPts];  // ... and its model index
};

// index of (a, b), a <= b, in the upper triangle of an n x n in row order
__host__ __device__ constexpr int upper_index(int n, int a, int b) { return a * n - a * (a - 1) / 2 + (b - a); }

// The points of rig pose record P in the builder's order (fit_member_walk, ctag_pose_dev.h); false when the record does not describe
// its detection record.  Wave-uniform.
__device__ __forceinline__ bool ifit_walk(const ctag_frame_result* __restrict__ res, int n_frames, const ctag_rig_pose_rec& P, const PoseModelDev& model, int lane,
                                          IfitWalk& W, int& n) {
    n = 0;
    if (P.status != CTAG_POSE_OK || P.frame < 0 || P.frame >= n_frames || model.n_models > 32767) return false;
    const ctag_frame_result& FR = res[P.frame];
    if (FR.status != CTAG_OK) return false;
    const bool ok = fit_member_walk(FR, P.member_mask, model, lane, 0, n, [](int, int) { return true; }, [&](int i, int32_t desc, int mi) {
        W.src[i] = desc;
        W.mdl[i] = (int16_t)mi;
    });
    return ok && n == P.n_points && n >= 4;
}

// Rule 2 at one point: the residual (q0, q1) of model point X seen at pixel uv under pose (R, dR, x) and camera c, the rows of Jp
// (j0, j1: rvec, tvec) and, WITH_JC, of Jc (c0, c1: the 16 parameters; tie != 0: the fx column carries tie x the fy column).  False
// for an unusable point: nothing else is written then.
template <bool WITH_JC>
__device__ __forceinline__ bool ifit_point(const PoseCam& c, double tie, const double* R, const double* dR, const double* x, const double* X, const double* uv,
                                           double& q0, double& q1, double* j0, double* j1, double* c0, double* c1) {
    const double P0 = (R[0] * X[0] + R[1] * X[1] + R[2] * X[2]) + x[3];
    const double P1 = (R[3] * X[0] + R[4] * X[1] + R[5] * X[2]) + x[4];
    const double P2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + x[5];
    if (!(P2 > 0.0)) return false;
    const double iz = 1.0 / P2;
    const double a = P0 * iz, b = P1 * iz;
    const double r2 = a * a + b * b, r4 = r2 * r2, r6 = r4 * r2;
    const double* k = c.k;
    const double num = 1.0 + k[0] * r2 + k[1] * r4 + k[4] * r6;
    const double den = 1.0 + k[5] * r2 + k[6] * r4 + k[7] * r6;
    if (!(den > 0.0)) return false;
    const double id = 1.0 / den, rad = num * id;
    const double a1 = 2.0 * a * b, a2 = r2 + 2.0 * a * a, a3 = r2 + 2.0 * b * b;
    const double xd = a * rad + k[2] * a1 + k[3] * a2 + k[8] * r2 + k[9] * r4;
    const double yd = b * rad + k[2] * a3 + k[3] * a1 + k[10] * r2 + k[11] * r4;
    const double e0 = (c.fx * xd + c.cx) - uv[0], e1 = (c.fy * yd + c.cy) - uv[1];
    if (!ctl::finite64(e0) || !ctl::finite64(e1)) return false;
    q0 = e0;
    q1 = e1;
    // d rad / d r2, then the 2 x 2 derivative of (xd, yd) in (a, b)
    const double drad = ((k[0] + 2.0 * k[1] * r2 + 3.0 * k[4] * r4) - rad * (k[5] + 2.0 * k[6] * r2 + 3.0 * k[7] * r4)) * id;
    const double dxx = rad + 2.0 * a * a * drad + 2.0 * k[2] * b + 6.0 * k[3] * a + 2.0 * k[8] * a + 4.0 * k[9] * r2 * a;
    const double dxy = 2.0 * a * b * drad + 2.0 * k[2] * a + 2.0 * k[3] * b + 2.0 * k[8] * b + 4.0 * k[9] * r2 * b;
    const double dyx = 2.0 * a * b * drad + 2.0 * k[2] * a + 2.0 * k[3] * b + 2.0 * k[10] * a + 4.0 * k[11] * r2 * a;
    const double dyy = rad + 2.0 * b * b * drad + 6.0 * k[2] * b + 2.0 * k[3] * a + 2.0 * k[10] * b + 4.0 * k[11] * r2 * b;
    // d residual / d P
    const double g0[3] = {c.fx * dxx * iz, c.fx * dxy * iz, -(c.fx * (dxx * a + dxy * b) * iz)};
    const double g1[3] = {c.fy * dyx * iz, c.fy * dyy * iz, -(c.fy * (dyx * a + dyy * b) * iz)};
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const double* D = dR + 9 * m;
        const double d0 = D[0] * X[0] + D[1] * X[1] + D[2] * X[2];
        const double d1 = D[3] * X[0] + D[4] * X[1] + D[5] * X[2];
        const double d2 = D[6] * X[0] + D[7] * X[1] + D[8] * X[2];
        j0[m] = g0[0] * d0 + g0[1] * d1 + g0[2] * d2;
        j1[m] = g1[0] * d0 + g1[1] * d1 + g1[2] * d2;
        j0[3 + m] = g0[m];
        j1[3 + m] = g1[m];
    }
    if constexpr (WITH_JC) {
        const double fa = c.fx * a * id, fb = c.fy * b * id;  // d (fx a rad) / d num, d (fy b rad) / d num
        c0[0] = xd, c1[0] = tie * yd;
        c0[1] = 0.0, c1[1] = yd;
        c0[2] = 1.0, c1[2] = 0.0;
        c0[3] = 0.0, c1[3] = 1.0;
        c0[4] = fa * r2, c1[4] = fb * r2;     // k1
        c0[5] = fa * r4, c1[5] = fb * r4;     // k2
        c0[6] = c.fx * a1, c1[6] = c.fy * a3; // p1
        c0[7] = c.fx * a2, c1[7] = c.fy * a1; // p2
        c0[8] = fa * r6, c1[8] = fb * r6;     // k3
        c0[9] = -(fa * rad * r2), c1[9] = -(fb * rad * r2);    // k4
        c0[10] = -(fa * rad * r4), c1[10] = -(fb * rad * r4);  // k5
        c0[11] = -(fa * rad * r6), c1[11] = -(fb * rad * r6);  // k6
        c0[12] = c.fx * r2, c1[12] = 0.0;  // s1
        c0[13] = c.fx * r4, c1[13] = 0.0;  // s2
        c0[14] = 0.0, c1[14] = c.fy * r2;  // s3
        c0[15] = 0.0, c1[15] = c.fy * r4;  // s4
    }
    return true;
}

// Rule 4 on observation records 0 .. n_obs-1 (indices into obs), in place: recs[obs[r]] gets rvec, tvec and cost; pflags[r] = 0, or
// kRecLeftOut / kRecUnusable when the record's start cannot be evaluated (the record is left as it was).
__global__ __launch_bounds__(64) void k_ifit_pose(const ctag_frame_result* __restrict__ res, int n_frames, ctag_rig_pose_rec* __restrict__ recs,
                                                  const int32_t* __restrict__ obs, int n_obs, PoseModelDev model, PoseCam cam, int32_t* __restrict__ pflags) {
    __shared__ IfitWalk W;
    const int lane = threadIdx.x;
    for (int r = (int)blockIdx.x; r < n_obs; r += gridDim.x) {
        ctag_rig_pose_rec& P = recs[obs[r]];
        wave_sync();  // the previous record's LDS reads are done
        int n;
        bool ok = ifit_walk(res, n_frames, P, model, lane, W, n);
        double x[6];
        ok = load_state6(P, x) && ok;
        wave_sync();
        if (!ok) {  // wave-uniform
            if (lane == 0) pflags[r] = kRecLeftOut;
            continue;
        }
        const ctag_frame_result& FR = res[P.frame];
        // the sums of a step at pose xs: U (21), sum Jp^T r (6), the cost; false when a point is unusable there
        auto eval = [&](const double* xs, double* H, double* b, double& cost) {
            double R[9], dR[27];
            ctl::angle_axis_rot(xs, R, dR);
#pragma unroll
            for (int e = 0; e < 21; e++) H[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) b[e] = 0.0;
            double c = 0.0, bad = 0.0;
            for (int i = lane; i < n; i += 64) {
                const int s = W.src[i];
                double uv[2], X[3], q0, q1, j0[6], j1[6];
                corner_pixel(model.corners + (size_t)W.mdl[i] * model.model_size * 24, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), uv, X);
                if (!ifit_point<false>(cam, 0.0, R, dR, xs, X, uv, q0, q1, j0, j1, nullptr, nullptr)) {
                    bad = 1.0;
                    continue;
                }
                gram6_add(j0, j1, H);
                grad6_add(j0, j1, q0, q1, b);
                c += q0 * q0;
                c += q1 * q1;
            }
#pragma unroll
            for (int e = 0; e < 21; e++) H[e] = wave_sum_f64(H[e]);
#pragma unroll
            for (int e = 0; e < 6; e++) b[e] = wave_sum_f64(b[e]);
            cost = 0.5 * wave_sum_f64(c);
            return wave_sum_f64(bad) == 0.0 && ctl::finite64(cost);
        };
        double H[21], b[6], cost;
        if (!eval(x, H, b, cost)) {  // wave-uniform, like everything below
            if (lane == 0) pflags[r] = kRecUnusable;
            continue;
        }
        double mu = kIfitMu0;
        for (int it = 0; it < kIfitPoseSteps && cost > 0.0 && mu <= kIfitMuMax; it++) {
            double Hd[21], Lc[36], d[6], xt[6], Ht[21], bt[6], ct = 0.0;
#pragma unroll
            for (int e = 0; e < 21; e++) Hd[e] = H[e];
#pragma unroll
            for (int a = 0; a < 6; a++) Hd[upper_index(6, a, a)] = H[upper_index(6, a, a)] + mu * H[upper_index(6, a, a)];
            bool good = chol6(Hd, Lc);
            if (good) {
#pragma unroll
                for (int a = 0; a < 6; a++) d[a] = -b[a];
                forward6(Lc, d);
                backward6(Lc, d);
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    xt[a] = x[a] + d[a];
                    good = good && ctl::finite64(xt[a]);
                }
                good = good && eval(xt, Ht, bt, ct) && ct < cost;
            }
            if (!good) {
                mu *= 4.0;
                continue;
            }
            const double drop = cost - ct;
#pragma unroll
            for (int e = 0; e < 21; e++) H[e] = Ht[e];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                b[a] = bt[a];
                x[a] = xt[a];
            }
            cost = ct;
            mu = mu / 3.0;
            if (drop < kIfitPoseTol * cost) break;
        }
        if (lane == 0) {
            for (int a = 0; a < 3; a++) {
                P.rvec[a] = x[a];
                P.tvec[a] = x[3 + a];
            }
            P.cost = cost;
            pflags[r] = 0;
        }
    }
}

struct IfitLds {
    IfitWalk W;
    double rows[64 * kIfitStride];  // a tile: point p's two rows at p * kIfitStride and p * kIfitStride + kIfitCols
    double G[kIfitGram];            // the record's Gram matrix
    double Z[6 * kIfitN];           // Z = L^-1 Jp^T Jc, row-major 6 x 16
};

// Observation records r0 .. r1-1 (indices into obs): workspace slot r - r0 gets the record's 136 + 16 reduced entries, flags[r] its
// state (0, kRecLeftOut, kRecSingular, kRecUnusable).
__global__ __launch_bounds__(64) void k_ifit_record(const ctag_frame_result* __restrict__ res, int n_frames, const ctag_rig_pose_rec* __restrict__ recs,
                                                    const int32_t* __restrict__ obs, int r0, int r1, PoseModelDev model, PoseCam cam, double tie,
                                                    double* __restrict__ ws, int32_t* __restrict__ flags) {
    __shared__ IfitLds L;
    const int lane = threadIdx.x;
    int ea[kIfitOwned], eb[kIfitOwned];  // the columns (a <= b) of the Gram entries lane, lane + 64, ... this lane owns; a = -1: none
#pragma unroll
    for (int k = 0; k < kIfitOwned; k++) {
        int rem = lane + 64 * k, a = 0;
        while (a < kIfitCols && rem >= kIfitCols - a) {
            rem -= kIfitCols - a;
            a++;
        }
        ea[k] = a < kIfitCols ? a : -1;
        eb[k] = a < kIfitCols ? a + rem : 0;
    }
    for (int r = r0 + (int)blockIdx.x; r < r1; r += gridDim.x) {
        const ctag_rig_pose_rec& P = recs[obs[r]];
        wave_sync();  // the previous record's LDS reads are done
        int n;
        bool ok = ifit_walk(res, n_frames, P, model, lane, L.W, n);
        double x[6];
        ok = load_state6(P, x) && ok;
        wave_sync();
        if (!ok) {  // wave-uniform
            if (lane == 0) flags[r] = kRecLeftOut;
            continue;
        }
        const ctag_frame_result& FR = res[P.frame];
        double R[9], dR[27];
        ctl::angle_axis_rot(x, R, dR);
        double acc[kIfitOwned];
#pragma unroll
        for (int k = 0; k < kIfitOwned; k++) acc[k] = 0.0;
        double bad = 0.0;
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int i = t0 + lane;
            if (i < n) {
                const int s = L.W.src[i];
                double uv[2], X[3], q0 = 0.0, q1 = 0.0;
                corner_pixel(model.corners + (size_t)L.W.mdl[i] * model.model_size * 24, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), uv, X);
                double* row = L.rows + lane * kIfitStride;  // the point's rows are formed where they lie
                if (ifit_point<true>(cam, tie, R, dR, x, X, uv, q0, q1, row + 1, row + kIfitCols + 1, row + 7, row + kIfitCols + 7)) {
                    row[0] = q0;
                    row[kIfitCols] = q1;
                } else {
                    bad = 1.0;
                    for (int a = 0; a < 2 * kIfitCols; a++) row[a] = 0.0;
                }
            }
            wave_sync();
            const int m = min(64, n - t0);
            for (int p = 0; p < m; p++) {  // the tile's points in point order
                const double* row = L.rows + p * kIfitStride;
#pragma unroll
                for (int k = 0; k < kIfitOwned; k++)
                    if (ea[k] >= 0) {
                        acc[k] += row[ea[k]] * row[eb[k]];
                        acc[k] += row[kIfitCols + ea[k]] * row[kIfitCols + eb[k]];
                    }
            }
            wave_sync();
        }
        if (wave_sum_f64(bad) != 0.0) {  // wave-uniform
            if (lane == 0) flags[r] = kRecUnusable;
            continue;
        }
#pragma unroll
        for (int k = 0; k < kIfitOwned; k++)
            if (ea[k] >= 0) L.G[lane + 64 * k] = acc[k];
        wave_sync();
        // every lane: U = L L^T and y = L^-1 sum Jp^T r
        double H[21], y[6], Lc[36];
        {
            int e = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int c = a; c < 6; c++) H[e++] = L.G[upper_index(kIfitCols, 1 + a, 1 + c)];
                y[a] = L.G[upper_index(kIfitCols, 0, 1 + a)];
            }
        }
        const bool pd = chol6(H, Lc);  // the same in every lane
        if (lane == 0) flags[r] = pd ? 0 : kRecSingular;
        if (!pd) continue;
        forward6(Lc, y);
        double* O = ws + (size_t)(r - r0) * kIfitDoubles;
        if (lane < kIfitN) {  // column `lane` of Z, and g_r's entry
            double z[6];
#pragma unroll
            for (int a = 0; a < 6; a++) z[a] = L.G[upper_index(kIfitCols, 1 + a, 7 + lane)];
            const double gj = L.G[upper_index(kIfitCols, 0, 7 + lane)] - forward6_dot(Lc, z, y);
#pragma unroll
            for (int a = 0; a < 6; a++) L.Z[a * kIfitN + lane] = z[a];
            O[kIfitUpper + lane] = gj;
        }
        wave_sync();
        for (int e = lane; e < kIfitUpper; e += 64) {
            int rem = e, i = 0;
            while (rem >= kIfitN - i) {
                rem -= kIfitN - i;
                i++;
            }
            const int j = i + rem;
            double zz = 0.0;
#pragma unroll
            for (int a = 0; a < 6; a++) zz += L.Z[a * kIfitN + i] * L.Z[a * kIfitN + j];
            O[e] = L.G[upper_index(kIfitCols, 7 + i, 7 + j)] - zz;
        }
    }
}

// Adds records r0 .. r1-1 to S [16 x 16, both triangles] and g [16]: thread t < 136 owns entry t of the upper triangle in row order,
// 136 <= t < 152 entry t - 136 of g.
__global__ __launch_bounds__(256) void k_ifit_assemble(const double* __restrict__ ws, const int32_t* __restrict__ flags, int r0, int r1, double* __restrict__ S,
                                                       double* __restrict__ g) {
    const int t = threadIdx.x;
    if (t >= kIfitDoubles) return;
    int i = 0, j = 0;
    if (t < kIfitUpper) {
        int rem = t;
        while (rem >= kIfitN - i) {
            rem -= kIfitN - i;
            i++;
        }
        j = i + rem;
    }
    double* dst = t < kIfitUpper ? S + i * kIfitN + j : g + (t - kIfitUpper);
    double acc = *dst;
    for (int r = r0; r < r1; r++) {
        if (flags[r] != 0) continue;
        acc += ws[(size_t)(r - r0) * kIfitDoubles + t];
    }
    *dst = acc;
    if (t < kIfitUpper && i != j) S[j * kIfitN + i] = acc;
}

// (S + lambda diag S) delta = -g over the rows whose bit is set in `mask`; the other rows are identity rows with a zero right-hand
// side.  bad[0] = 1 for a pivot that is not positive (delta stays as it was).  Not k_fit_solve (ctag_fit_solve.h), on purpose: the
// two triangular solves run row by row here and column by column there, which subtracts in another order per element.
__global__ __launch_bounds__(64) void k_ifit_solve(const double* __restrict__ S, const double* __restrict__ g, const double* __restrict__ lambda,
                                                   const int32_t* __restrict__ active, uint32_t mask, double* __restrict__ delta, int32_t* __restrict__ bad) {
    __shared__ double A[kIfitN][kIfitN + 1];
    __shared__ double rhs[kIfitN];
    if (!active[0]) return;
    const int lane = threadIdx.x;
    const double lam = lambda[0];
    for (int e = lane; e < kIfitN * kIfitN; e += 64) {
        const int i = e / kIfitN, j = e - i * kIfitN;
        const bool fi = (mask >> i) & 1u, fj = (mask >> j) & 1u;
        double v = i == j ? 1.0 : 0.0;
        if (fi && fj) v = i == j ? S[e] + lam * S[e] : S[e];
        A[i][j] = v;
    }
    if (lane < kIfitN) rhs[lane] = ((mask >> lane) & 1u) ? -g[lane] : 0.0;
    __syncthreads();
    bool pd = true;
    for (int j = 0; j < kIfitN; j++) {
        double d = A[j][j];
        if (!(d > 0.0) || !ctl::finite64(d)) pd = false;
        d = ctm::sqrt64(d);
        __syncthreads();
        if (lane == j) A[j][j] = d;
        if (lane > j && lane < kIfitN) A[lane][j] = A[lane][j] / d;
        __syncthreads();
        if (lane > j && lane < kIfitN)
            for (int k = j + 1; k <= lane; k++) A[lane][k] -= A[lane][j] * A[k][j];
        __syncthreads();
    }
    if (lane != 0) return;
    if (!pd) {
        bad[0] = 1;
        return;
    }
    double x[kIfitN];
    for (int i = 0; i < kIfitN; i++) {
        double s = rhs[i];
        for (int k = 0; k < i; k++) s -= A[i][k] * x[k];
        x[i] = s / A[i][i];
    }
    for (int i = kIfitN - 1; i >= 0; i--) {
        double s = x[i];
        for (int k = i + 1; k < kIfitN; k++) s -= A[k][i] * x[k];
        x[i] = s / A[i][i];
    }
    for (int i = 0; i < kIfitN; i++) delta[i] = x[i];
}

}  // namespace ctag

// =====================================================================================================
// host side: what the fits share is ctag_fit_host.h's (namespace ctag::fit)
// =====================================================================================================
namespace {

namespace fit = ctag::fit;
constexpr int kN = ctag::kIfitN;

// The device side of one call: the one system (group 0), the record workspace, the view poses' flags.
struct IfitWork : fit::Systems {
    fit::Call c;
    uint32_t mask = 0;  // the free parameters
    double tie = 0.0;   // rule 5's ratio, 0 without tie_focal
    std::vector<int32_t> pflags;
    ctag::DevBuf<int32_t> d_pflags;
    ctag::DevBuf<double> d_ws;

    int setup(int pass_records) {
        const int rc = Systems::setup(c, 1, kN, pass_records, ctag::kIfitPassRecords);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_pflags.grow((size_t)std::max(R, 1)));
        FIT_HIP(d_ws.grow((size_t)pass * ctag::kIfitDoubles));
        pflags.assign(R, 0);
        return CTAG_OK;
    }

    static ctag::PoseModelDev dev_model(const ctag_model* model) { return ctag::PoseModelDev{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p}; }

    // rule 4 on every observation record of recs_dev, in place, under cam (timed in slot 1); *usable = every record could be evaluated.  Waits.
    int view_poses(const ctag_model* model, const ctag::PoseCam& cam, ctag_rig_pose_rec* recs_dev, bool* usable) {
        *usable = true;
        if (R == 0) return CTAG_OK;
        if (c.mark(0) != CTAG_OK) return CTAG_ERR_HIP;
        hipLaunchKernelGGL(ctag::k_ifit_pose, dim3(std::min(R, ctag::kIfitGrid)), dim3(64), 0, c.s, c.res, c.n_frames, recs_dev, d_obs.p, R, dev_model(model), cam, d_pflags.p);
        if (fit::launched() != CTAG_OK || c.mark(1) != CTAG_OK) return CTAG_ERR_HIP;
        FIT_HIP(hipMemcpyAsync(pflags.data(), d_pflags.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, c.s));
        FIT_HIP(hipStreamSynchronize(c.s));
        c.add_ms(1, 0);
        for (int32_t f : pflags)
            if (f != 0) *usable = false;
        return CTAG_OK;
    }

    // S and g at (cam, recs_dev).  Waits.
    int build_system(const ctag_model* model, const ctag::PoseCam& cam, const ctag_rig_pose_rec* recs_dev) {
        const ctag::PoseModelDev md = dev_model(model);
        return build_timed(c, [&](int r0, int r1) {
            hipLaunchKernelGGL(ctag::k_ifit_record, dim3(std::min(r1 - r0, ctag::kIfitGrid)), dim3(64), 0, c.s, c.res, c.n_frames, recs_dev, d_obs.p, r0, r1, md, cam, tie,
                               d_ws.p, d_flags.p);
            hipLaunchKernelGGL(ctag::k_ifit_assemble, dim3(1), dim3(256), 0, c.s, d_ws.p, d_flags.p, r0, r1, d_S.p, d_g.p);
        });
    }

    int solve(const std::vector<double>& lambda, const std::vector<int32_t>& active, std::vector<double>& delta, std::vector<int32_t>& bad) {
        // every observation record's pose was solved on this state, so one that is flagged at all makes the system bad
        return Systems::solve(c, lambda, active, ~0, delta, bad, [&]() {
            hipLaunchKernelGGL(ctag::k_ifit_solve, dim3(1), dim3(64), 0, c.s, d_S.p, d_g.p, d_lambda.p, d_active.p, mask, d_delta.p, d_bad.p);
        });
    }

    int fetch_S(double* S) {
        FIT_HIP(hipMemcpy(S, d_S.p, sizeof(double) * kN * kN, hipMemcpyDeviceToHost));
        return CTAG_OK;
    }
};

// parameter order of CTAG_INTR_PARAMS
void params_of(const ctag_camera& c, double* p) {
    p[0] = c.K[0], p[1] = c.K[4], p[2] = c.K[2], p[3] = c.K[5];
    for (int i = 0; i < 12; i++) p[4 + i] = i < c.n_dist ? (double)c.dist[i] : 0.0;
}

// rule 3: the trial's doubles rounded to the camera's floats
void set_params(ctag_camera& c, const double* p) {
    c.K[0] = (float)p[0], c.K[4] = (float)p[1], c.K[2] = (float)p[2], c.K[5] = (float)p[3];
    for (int i = 0; i < 12 && i < c.n_dist; i++) c.dist[i] = (float)p[4 + i];
}

bool camera_usable(const ctag_camera& c) {
    bool ok = std::isfinite(c.K[0]) && std::isfinite(c.K[4]) && c.K[0] > 0.f && c.K[4] > 0.f && std::isfinite(c.K[2]) && std::isfinite(c.K[5]);
    for (int i = 0; i < 12 && i < c.n_dist; i++) ok = ok && std::isfinite(c.dist[i]);
    return ok;
}

// the diagonal of the inverse of S over the rows of `mask` (0 elsewhere), by Cholesky in double; false on a pivot that is not positive
bool inverse_diagonal(const double* S, uint32_t mask, double* diag) {
    int idx[kN], n = 0;
    for (int i = 0; i < kN; i++) {
        diag[i] = 0.0;
        if ((mask >> i) & 1u) idx[n++] = i;
    }
    double Lm[kN][kN] = {};
    for (int j = 0; j < n; j++) {
        double d = S[idx[j] * kN + idx[j]];
        for (int k = 0; k < j; k++) d -= Lm[j][k] * Lm[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        Lm[j][j] = std::sqrt(d);
        for (int i = j + 1; i < n; i++) {
            double s = S[idx[i] * kN + idx[j]];
            for (int k = 0; k < j; k++) s -= Lm[i][k] * Lm[j][k];
            Lm[i][j] = s / Lm[j][j];
        }
    }
    for (int c = 0; c < n; c++) {  // column c of L^-1; (S^-1)_cc = its squared norm
        double x[kN] = {};
        double s2 = 0.0;
        for (int i = c; i < n; i++) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; k++) s -= Lm[i][k] * x[k];
            x[i] = s / Lm[i][i];
            s2 += x[i] * x[i];
        }
        diag[idx[c]] = s2;
    }
    return true;
}

int ifit_opts(const ctag_intrinsics_fit_opts* o, const ctag_camera* seed, ctag_intrinsics_fit_opts& r, uint32_t& mask, double& tie) {
    ctag_intrinsics_fit_opts_default(&r);
    if (o) r = *o;
    if (r.max_rounds < 0 || r.min_points < 1 || !fit::lm_opts_ok(r)) return CTAG_ERR_ARG;
    const int nd = std::min(std::max(seed->n_dist, 0), 12);
    mask = r.free_mask;
    if (mask == 0u) mask = (1u << (4 + nd)) - 1u;
    if (mask >> (4 + nd)) return CTAG_ERR_ARG;  // a bit at or above CTAG_INTR_PARAMS, or on a coefficient the seed does not have
    tie = 0.0;
    if (r.tie_focal) {
        mask &= ~2u;
        tie = (double)seed->K[4] / (double)seed->K[0];
        if (!std::isfinite(tie) || !(tie > 0.0)) return CTAG_ERR_ARG;
    }
    return mask ? CTAG_OK : CTAG_ERR_ARG;
}

int popcount16(uint32_t m) {
    int n = 0;
    for (int i = 0; i < kN; i++) n += (m >> i) & 1u;
    return n;
}

}  // namespace

namespace ctag {

int ifit_record_grid() { return kIfitGrid; }
int ifit_pass_records() { return kIfitPassRecords; }

// what the two probes share: the call's context, the caller's records on the device, the observation set (every CTAG_POSE_OK record
// with at least min_points points)
static int ifit_probe_prepare(IfitWork& w, ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* recs, size_t n_items,
                              const ctag_model* model_c, const ctag_camera* camera, int min_points, DevBuf<ctag_frame_result>& d_res, DevBuf<ctag_rig_pose_rec>& d_recs) {
    if (!camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    int rc = w.c.prepare(h, kIntrFitState, nullptr, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    if (model_to_device(const_cast<ctag_model*>(model_c), handle_device(h)) != CTAG_OK) return CTAG_ERR_HIP;
    rc = fit::upload_probe_inputs(w.c, results, d_res, recs, n_items, d_recs);
    if (rc != CTAG_OK) return rc;
    for (size_t i = 0; i < n_items; i++)
        if (recs[i].status == CTAG_POSE_OK && recs[i].n_points >= min_points) {
            w.obs.push_back((int32_t)i);
            w.rec_group.push_back(0);
        }
    return w.obs.empty() ? CTAG_ERR_ARG : CTAG_OK;
}

int ifit_probe_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* recs, const ctag_model* model, const ctag_rigs* rigs,
                      const ctag_camera* camera, uint32_t free_mask, int tie_focal, double lambda, int pass_records, double* S, double* g, double* delta,
                      int32_t* n_free, int32_t* bad_pivot) {
    if (!h || !results || n_frames < 1 || !recs || !model || !rigs || !camera || !S || !g || !delta || !n_free || !bad_pivot || !std::isfinite(lambda)) return CTAG_ERR_ARG;
    if (rigs->n_models != model->n_models || (long long)n_frames * rigs->n_rigs > (1ll << 28)) return CTAG_ERR_ARG;
    ctag_intrinsics_fit_opts o, opts;
    ctag_intrinsics_fit_opts_default(&o);
    o.free_mask = free_mask;
    o.tie_focal = tie_focal;
    IfitWork w;
    if (ifit_opts(&o, camera, opts, w.mask, w.tie) != CTAG_OK) return CTAG_ERR_ARG;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<ctag_rig_pose_rec> d_recs;
    int rc = ifit_probe_prepare(w, h, results, n_frames, recs, (size_t)n_frames * rigs->n_rigs, model, camera, 1, d_res, d_recs);
    if (rc != CTAG_OK) return rc;
    rc = w.setup(pass_records);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(model, w.c.cam, d_recs.p);
    if (rc != CTAG_OK) return rc;
    std::vector<double> lam(1, lambda), d;
    std::vector<int32_t> active(1, 1), bad;
    rc = w.solve(lam, active, d, bad);
    if (rc != CTAG_OK) return rc;
    FIT_HIP(hipMemcpy(S, w.d_S.p, sizeof(double) * kIfitN * kIfitN, hipMemcpyDeviceToHost));
    FIT_HIP(hipMemcpy(g, w.d_g.p, sizeof(double) * kIfitN, hipMemcpyDeviceToHost));
    for (int i = 0; i < kIfitN; i++) delta[i] = d[i];
    *n_free = popcount16(w.mask);
    *bad_pivot = bad[0];
    return CTAG_OK;
}

int ifit_probe_poses(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* recs, const ctag_model* model, const ctag_rigs* rigs,
                     const ctag_camera* camera, ctag_rig_pose_rec* out, int32_t* usable) {
    if (!h || !results || n_frames < 1 || !recs || !model || !rigs || !camera || !out || !usable) return CTAG_ERR_ARG;
    if (rigs->n_models != model->n_models || (long long)n_frames * rigs->n_rigs > (1ll << 28)) return CTAG_ERR_ARG;
    const size_t n_items = (size_t)n_frames * rigs->n_rigs;
    IfitWork w;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<ctag_rig_pose_rec> d_recs;
    int rc = ifit_probe_prepare(w, h, results, n_frames, recs, n_items, model, camera, 1, d_res, d_recs);
    if (rc != CTAG_OK) return rc;
    rc = w.setup(0);
    if (rc != CTAG_OK) return rc;
    bool ok = false;
    rc = w.view_poses(model, w.c.cam, d_recs.p, &ok);
    if (rc != CTAG_OK) return rc;
    FIT_HIP(hipMemcpy(out, d_recs.p, sizeof(ctag_rig_pose_rec) * n_items, hipMemcpyDeviceToHost));
    *usable = ok ? 1 : 0;
    return CTAG_OK;
}

}  // namespace ctag

extern "C" {

void ctag_intrinsics_fit_opts_default(ctag_intrinsics_fit_opts* o) {
    if (!o) return;
    o->max_rounds = 30;
    o->min_points = 8;
    o->free_mask = 0;
    o->tie_focal = 0;
    o->lambda0 = 1e-3;
    o->lambda_max = 1e6;
    o->rel_tol = 7.71e-9;  // 4 x 1.928e-9: what a one-ulp move of one camera field does to the cost of a returned state through the view poses
}

int ctag_intrinsics_fit_last_ms(ctag_handle* h, float* out4) { return fit::last_ms(h, ctag::kIntrFitState, out4); }  // rig pose, view pose, record + assemble, solve

int ctag_intrinsics_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model_c, const ctag_rigs* rigs,
                               const ctag_camera* seed, const ctag_intrinsics_fit_opts* opts_in, ctag_camera* out, ctag_intrinsics_fit_stat* stat,
                               ctag_rig_pose_rec* poses_out) {
    if (!h || !results_dev || n_frames < 1 || !model_c || !rigs || !seed || !out || !stat) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(seed)) return CTAG_ERR_UNSUPPORTED;
    IfitWork w;
    ctag_intrinsics_fit_opts opts;
    if (ifit_opts(opts_in, seed, opts, w.mask, w.tie) != CTAG_OK) return CTAG_ERR_ARG;
    if (model_c->model_size != ctag::handle_dict_cols(h) || model_c->model_size > CTAG_MAX_CODE_POS) return CTAG_ERR_ARG;
    if (rigs->n_models != model_c->n_models) return CTAG_ERR_ARG;
    if ((long long)n_frames * CTAG_MAX_MARKERS > (1ll << 30) || (long long)n_frames * rigs->n_rigs > (1ll << 28)) return CTAG_ERR_LIMIT;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    int rc = w.c.prepare(h, ctag::kIntrFitState, results_dev, n_frames, seed);
    if (rc != CTAG_OK) return rc;
    const int n_free = popcount16(w.mask);
    std::memset(stat, 0, sizeof(*stat));
    stat->status = CTAG_POSE_NOT_SEEN;
    stat->n_free = n_free;
    stat->free_mask = w.mask;
    stat->lambda = opts.lambda0;
    *out = *seed;
    const size_t n_items = (size_t)n_frames * rigs->n_rigs;

    // ---- rule 1: the seed pass and the observation set
    ctag::DevBuf<ctag_rig_pose_rec> d_a, d_b;
    FIT_HIP(d_a.grow(n_items));
    FIT_HIP(d_b.grow(n_items));
    ctag_rig_pose_rec *d_acc = d_a.p, *d_trial = d_b.p;
    std::vector<ctag_rig_pose_rec> seed_recs, acc, trial;
    rc = w.c.pose_pass(0, [&]() { return ctag_rig_pose_batch_device(h, results_dev, n_frames, model, rigs, seed, d_acc); }, d_acc, n_items, seed_recs);
    if (rc != CTAG_OK) return rc;
    if (poses_out) std::memcpy(poses_out, seed_recs.data(), sizeof(ctag_rig_pose_rec) * n_items);
    for (size_t i = 0; i < n_items; i++)
        if (seed_recs[i].status == CTAG_POSE_OK && seed_recs[i].n_points >= opts.min_points) {
            w.obs.push_back((int32_t)i);
            w.rec_group.push_back(0);
            stat->n_records++;
            stat->n_points += seed_recs[i].n_points;
        }
    if (w.obs.empty()) return CTAG_OK;
    const long long dof = 2ll * stat->n_points - 6ll * stat->n_records - n_free;
    if (dof <= 0) {
        stat->status = CTAG_POSE_TOO_FEW;
        return CTAG_OK;
    }
    rc = w.setup(0);
    if (rc != CTAG_OK) return rc;

    // ---- round 0: the view poses under the seed, the system there
    ctag_camera cur = *seed, tri = *seed;
    bool usable = false;
    rc = w.view_poses(model, ctag::make_pose_cam(&cur), d_acc, &usable);
    if (rc != CTAG_OK) return rc;
    stat->status = CTAG_POSE_DEGENERATE;
    if (!usable) return CTAG_OK;
    if (w.c.fetch(d_acc, n_items, acc) != CTAG_OK) return CTAG_ERR_HIP;
    fit::Lm lm;
    lm.start(1, opts.lambda0);
    std::vector<uint8_t> all_ok;
    w.costs_of(acc, nullptr, lm.cost, all_ok);
    if (!std::isfinite(lm.cost[0])) return CTAG_OK;
    double S[kN * kN], diag[kN];
    rc = w.build_system(model, ctag::make_pose_cam(&cur), d_acc);
    if (rc != CTAG_OK) return rc;
    if (w.fetch_S(S) != CTAG_OK) return CTAG_ERR_HIP;
    bool flagged = false;
    for (int32_t f : w.flags) flagged = flagged || f != 0;
    if (flagged || !inverse_diagonal(S, w.mask, diag)) return CTAG_OK;
    stat->status = CTAG_POSE_OK;
    stat->cost0 = lm.cost[0];
    if (opts.max_rounds > 0) lm.active[0] = 1;

    // ---- rule 5: the rounds.  cur / d_acc / acc are the accepted state, tri / d_trial / trial the trial of a round
    bool need_system = false, s_current = true;  // S on the host is the accepted state's
    std::vector<double> delta, cost_trial(1, 0.0);
    std::vector<int32_t> bad;
    while (lm.any_active()) {
        if (need_system) {
            rc = w.build_system(model, ctag::make_pose_cam(&cur), d_acc);
            if (rc != CTAG_OK) return rc;
            need_system = false;
        }
        rc = w.solve(lm.lambda, lm.active, delta, bad);
        if (rc != CTAG_OK) return rc;
        usable = !bad[0];
        if (usable) {
            double p[kN];
            params_of(cur, p);
            for (int i = 0; i < kN; i++)
                if ((w.mask >> i) & 1u) p[i] += delta[i];
            if (w.tie != 0.0) p[1] = p[0] * w.tie;
            tri = cur;
            set_params(tri, p);
            usable = camera_usable(tri);
        }
        if (usable) {
            FIT_HIP(hipMemcpyAsync(d_trial, d_acc, sizeof(ctag_rig_pose_rec) * n_items, hipMemcpyDeviceToDevice, w.c.s));
            rc = w.view_poses(model, ctag::make_pose_cam(&tri), d_trial, &usable);
            if (rc != CTAG_OK) return rc;
        }
        if (usable) {
            if (w.c.fetch(d_trial, n_items, trial) != CTAG_OK) return CTAG_ERR_HIP;
            w.costs_of(trial, nullptr, cost_trial, all_ok);
            usable = std::isfinite(cost_trial[0]);
        }
        if (!lm.decide(0, usable, cost_trial[0], opts)) continue;
        cur = tri;
        std::swap(d_acc, d_trial);
        acc.swap(trial);
        need_system = true;
        s_current = false;
    }

    // ---- rule 6: the result, its sigmas, and the pose back end's own cost under it
    if (need_system) {
        rc = w.build_system(model, ctag::make_pose_cam(&cur), d_acc);
        if (rc != CTAG_OK) return rc;
    }
    if (!s_current && w.fetch_S(S) != CTAG_OK) return CTAG_ERR_HIP;
    *out = cur;
    if (poses_out) std::memcpy(poses_out, acc.data(), sizeof(ctag_rig_pose_rec) * n_items);
    stat->rounds = lm.rounds[0];
    stat->cost = lm.cost[0];
    stat->lambda = lm.lambda[0];
    stat->rms_px = std::sqrt(2.0 * lm.cost[0] / (double)stat->n_points);
    stat->sigma2_hat = 2.0 * lm.cost[0] / (double)dof;
    // every record of an accepted state had its pose solved there; should one be flagged all the same it is missing from S, and the
    // sigmas stay 0 rather than describe a system that n_records and sigma2_hat do not
    flagged = false;
    for (int32_t f : w.flags) flagged = flagged || f != 0;
    if (!flagged && inverse_diagonal(S, w.mask, diag)) {
        for (int i = 0; i < kN; i++) stat->sigma[i] = std::sqrt(stat->sigma2_hat * diag[i]);
        if (w.tie != 0.0) stat->sigma[1] = w.tie * stat->sigma[0];
    }
    rc = w.c.pose_pass(0, [&]() { return ctag_rig_pose_batch_device(h, results_dev, n_frames, model, rigs, &cur, d_trial); }, d_trial, n_items, trial);
    if (rc != CTAG_OK) return rc;
    std::vector<double> pc;
    w.costs_of(trial, nullptr, pc, all_ok);
    stat->pose_cost = pc[0];
    return CTAG_OK;
}

int ctag_intrinsics_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* seed,
                        const ctag_intrinsics_fit_opts* opts, ctag_camera* out, ctag_intrinsics_fit_stat* stat, ctag_rig_pose_rec* poses_out) {
    if (!h || !results || n_frames < 1 || !model || !rigs || !seed || !out || !stat) return CTAG_ERR_ARG;
    if ((long long)n_frames > (1ll << 24)) return CTAG_ERR_LIMIT;
    return fit::with_results_on_device(h, results, n_frames, [&](const ctag_frame_result* results_dev) {
        return ctag_intrinsics_fit_device(h, results_dev, n_frames, model, rigs, seed, opts, out, stat, poses_out);
    });
}

}  // extern "C"
