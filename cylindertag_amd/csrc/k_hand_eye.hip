// k_hand_eye.hip -- hand-eye calibration: per rig the two fixed transforms P and Q of A_f ~ P o C_f o Q from the rig pose records of a
// batch, their covariances and one link pose per frame, on the device.  The semantics are stated in include/ctag_pose.h (hand-eye
// calibration, rules 1-10).
//
// Mapping.  An item is (frame f, rig g); the workspace is rig-major, item i = g * n_frames + f.  A problem is a rig;
// its frames are cut into chunks of 64 consecutive frame indices, lane = frame mod 64.
//   per item, one thread each     k_he_gather (either record kind -> Rm, tm, V with cov^-1 = V^T V, used; the thread of rig 0 also takes in the
//                                 frame's link pose, inverted or not as the mode says)
//   per problem, one wavefront    k_he_start (rule 5: three dependent reductions over the chunks in ascending order, svd3 and the 6x6
//                                 solve in every lane alike), k_he_solve (the chunk slots added in ascending order, each entry by its
//                                 owner lane; the damped 12x12 Cholesky and the step in registers, every lane alike; the trial state),
//                                 k_he_finish (the undamped matrix at the returned state, its scaled pivots, the inverse, the records)
//   per chunk, one wavefront      k_he_lin: a lane forms its frame's residual e, V e, the 6x12 J and V J; each of the 78 upper entries of
//                                 J^T W J = (V J)^T (V J), the 12 of the gradient and the cost term is reduced by wave_sum_f64 into the chunk's slot,
//                                 which only this wave writes.  LIN = false is the trial's cost alone.
//   per problem, one thread       k_he_decide: the chunk-ordered cost, then the Levenberg-Marquardt decision of ctag_lm.h
// Everything is FP64 VALU.  No sum over frames is taken any other way (rule 9); there are no floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_linalg.h"
#include "ctag_lm.h"
#include "ctag_loss.h"
#include "ctag_so3.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_link_pose) == 48, "ctag_link_pose layout");
static_assert(sizeof(ctag_hand_eye_opts) == 32, "ctag_hand_eye_opts layout");
static_assert(sizeof(ctag_hand_eye_rec) == 1312, "ctag_hand_eye_rec layout");
static_assert(sizeof(ctag_hand_eye_frame_rec) == 80, "ctag_hand_eye_frame_rec layout");

namespace ctag {

constexpr double kHeRelTol = 1e-12, kHeLambdaMax = 1e6, kHeMinPivot = 1e-12, kHeMaxAngle2 = 9.0;
// a chunk's slot: the 78 upper entries of J^T W J (entry (i, j), i <= j, at j (j + 1) / 2 + i), the 12 of the gradient, the cost of the
// accepted state, the cost of the trial state, the number of downweighted frames
constexpr int kHeSlot = 93, kHeSlotCost = 90, kHeSlotTrial = 91, kHeSlotDown = 92;
constexpr int kHeItemDoubles = 9 + 3 + 36 + 8, kHeFrameDoubles = 12, kHeRigDoubles = 24 + 24 + 3, kHeRigInts = 6;

struct HeWs {
    double *Rm, *tm, *V, *fr;                 // per item: 9, 3, 36 (W = V^T V, V lower triangular); 8: e, mahalanobis2 and weight at the returned state
    double *RC, *tC;                          // per frame: 9, 3
    double* slot;                             // per chunk of a rig: kHeSlot
    double *X, *XT, *lambda, *cost, *cost0;   // per rig: 24 (R_P, t_P, R_Q, t_Q) accepted and trial
    int32_t* used;                            // per item
    int32_t *bad, *status, *active, *rounds, *sing, *n_used;  // per rig
    int n_frames, n_rigs, n_chunks;
};

struct HeP {
    int loss, max_iterations;
    double a, a2, lambda0;
};

__device__ __forceinline__ void mat3_mul_tn(const double* A, const double* B, double* C) {  // C = A^T B
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void mat3_vec(const double* A, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
__device__ __forceinline__ double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// the rotation nearest M in the Frobenius norm: U diag(1, 1, det(U) det(V)) V^T
__device__ __forceinline__ void nearest_rotation(const double* M, double* R) {
    double U[9], sv[3], V[9];
    ctl::svd3(M, U, sv, V);
    const double sg = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) R[a * 3 + b] = U[a * 3] * V[b * 3] + U[a * 3 + 1] * V[b * 3 + 1] + sg * U[a * 3 + 2] * V[b * 3 + 2];
}

// ---- gather: either record kind to the sample arrays, the links to C_f -------------------------------------------------------------------
template <class Rec>
__global__ __launch_bounds__(256) void k_he_gather(const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov,
                                                   const ctag_link_pose* __restrict__ links, int invert, HeWs ws) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= ws.n_frames * ws.n_rigs) return;
    const int f = w / ws.n_rigs, g = w - f * ws.n_rigs;
    const size_t i = (size_t)g * ws.n_frames + f;
    const ctag_link_pose Lk = links[f];
    bool link_ok = true;
    for (int k = 0; k < 3; k++) link_ok = link_ok && ctl::finite64(Lk.rvec[k]) && ctl::finite64(Lk.tvec[k]);
    if (g == 0) {
        double R[9], C[12];
        for (int k = 0; k < 12; k++) C[k] = 0.0;
        if (link_ok) {
            ctl::angle_axis_rot(Lk.rvec, R, nullptr);
            if (invert) {  // C_f = link_f^-1: (R^T, -R^T t)
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b < 3; b++) C[a * 3 + b] = R[b * 3 + a];
                for (int a = 0; a < 3; a++) C[9 + a] = -(R[a] * Lk.tvec[0] + R[3 + a] * Lk.tvec[1] + R[6 + a] * Lk.tvec[2]);
            } else {
                for (int k = 0; k < 9; k++) C[k] = R[k];
                for (int k = 0; k < 3; k++) C[9 + k] = Lk.tvec[k];
            }
        }
        for (int k = 0; k < 9; k++) ws.RC[(size_t)f * 9 + k] = C[k];
        for (int k = 0; k < 3; k++) ws.tC[(size_t)f * 3 + k] = C[9 + k];
    }
    const Rec& P = recs[w];
    const ctag_pose_cov_rec& Q = cov[w];
    if (misplaced_or_rvec(P, Q, f, g)) atomicOr(&ws.bad[g], 1);
    const bool measured = measured_sample<true>(P, Q, kHeMinPivot, ws.Rm + i * 9, ws.tm + i * 3, ws.V + i * 36);  // V, with cov^-1 = V^T V
    ws.used[i] = measured && link_ok ? 1 : 0;
}

// ---- rule 5: one wavefront per problem ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_he_start(HeWs ws) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)g * ws.n_frames;
    int n_used = 0, k0 = -1;
    for (int c = 0; c < ws.n_chunks; c++) {
        const int f = c * 64 + lane;
        const unsigned long long m = __ballot(f < ws.n_frames && ws.used[base + f] != 0);
        n_used += __popcll(m);
        if (k0 < 0 && m) k0 = c * 64 + __ffsll((long long)m) - 1;
    }
    int status = CTAG_HE_OK;
    if (ws.bad[g]) {
        status = CTAG_HE_BAD_INPUT;
        n_used = 0;
    } else if (n_used < 3) {
        status = CTAG_HE_TOO_FEW;
    }
    double X[24];
    for (int k = 0; k < 24; k++) X[k] = 0.0;
    if (status == CTAG_HE_OK) {
        double Rm0[9], RC0[9], acc[15];
        for (int k = 0; k < 9; k++) {
            Rm0[k] = ws.Rm[(base + k0) * 9 + k];
            RC0[k] = ws.RC[(size_t)k0 * 9 + k];
        }
        // S = sum alpha beta^T
        for (int k = 0; k < 9; k++) acc[k] = 0.0;
        for (int c = 0; c < ws.n_chunks; c++) {
            const int f = c * 64 + lane;
            double ab[9];
            for (int k = 0; k < 9; k++) ab[k] = 0.0;
            if (f < ws.n_frames && ws.used[base + f]) {
                double D[9], al[3], be[3];
                mat3_mul_nt(ws.Rm + (base + f) * 9, Rm0, D);
                so3_log(D, al);
                mat3_mul_nt(ws.RC + (size_t)f * 9, RC0, D);
                so3_log(D, be);
                if (al[0] * al[0] + al[1] * al[1] + al[2] * al[2] <= kHeMaxAngle2 && be[0] * be[0] + be[1] * be[1] + be[2] * be[2] <= kHeMaxAngle2)
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) ab[a * 3 + b] = al[a] * be[b];
            }
            for (int k = 0; k < 9; k++) acc[k] += wave_sum_f64(ab[k]);
        }
        double* RP = X;
        nearest_rotation(acc, RP);
        // R_Q nearest sum R_C^T R_P^T Rm
        for (int k = 0; k < 9; k++) acc[k] = 0.0;
        for (int c = 0; c < ws.n_chunks; c++) {
            const int f = c * 64 + lane;
            double M[9];
            for (int k = 0; k < 9; k++) M[k] = 0.0;
            if (f < ws.n_frames && ws.used[base + f]) {
                double T[9];
                mat3_mul_tn(RP, ws.Rm + (base + f) * 9, T);
                mat3_mul_tn(ws.RC + (size_t)f * 9, T, M);
            }
            for (int k = 0; k < 9; k++) acc[k] += wave_sum_f64(M[k]);
        }
        nearest_rotation(acc, X + 12);
        // [B | I] [t_Q; t_P] = r, B = R_P R_C, r = tm - R_P t_C: B^T B = I, so the normal matrix is [[n I, sum B^T], [sum B, n I]]
        for (int k = 0; k < 15; k++) acc[k] = 0.0;
        for (int c = 0; c < ws.n_chunks; c++) {
            const int f = c * 64 + lane;
            double v[15];
            for (int k = 0; k < 15; k++) v[k] = 0.0;
            if (f < ws.n_frames && ws.used[base + f]) {
                double r[3], pc[3];
                mat3_mul(RP, ws.RC + (size_t)f * 9, v);
                mat3_vec(RP, ws.tC + (size_t)f * 3, pc);
                for (int k = 0; k < 3; k++) r[k] = ws.tm[(base + f) * 3 + k] - pc[k];
                for (int k = 0; k < 3; k++) v[9 + k] = v[k] * r[0] + v[3 + k] * r[1] + v[6 + k] * r[2];
                for (int k = 0; k < 3; k++) v[12 + k] = r[k];
            }
            for (int k = 0; k < 15; k++) acc[k] += wave_sum_f64(v[k]);
        }
        double H[36], x[6];
        for (int k = 0; k < 36; k++) H[k] = 0.0;
        for (int a = 0; a < 3; a++) {
            H[a * 6 + a] = (double)n_used;
            H[(3 + a) * 6 + 3 + a] = (double)n_used;
            for (int b = 0; b < 3; b++) {
                H[(3 + a) * 6 + b] = acc[a * 3 + b];
                H[b * 6 + 3 + a] = acc[a * 3 + b];
            }
        }
        if (ctl::chol6_solve(H, acc + 9, x)) {
            for (int k = 0; k < 3; k++) {
                X[21 + k] = x[k];
                X[9 + k] = x[3 + k];
            }
        } else {
            status = CTAG_HE_SINGULAR;
            for (int k = 0; k < 24; k++) X[k] = 0.0;
        }
    }
    if (lane == 0) {
        for (int k = 0; k < 24; k++) ws.X[(size_t)g * 24 + k] = X[k];
        ws.status[g] = status;
        ws.n_used[g] = n_used;
        ws.active[g] = 0;
        ws.rounds[g] = 0;
        ws.sing[g] = 0;
        ws.lambda[g] = 0.0;
        ws.cost[g] = 0.0;
        ws.cost0[g] = 0.0;
    }
}

// ---- rules 3 and 4 at one frame: one wavefront per chunk ------------------------------------------------------------------------------------
// trial: the state is XT, not X.  all_problems: every problem that has a state, stopped or not (the start's cost and the pass behind the
// rounds), and the frames' residuals are kept for the records; otherwise the problems still running.
template <bool LIN>
__global__ __launch_bounds__(64) void k_he_lin(HeWs ws, HeP P, int trial, int all_problems) {
    const int g = blockIdx.x / ws.n_chunks, c = blockIdx.x - g * ws.n_chunks, lane = threadIdx.x;
    if (ws.status[g] != CTAG_HE_OK) return;
    if (!all_problems && !ws.active[g]) return;
    const int f = c * 64 + lane;
    const size_t i = (size_t)g * ws.n_frames + f;
    const bool used = f < ws.n_frames && ws.used[i] != 0;
    double e[6], ve[6], Vm[36], J[72];  // the residual and V e; V; J
    double wgt = 0.0, rho = 0.0, s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) e[k] = ve[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 36; k++) Vm[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 72; k++) J[k] = 0.0;
    if (used) {
        const double* X = (trial ? ws.XT : ws.X) + (size_t)g * 24;
        double RP[9], RQ[9], tP[3], tQ[3], B[9], Rp[9], D[9], u[3], pc[3];
        for (int k = 0; k < 9; k++) {
            RP[k] = X[k];
            RQ[k] = X[12 + k];
        }
        for (int k = 0; k < 3; k++) {
            tP[k] = X[9 + k];
            tQ[k] = X[21 + k];
        }
        mat3_mul(RP, ws.RC + (size_t)f * 9, B);
        mat3_mul(B, RQ, Rp);
        mat3_vec(ws.RC + (size_t)f * 9, tQ, pc);  // u = R_P (R_C t_Q + t_C): the inner vector is rounded once, then rotated once
        for (int k = 0; k < 3; k++) pc[k] += ws.tC[(size_t)f * 3 + k];
        mat3_vec(RP, pc, u);
        mat3_mul_nt(Rp, ws.Rm + i * 9, D);
        so3_log(D, e);
        for (int k = 0; k < 3; k++) e[3 + k] = u[k] + tP[k] - ws.tm[i * 3 + k];
#pragma unroll
        for (int k = 0; k < 36; k++) Vm[k] = ws.V[i * 36 + k];
        // the whitened residual: e^T W e = |V e|^2, a sum of squares -- e^T W e itself cancels by the condition of W, and next to the
        // minimum a round is accepted or not by a difference of two such sums
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b <= a; b++) t += Vm[a * 6 + b] * e[b];
            ve[a] = t;
            s += t * t;
        }
        if (P.loss == CTAG_TRACK_LOSS_NONE) {
            rho = s;
            wgt = 1.0;
        } else {
            robust_loss(P.loss, P.a, P.a2, s, rho, wgt);
        }
        if (LIN) {
            double Ji[9], JiB[9];
            so3_jlinv(e, Ji);
            mat3_mul(Ji, B, JiB);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    J[r * 12 + q] = Ji[r * 3 + q];
                    J[r * 12 + 6 + q] = JiB[r * 3 + q];
                    J[(3 + r) * 12 + 9 + q] = B[r * 3 + q];
                }
            // -[u]x
            J[3 * 12 + 1] = u[2];
            J[3 * 12 + 2] = -u[1];
            J[4 * 12 + 0] = -u[2];
            J[4 * 12 + 2] = u[0];
            J[5 * 12 + 0] = u[1];
            J[5 * 12 + 1] = -u[0];
            J[3 * 12 + 3] = J[4 * 12 + 4] = J[5 * 12 + 5] = 1.0;
        }
    }
    double* slot = ws.slot + ((size_t)g * ws.n_chunks + c) * kHeSlot;
    const double cterm = wave_sum_f64(0.5 * rho);
    if (!LIN) {
        if (lane == 0) slot[kHeSlotTrial] = cterm;
        return;
    }
    const unsigned long long down = __ballot(used && P.loss != CTAG_TRACK_LOSS_NONE && s > P.a2);
    if (lane == 0) {
        slot[kHeSlotCost] = cterm;
        slot[kHeSlotDown] = (double)__popcll(down);
    }
    if (all_problems && f < ws.n_frames) {
        double* fr = ws.fr + i * 8;
        for (int k = 0; k < 6; k++) fr[k] = e[k];
        fr[6] = s;
        fr[7] = wgt;
    }
    // J <- V J, column by column; then J^T W J = (V J)^T (V J) and the gradient (V J)^T (V e), each times the loss's weight
#pragma unroll
    for (int j = 0; j < 12; j++) {
        double vj[6];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q <= r; q++) t += Vm[r * 6 + q] * J[q * 12 + j];
            vj[r] = t;
        }
#pragma unroll
        for (int r = 0; r < 6; r++) J[r * 12 + j] = vj[r];
#pragma unroll
        for (int a = 0; a <= j; a++) {
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < 6; r++) t += J[r * 12 + a] * vj[r];
            t = wave_sum_f64(wgt * t);
            if (lane == 0) slot[j * (j + 1) / 2 + a] = t;
        }
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) t += vj[r] * ve[r];
        t = wave_sum_f64(wgt * t);
        if (lane == 0) slot[78 + j] = t;
    }
}

// ---- 12x12 in registers, every lane alike --------------------------------------------------------------------------------------------------
// A = L L^T in place (the lower triangle is read and written); min_pivot the smallest pivot met; false at the first pivot not above
// min_allowed (or not a number)
__device__ __forceinline__ bool chol12(double* A, double min_allowed, double& min_pivot) {
    min_pivot = A[0];
#pragma unroll
    for (int j = 0; j < 12; j++) {
        double d = A[j * 12 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= A[j * 12 + k] * A[j * 12 + k];
        if (!(d >= min_pivot)) min_pivot = d;
        if (!(d > min_allowed)) return false;
        d = ctm::sqrt64(d);
        A[j * 12 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 12; i++) {
            double t = A[i * 12 + j];
#pragma unroll
            for (int k = 0; k < j; k++) t -= A[i * 12 + k] * A[j * 12 + k];
            A[i * 12 + j] = t / d;
        }
    }
    return true;
}

// the chunk slots of problem g added in ascending order, entry k by lane k % 64, into sh[0 .. 92]
__device__ __forceinline__ void he_sum_slots(const HeWs& ws, int g, int lane, double* sh) {
    for (int k = lane; k < kHeSlot; k += 64) {
        double acc = 0.0;
        for (int c = 0; c < ws.n_chunks; c++) acc += ws.slot[((size_t)g * ws.n_chunks + c) * kHeSlot + k];
        sh[k] = acc;
    }
    __syncthreads();
}

// ---- a round's step: one wavefront per problem ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_he_solve(HeWs ws) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (ws.status[g] != CTAG_HE_OK || !ws.active[g]) return;
    __shared__ double sh[kHeSlot];
    he_sum_slots(ws, g, lane, sh);
    double A[144], y[12], d[12];
#pragma unroll
    for (int j = 0; j < 12; j++)
#pragma unroll
        for (int a = 0; a <= j; a++) A[j * 12 + a] = sh[j * (j + 1) / 2 + a];
    const double lam = ws.lambda[g];
#pragma unroll
    for (int j = 0; j < 12; j++) A[j * 12 + j] += lam * A[j * 12 + j];
    double mp;
    if (!chol12(A, 0.0, mp)) {
        if (lane == 0) ws.sing[g] = 1;
        return;
    }
#pragma unroll
    for (int a = 0; a < 12; a++) {
        double t = -sh[78 + a];
#pragma unroll
        for (int k = 0; k < a; k++) t -= A[a * 12 + k] * y[k];
        y[a] = t / A[a * 12 + a];
    }
#pragma unroll
    for (int a = 11; a >= 0; a--) {
        double t = y[a];
#pragma unroll
        for (int k = a + 1; k < 12; k++) t -= A[k * 12 + a] * d[k];
        d[a] = t / A[a * 12 + a];
    }
    if (lane == 0) {
        const double* X = ws.X + (size_t)g * 24;
        double* T = ws.XT + (size_t)g * 24;
        double E[9], R[9];
        ctl::angle_axis_rot(d, E, nullptr);
        mat3_mul(E, X, R);
        for (int k = 0; k < 9; k++) T[k] = R[k];
        for (int k = 0; k < 3; k++) T[9 + k] = X[9 + k] + d[3 + k];
        ctl::angle_axis_rot(d + 6, E, nullptr);
        mat3_mul(E, X + 12, R);
        for (int k = 0; k < 9; k++) T[12 + k] = R[k];
        for (int k = 0; k < 3; k++) T[21 + k] = X[21 + k] + d[9 + k];
    }
}

// ---- a problem's cost and decision: mode 0 takes the start's cost, mode 1 decides the round ----------------------------------------------------
__global__ __launch_bounds__(64) void k_he_decide(HeWs ws, HeP P, int mode) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ws.n_rigs || ws.status[g] != CTAG_HE_OK) return;
    if (mode == 1 && !ws.active[g]) return;
    double c = 0.0;
    for (int k = 0; k < ws.n_chunks; k++) c += ws.slot[((size_t)g * ws.n_chunks + k) * kHeSlot + (mode == 0 ? kHeSlotCost : kHeSlotTrial)];
    if (mode == 0) {
        ws.cost0[g] = c;
        ws.cost[g] = c;
        ws.lambda[g] = P.lambda0;
        ws.active[g] = ctl::finite64(c) ? 1 : 0;
        return;
    }
    LmState st{ws.lambda[g], ws.cost[g], 1, ws.rounds[g]};
    const bool usable = ws.sing[g] == 0 && ctl::finite64(c);
    if (lm_decide(st, usable, c, kHeRelTol, kHeLambdaMax, P.max_iterations))
        for (int k = 0; k < 24; k++) ws.X[(size_t)g * 24 + k] = ws.XT[(size_t)g * 24 + k];
    ws.lambda[g] = st.lambda;
    ws.cost[g] = st.cost;
    ws.active[g] = st.active;
    ws.rounds[g] = st.rounds;
    ws.sing[g] = 0;
}

// ---- rule 8: one wavefront per problem ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_he_finish(HeWs ws, HeP P, ctag_hand_eye_rec* __restrict__ out, ctag_hand_eye_frame_rec* __restrict__ frames) {
    const int g = blockIdx.x, lane = threadIdx.x;
    __shared__ double sh[kHeSlot];
    __shared__ double Wi[144];  // L^-1 of the scaled matrix, column j by lane j
    __shared__ double dsh[12];  // the scaling, diag^-1/2
    int status = ws.status[g];
    const bool has_state = status == CTAG_HE_OK;
    double dg[12], min_pivot = 0.0;
    bool solved = false;
    if (has_state) {
        he_sum_slots(ws, g, lane, sh);
        double A[144];
        bool good = ctl::finite64(ws.cost[g]);
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const double h = sh[j * (j + 1) / 2 + j];
            good = good && ctl::finite64(h) && h > 0.0;
            dg[j] = 1.0 / ctm::sqrt64(h);
        }
#pragma unroll
        for (int j = 0; j < 12; j++)
#pragma unroll
            for (int a = 0; a <= j; a++) A[j * 12 + a] = dg[j] * sh[j * (j + 1) / 2 + a] * dg[a];
        solved = good && chol12(A, kHeMinPivot, min_pivot);
        if (!good) min_pivot = 0.0;
        if (solved) {
            // column `lane` of L^-1
            double y[12];
#pragma unroll
            for (int a = 0; a < 12; a++) {
                double t = a == lane ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < a; k++) t -= A[a * 12 + k] * y[k];
                y[a] = t / A[a * 12 + a];
            }
            if (lane < 12) {
                dsh[lane] = 1.0 / ctm::sqrt64(sh[lane * (lane + 1) / 2 + lane]);
#pragma unroll
                for (int a = 0; a < 12; a++) Wi[a * 12 + lane] = a < lane ? 0.0 : y[a];
            }
        } else {
            status = CTAG_HE_SINGULAR;
        }
    }
    __syncthreads();
    ctag_hand_eye_rec* R = out + g;
    if (solved) {  // inv = D L^-T L^-1 D, entry (a, b), a <= b, by its owner lane, mirrored
        for (int en = lane; en < 78; en += 64) {
            int b = 0;
            while ((b + 1) * (b + 2) / 2 <= en) b++;
            const int a = en - b * (b + 1) / 2;
            double t = 0.0;
            for (int k = b; k < 12; k++) t += Wi[k * 12 + a] * Wi[k * 12 + b];
            t = dsh[a] * t * dsh[b];
            R->cov[a * 12 + b] = t;
            R->cov[b * 12 + a] = t;
        }
    } else {
        for (int k = lane; k < 144; k += 64) R->cov[k] = 0.0;
    }
    if (lane == 0) {
        const int n_used = ws.n_used[g];
        R->status = status;
        R->rig = g;
        R->n_used = n_used;
        R->n_downweighted = has_state ? (int)sh[kHeSlotDown] : 0;
        R->rounds = ws.rounds[g];
        const int dof = 6 * n_used - 12;
        const bool counted = status == CTAG_HE_OK || status == CTAG_HE_SINGULAR;
        R->dof = counted ? dof : 0;
        const double* X = ws.X + (size_t)g * 24;
        for (int k = 0; k < 3; k++) R->P.rvec[k] = R->P.tvec[k] = R->Q.rvec[k] = R->Q.tvec[k] = 0.0;
        if (has_state) {
            so3_log(X, R->P.rvec);
            so3_log(X + 12, R->Q.rvec);
            for (int k = 0; k < 3; k++) {
                R->P.tvec[k] = X[9 + k];
                R->Q.tvec[k] = X[21 + k];
            }
        }
        const double cost = has_state ? ws.cost[g] : 0.0;
        R->cost0 = has_state ? ws.cost0[g] : 0.0;
        R->cost = cost;
        R->lambda = has_state ? ws.lambda[g] : 0.0;
        R->sigma2_hat = has_state && dof > 0 ? 2.0 * cost / (double)dof : 0.0;
        R->min_pivot = has_state ? min_pivot : 0.0;
    }
    if (!frames) return;
    for (int f = lane; f < ws.n_frames; f += 64) {
        const size_t i = (size_t)g * ws.n_frames + f;
        ctag_hand_eye_frame_rec r;
        unsigned long long* words = reinterpret_cast<unsigned long long*>(&r);
        for (int k = 0; k < (int)(sizeof(r) / 8); k++) words[k] = 0ull;
        r.rig = g;
        r.frame = f;
        if (has_state && ws.used[i]) {
            const double* fr = ws.fr + i * 8;
            r.status = status;
            for (int k = 0; k < 6; k++) r.e[k] = fr[k];
            r.mahalanobis2 = fr[6];
            r.weight = fr[7];
            r.flags = CTAG_HE_FLAG_USED | (P.loss != CTAG_TRACK_LOSS_NONE && fr[6] > P.a2 ? CTAG_HE_FLAG_DOWNWEIGHTED : 0u);
        }
        frames[(size_t)f * ws.n_rigs + g] = r;
    }
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
namespace {

struct HandEyeState {
    ctag::DevBuf<double> d_ws;
    ctag::DevBuf<int32_t> d_int;
    ctag::DevBuf<ctag_link_pose> d_links;
    ctag::DevBuf<unsigned char> d_in;          // the host forms' records
    ctag::DevBuf<ctag_pose_cov_rec> d_cov;
    ctag::DevBuf<ctag_hand_eye_rec> d_out;
    ctag::DevBuf<ctag_hand_eye_frame_rec> d_frames;
    std::vector<ctag_link_pose> links;         // the links of the call in flight: the caller's array may go once the call returns
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t done = nullptr;                 // behind the last hand-eye call's kernels: the workspace and `links` are free again
    bool in_flight = false;
    bool timed = false;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
};

void he_state_free(void* p) {
    HandEyeState* s = static_cast<HandEyeState*>(p);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->done) (void)hipEventDestroy(s->done);
    delete s;
}

HandEyeState* he_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kHandEyeState, he_state_free);
    if (!*slot) {
        HandEyeState* s = new (std::nothrow) HandEyeState();
        if (!s) return nullptr;
        for (auto& e : s->ev)
            if (hipEventCreate(&e) != hipSuccess) {
                he_state_free(s);
                return nullptr;
            }
        if (hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess) {
            he_state_free(s);
            return nullptr;
        }
        *slot = s;
    }
    return static_cast<HandEyeState*>(*slot);
}

int he_opts(const ctag_hand_eye_opts* o, ctag::HeP& p, int& mode) {
    ctag_hand_eye_opts d;
    ctag_hand_eye_opts_default(&d);
    if (!o) o = &d;
    if (o->struct_size != sizeof(ctag_hand_eye_opts)) return CTAG_ERR_ARG;
    if (o->mode != CTAG_HAND_EYE_CAMERA_ON_LINK && o->mode != CTAG_HAND_EYE_RIG_ON_LINK) return CTAG_ERR_ARG;
    if (o->loss != CTAG_LOSS_HUBER && o->loss != CTAG_LOSS_CAUCHY && o->loss != CTAG_TRACK_LOSS_NONE) return CTAG_ERR_ARG;
    if (o->max_iterations < 1) return CTAG_ERR_ARG;
    if (!std::isfinite(o->loss_scale) || !(o->loss_scale > 0.0)) return CTAG_ERR_ARG;
    if (!std::isfinite(o->lambda0) || o->lambda0 < 0.0) return CTAG_ERR_ARG;
    p.loss = o->loss;
    p.max_iterations = o->max_iterations;
    p.a = o->loss_scale;
    p.a2 = o->loss_scale * o->loss_scale;
    p.lambda0 = o->lambda0;
    mode = o->mode;
    return CTAG_OK;
}

size_t he_ws_doubles(size_t n_items, size_t n_frames, size_t n_rigs, size_t n_chunks) {
    return n_items * ctag::kHeItemDoubles + n_frames * ctag::kHeFrameDoubles + n_rigs * n_chunks * ctag::kHeSlot + n_rigs * ctag::kHeRigDoubles;
}

void he_carve(HandEyeState* st, int n_frames, int n_rigs, int n_chunks, ctag::HeWs& ws) {
    const size_t n = (size_t)n_frames * n_rigs, nf = (size_t)n_frames, nr = (size_t)n_rigs;
    double* d = st->d_ws.p;
    auto take = [&](size_t count) {
        double* r = d;
        d += count;
        return r;
    };
    ws.Rm = take(9 * n), ws.tm = take(3 * n), ws.V = take(36 * n), ws.fr = take(8 * n);
    ws.RC = take(9 * nf), ws.tC = take(3 * nf);
    ws.slot = take(nr * n_chunks * ctag::kHeSlot);
    ws.X = take(24 * nr), ws.XT = take(24 * nr), ws.lambda = take(nr), ws.cost = take(nr), ws.cost0 = take(nr);
    int32_t* q = st->d_int.p;
    auto itake = [&](size_t count) {
        int32_t* r = q;
        q += count;
        return r;
    };
    ws.used = itake(n);
    ws.bad = itake(nr), ws.status = itake(nr), ws.active = itake(nr), ws.rounds = itake(nr), ws.sing = itake(nr), ws.n_used = itake(nr);
    ws.n_frames = n_frames;
    ws.n_rigs = n_rigs;
    ws.n_chunks = n_chunks;
}

template <class Rec>
int he_device(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs_dev, const ctag_pose_cov_rec* cov_dev, int n_frames, const ctag_link_pose* links,
              const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out_dev, ctag_hand_eye_frame_rec* frames_dev) {
    if (!h || !rigs || !recs_dev || !cov_dev || n_frames < 1 || !links || !out_dev) return CTAG_ERR_ARG;
    ctag::HeP P;
    int mode = 0;
    if (he_opts(opts, P, mode) != CTAG_OK) return CTAG_ERR_ARG;
    const int n_rigs = rigs->n_rigs;
    const long long n_items = (long long)n_frames * n_rigs;
    if (n_rigs < 1 || n_items > CTAG_HAND_EYE_MAX_ITEMS) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    HandEyeState* st = he_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    // an earlier hand-eye call's kernels may still read the workspace and the links: that call is waited for, nothing else on the stream is
    if (st->in_flight && hipEventSynchronize(st->done) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = false;
    const size_t n = (size_t)n_items;
    const int n_chunks = (n_frames + 63) / 64;
    if (st->d_ws.grow(he_ws_doubles(n, (size_t)n_frames, (size_t)n_rigs, (size_t)n_chunks)) != hipSuccess ||
        st->d_int.grow(n + (size_t)ctag::kHeRigInts * n_rigs) != hipSuccess || st->d_links.grow((size_t)n_frames) != hipSuccess)
        return CTAG_ERR_HIP;
    st->links.assign(links, links + n_frames);
    if (hipMemcpyAsync(st->d_links.p, st->links.data(), sizeof(ctag_link_pose) * (size_t)n_frames, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    ctag::HeWs ws;
    he_carve(st, n_frames, n_rigs, n_chunks, ws);
    if (hipMemsetAsync(ws.bad, 0, sizeof(int32_t) * (size_t)n_rigs, s) != hipSuccess) return CTAG_ERR_HIP;
    const bool timing = ctag::handle_timing(h);
    st->timed = timing;
    auto mark = [&](int k) { return !timing || hipEventRecord(st->ev[k], s) == hipSuccess; };
    const dim3 per_item((unsigned)((n + 255) / 256)), per_chunk((unsigned)n_rigs * (unsigned)n_chunks), per_rig((unsigned)n_rigs);
    const dim3 rig_threads((unsigned)((n_rigs + 63) / 64));
    if (!mark(0)) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_he_gather<Rec>, per_item, dim3(256), 0, s, recs_dev, cov_dev, st->d_links.p,
                       mode == CTAG_HAND_EYE_CAMERA_ON_LINK ? 1 : 0, ws);
    hipLaunchKernelGGL(ctag::k_he_start, per_rig, dim3(64), 0, s, ws);
    hipLaunchKernelGGL(ctag::k_he_lin<true>, per_chunk, dim3(64), 0, s, ws, P, 0, 1);  // every problem that has a start, so that cost0 is there
    hipLaunchKernelGGL(ctag::k_he_decide, rig_threads, dim3(64), 0, s, ws, P, 0);
    if (!mark(1)) return CTAG_ERR_HIP;
    for (int round = 0; round < P.max_iterations; round++) {
        if (round > 0) hipLaunchKernelGGL(ctag::k_he_lin<true>, per_chunk, dim3(64), 0, s, ws, P, 0, 0);
        hipLaunchKernelGGL(ctag::k_he_solve, per_rig, dim3(64), 0, s, ws);
        hipLaunchKernelGGL(ctag::k_he_lin<false>, per_chunk, dim3(64), 0, s, ws, P, 1, 0);
        hipLaunchKernelGGL(ctag::k_he_decide, rig_threads, dim3(64), 0, s, ws, P, 1);
    }
    if (!mark(2)) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_he_lin<true>, per_chunk, dim3(64), 0, s, ws, P, 0, 1);
    hipLaunchKernelGGL(ctag::k_he_finish, per_rig, dim3(64), 0, s, ws, P, out_dev, frames_dev);
    if (hipGetLastError() != hipSuccess || !mark(3)) return CTAG_ERR_HIP;
    if (hipEventRecord(st->done, s) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = true;
    return CTAG_OK;
}

template <class Rec>
int he_host(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, const ctag_link_pose* links,
            const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out, ctag_hand_eye_frame_rec* frames) {
    if (!h || !rigs || !recs || !cov || n_frames < 1 || !links || !out) return CTAG_ERR_ARG;
    const long long n_items = (long long)n_frames * rigs->n_rigs;
    if (rigs->n_rigs < 1 || n_items > CTAG_HAND_EYE_MAX_ITEMS) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    HandEyeState* st = he_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    // the buffers below are read and written by the kernels of an earlier device-form call only through the caller's own pointers, and
    // every earlier host form has waited for its own work: they are free
    const size_t n = (size_t)n_items, nr = (size_t)rigs->n_rigs;
    if (st->d_in.grow(sizeof(Rec) * n) != hipSuccess || st->d_cov.grow(n) != hipSuccess || st->d_out.grow(nr) != hipSuccess ||
        (frames && st->d_frames.grow(n) != hipSuccess))
        return CTAG_ERR_HIP;
    if (hipMemcpyAsync(st->d_in.p, recs, sizeof(Rec) * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(st->d_cov.p, cov, sizeof(ctag_pose_cov_rec) * n, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    const int rc = he_device<Rec>(h, rigs, reinterpret_cast<const Rec*>(st->d_in.p), st->d_cov.p, n_frames, links, opts, st->d_out.p,
                                  frames ? st->d_frames.p : nullptr);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_hand_eye_rec) * nr, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (frames && hipMemcpyAsync(frames, st->d_frames.p, sizeof(ctag_hand_eye_frame_rec) * n, hipMemcpyDeviceToHost, s) != hipSuccess))
        return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_hand_eye_opts_default(ctag_hand_eye_opts* o) {
    if (!o) return;
    o->struct_size = (uint32_t)sizeof(ctag_hand_eye_opts);
    o->mode = CTAG_HAND_EYE_CAMERA_ON_LINK;
    o->loss = CTAG_TRACK_LOSS_NONE;
    o->max_iterations = 20;
    o->loss_scale = 4.0;
    o->lambda0 = 1e-3;
}

int ctag_rig_hand_eye_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                 int n_frames, const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out_dev,
                                 ctag_hand_eye_frame_rec* frames_dev) {
    return he_device<ctag_rig_pose_rec>(h, rigs, rig_poses_dev, cov_dev, n_frames, links, opts, out_dev, frames_dev);
}

int ctag_mv_rig_hand_eye_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                    int n_frames, const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out_dev,
                                    ctag_hand_eye_frame_rec* frames_dev) {
    return he_device<ctag_mv_pose_rec>(h, rigs, mv_poses_dev, cov_dev, n_frames, links, opts, out_dev, frames_dev);
}

int ctag_rig_hand_eye_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                          const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out, ctag_hand_eye_frame_rec* frames) {
    return he_host<ctag_rig_pose_rec>(h, rigs, rig_poses, cov, n_frames, links, opts, out, frames);
}

int ctag_mv_rig_hand_eye_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                             const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out, ctag_hand_eye_frame_rec* frames) {
    return he_host<ctag_mv_pose_rec>(h, rigs, mv_poses, cov, n_frames, links, opts, out, frames);
}

int ctag_hand_eye_last_ms(ctag_handle* h, float* out4) {
    if (!h || !out4) return CTAG_ERR_ARG;
    HandEyeState* st = he_state(h);
    if (!st) return CTAG_ERR_HIP;
    if (st->timed) {
        st->timed = false;
        for (float& v : st->ms) v = 0.f;
        if (hipEventSynchronize(st->ev[3]) == hipSuccess) {
            for (int k = 0; k < 3; k++) (void)hipEventElapsedTime(&st->ms[k], st->ev[k], st->ev[k + 1]);
            (void)hipEventElapsedTime(&st->ms[3], st->ev[0], st->ev[3]);
        }
    }
    for (int k = 0; k < 4; k++) out4[k] = st->ms[k];
    return CTAG_OK;
}

}  // extern "C"
