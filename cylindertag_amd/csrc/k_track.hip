// k_track.hip -- one smoothed trajectory per rig over the frames of a batch: the rig pose records and their covariances under a
// constant-velocity model (white noise on acceleration), on the device.  The semantics are stated in include/ctag_pose.h (track
// smoothing, rules 1-10).
//
// Mapping.  An item is (frame f, rig g); the workspace is rig-major, item i = g * n_frames + f, so that a rig's
// time axis is contiguous.  A piece's state (lambda, cost, active, rounds, singular) lives in the slot of its first frame.
//   per item, one thread each   k_track_gather (either record kind -> R, t, W = cov^-1), k_track_start_pose / _vel (rule 5),
//                               k_track_lin (a frame's 12x12 diagonal block D, its coupling C to the next frame, -gradient and cost
//                               term), k_track_trial, k_track_write
//   per rig, one wavefront      k_track_pieces: the piece and separator tables by ballots over 64 frames at a time, forwards and backwards
//   per segment, one wavefront  k_track_seg_factor: the block Cholesky chain over the frames between two separators with the coupling to
//                               the left separator carried along -> the segment's Schur complement on its two separators;
//                               k_track_seg_back: the back-substitution and, in the last pass, the marginals of the interiors
//   per piece, one wavefront    k_track_sep: the separators' chain (factor, solve, selected inverse); k_track_decide: the cost and the
//                               Levenberg-Marquardt decision of ctag_lm.h
// A 12x12 block is 144 doubles in LDS, entry e owned by lane e % 64; a segment's wave holds the blocks of the frame it works on and the
// ones it carries (SegLds, 13 344 B for every L); the factors of the other frames stream to and from the workspace, which is L2-resident.
// Everything is FP64 VALU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_linalg.h"
#include "ctag_lm.h"
#include "ctag_loss.h"
#include "ctag_m12.h"
#include "ctag_so3.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_track_rec) == 464, "ctag_track_rec layout");
static_assert(sizeof(ctag_track_stat) == 40, "ctag_track_stat layout");
static_assert(sizeof(ctag_track_opts) == 80, "ctag_track_opts layout");

namespace ctag {

constexpr int kTrackDefaultSegment = 64;  // measured: DESIGN.md section 21
constexpr double kTrackRelTol = 1e-12, kTrackLambdaMax = 1e6, kTrackMinPivot = 1e-12;
constexpr int kTrackItemDoubles = 48 + 18 + 18 + 3 * 144 + 12 + 3 * 144 + 24 + 12 + 42 + 4 + 3;  // 1045
constexpr int kTrackItemInts = 10;

struct TrackWs {  // every array has n_items entries of the stated size
    double *Rm, *tm, *W;           // 9, 3, 36: the measurement
    double *X, *XT;                // 18: R, t, w, v of the accepted and of the trial state
    double *D, *C, *Y, *g;         // 144, 144, 144, 12: the frame's blocks, then its factors L, Z, Y, y
    double *SA, *SB, *ST, *gA, *gB;  // separators: the segments' Schur terms, then the chain's factors, then the marginals
    double *delta, *marg;          // 12; 42: the pose marginal and the six velocity sigmas
    double *cterm, *cterm_t, *m2, *wt;
    double *lambda, *cost, *cost0;  // per piece
    int32_t *measured, *pa, *pb, *prevm, *nextm, *active, *rounds, *sing, *seplist, *piecelist;
    int32_t *n_seps, *n_pieces, *bad, *rig_stat;  // per rig; rig_stat: n_measured, n_tracked, longest (3 per rig)
    int n_frames, n_rigs;
};

struct TrackP {
    int loss, max_iterations, max_gap, L;
    double q_rot, q_trans, ivr2, ivt2, a, a2, lambda0;
};


// ---- gather: either record kind to the sample arrays ----------------------------------------------------------------------------------------
template <class Rec>
__global__ __launch_bounds__(256) void k_track_gather(const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov, TrackWs ws) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_items = ws.n_frames * ws.n_rigs;
    if (w >= n_items) return;
    const int f = w / ws.n_rigs, g = w - f * ws.n_rigs;
    const int i = g * ws.n_frames + f;
    const Rec& P = recs[w];
    const ctag_pose_cov_rec& Q = cov[w];
    if (misplaced_or_rvec(P, Q, f, g)) atomicOr(&ws.bad[g], 1);
    ws.measured[i] = measured_sample(P, Q, kTrackMinPivot, ws.Rm + (size_t)i * 9, ws.tm + (size_t)i * 3, ws.W + (size_t)i * 36) ? 1 : 0;
}

// ---- pieces: one wavefront per rig ---------------------------------------------------------------------------------------------------------
// Forwards over 64 frames at a time: the latest measured frame at or before f, the piece starts and the piece each frame would belong
// to; backwards: the earliest measured frame at or after f and the piece ends.  A frame is in a piece when it is measured or its two
// measured neighbours are at most max_gap apart.  Then the lists of pieces and of separators (local frames 0, L, 2L, ... of a piece).
__global__ __launch_bounds__(64) void k_track_pieces(TrackWs ws, int max_gap, int L) {
    const int g = blockIdx.x, lane = threadIdx.x, n = ws.n_frames;
    const size_t base = (size_t)g * n;
    const bool bad = ws.bad[g] != 0;
    int carry_prev = -1, carry_a = -1, n_pieces = 0, n_measured = 0;
    for (int f0 = 0; f0 < n; f0 += 64) {  // wave-uniform
        const int f = f0 + lane;
        const bool m = f < n && !bad && ws.measured[base + f] != 0;
        const unsigned long long M = __builtin_amdgcn_ballot_w64(m);
        const unsigned long long below = M & ((1ull << lane) - 1ull);
        const int prev_strict = below ? f0 + 63 - __builtin_clzll(below) : carry_prev;
        const bool start = m && (prev_strict < 0 || f - prev_strict > max_gap);
        const unsigned long long S = __builtin_amdgcn_ballot_w64(start);
        const unsigned long long upto = S & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int a = upto ? f0 + 63 - __builtin_clzll(upto) : carry_a;
        const int id = n_pieces + wave_incl_scan(start ? 1 : 0) - 1;
        if (f < n) {
            ws.prevm[base + f] = m ? f : prev_strict;
            ws.pa[base + f] = a;
            if (start) ws.piecelist[base + id] = f;
        }
        if (M) carry_prev = f0 + 63 - __builtin_clzll(M);
        if (S) carry_a = f0 + 63 - __builtin_clzll(S);
        n_pieces += __builtin_popcountll(S);
        n_measured += __builtin_popcountll(M);
    }
    int carry_next = -1, carry_b = -1;
    for (int f0 = ((n - 1) / 64) * 64; f0 >= 0; f0 -= 64) {
        const int f = f0 + lane;
        const bool m = f < n && !bad && ws.measured[base + f] != 0;
        const unsigned long long M = __builtin_amdgcn_ballot_w64(m);
        const unsigned long long above = lane == 63 ? 0ull : M & ~((2ull << lane) - 1ull);
        const int next_strict = above ? f0 + __builtin_ctzll(above) : carry_next;
        const bool end = m && (next_strict < 0 || next_strict - f > max_gap);
        const unsigned long long E = __builtin_amdgcn_ballot_w64(end);
        const unsigned long long from = E & ~((1ull << lane) - 1ull);
        const int b = from ? f0 + __builtin_ctzll(from) : carry_b;
        if (f < n) {
            const int nx = m ? f : next_strict;
            const int pv = ws.prevm[base + f];
            const bool in = m || (pv >= 0 && nx >= 0 && nx - pv <= max_gap);
            ws.nextm[base + f] = nx;
            ws.pb[base + f] = in ? b : -1;
            if (!in) ws.pa[base + f] = -1;
        }
        if (M) carry_next = f0 + __builtin_ctzll(M);
        if (E) carry_b = f0 + __builtin_ctzll(E);
    }
    __syncthreads();
    int n_seps = 0, n_tracked = 0, longest = 0;
    for (int f0 = 0; f0 < n; f0 += 64) {
        const int f = f0 + lane;
        const int a = f < n ? ws.pa[base + f] : -1;
        const bool sep = a >= 0 && (f - a) % L == 0;
        const int idx = n_seps + wave_incl_scan(sep ? 1 : 0) - 1;
        if (sep) ws.seplist[base + idx] = f;
        n_seps += __builtin_popcountll(__builtin_amdgcn_ballot_w64(sep));
        n_tracked += __builtin_popcountll(__builtin_amdgcn_ballot_w64(a >= 0));
        int len = a == f ? ws.pb[base + f] - a + 1 : 0;
        double dl = (double)len;
        int who = lane;
        wave_max_f64(dl, who);
        longest = max(longest, (int)dl);
    }
    if (lane == 0) {
        ws.n_seps[g] = n_seps;
        ws.n_pieces[g] = n_pieces;
        ws.rig_stat[g * 3 + 0] = n_measured;
        ws.rig_stat[g * 3 + 1] = n_tracked;
        ws.rig_stat[g * 3 + 2] = longest;
    }
}

// ---- rule 5 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_start_pose(TrackWs ws, const double* __restrict__ times) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ws.n_frames * ws.n_rigs) return;
    const int g = i / ws.n_frames, f = i - g * ws.n_frames;
    if (ws.pa[i] < 0) return;
    double* X = ws.X + (size_t)i * 18;
    if (ws.measured[i]) {
        for (int k = 0; k < 9; k++) X[k] = ws.Rm[(size_t)i * 9 + k];
        for (int k = 0; k < 3; k++) X[9 + k] = ws.tm[(size_t)i * 3 + k];
        return;
    }
    const size_t p = (size_t)g * ws.n_frames + ws.prevm[i], n = (size_t)g * ws.n_frames + ws.nextm[i];
    const double s = (times[f] - times[ws.prevm[i]]) / (times[ws.nextm[i]] - times[ws.prevm[i]]);
    double Rel[9], r[3], E[9];
    mat3_mul_nt(ws.Rm + n * 9, ws.Rm + p * 9, Rel);
    so3_log(Rel, r);
    for (int k = 0; k < 3; k++) r[k] = s * r[k];
    ctl::angle_axis_rot(r, E, nullptr);
    mat3_mul(E, ws.Rm + p * 9, X);
    for (int k = 0; k < 3; k++) X[9 + k] = ws.tm[p * 3 + k] + s * (ws.tm[n * 3 + k] - ws.tm[p * 3 + k]);
}

__global__ __launch_bounds__(256) void k_track_start_vel(TrackWs ws, const double* __restrict__ times) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ws.n_frames * ws.n_rigs) return;
    const int g = i / ws.n_frames, f = i - g * ws.n_frames;
    const int a = ws.pa[i], b = ws.pb[i];
    if (a < 0) return;
    double* X = ws.X + (size_t)i * 18;
    if (a == b) {
        for (int k = 0; k < 6; k++) X[12 + k] = 0.0;
        return;
    }
    const int f0 = f < b ? f : f - 1;  // the last frame copies its predecessor's
    const double* X0 = ws.X + ((size_t)g * ws.n_frames + f0) * 18;
    const double* X1 = X0 + 18;
    const double dt = times[f0 + 1] - times[f0];
    double Rel[9], r[3];
    mat3_mul_nt(X1, X0, Rel);
    so3_log(Rel, r);
    for (int k = 0; k < 3; k++) {
        X[12 + k] = r[k] / dt;
        X[15 + k] = (X1[9 + k] - X0[9 + k]) / dt;
    }
}

// ---- rule 4 at one frame: its cost term, and with LIN its blocks -----------------------------------------------------------------------------
__device__ __forceinline__ void put3(double* M, int bi, int bj, const double* B, double sc) {  // block (bi, bj) = sc B, block (bj, bi) its transpose
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v = sc * B[r * 3 + c];
            M[(3 * bi + r) * 12 + 3 * bj + c] = v;
            M[(3 * bj + c) * 12 + 3 * bi + r] = v;
        }
}
__device__ __forceinline__ void put3_one(double* M, int bi, int bj, const double* B, double sc) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[(3 * bi + r) * 12 + 3 * bj + c] = sc * B[r * 3 + c];
}

struct Motion {  // the motion term between X0 and X1
    double A[9];            // Jl^-1(psi)
    double ma[6], mb[6];    // M r: rows of a, rows of b
    double al[2], be[2], ga[2], de[2];  // 12 / (q D^3), 6 / (q D^2), 4 / (q D), 2 / (q D) for rotation, translation
    double dt, cost;
};
__device__ __forceinline__ void motion_term(const double* X0, const double* X1, double dt, const TrackP& P, Motion& m) {
    double Rel[9], psi[3], a[6], b[6];
    mat3_mul_nt(X1, X0, Rel);
    so3_log(Rel, psi);
    so3_jlinv(psi, m.A);
    for (int k = 0; k < 3; k++) {
        a[k] = psi[k] - dt * X0[12 + k];
        a[3 + k] = X1[9 + k] - X0[9 + k] - dt * X0[15 + k];
        b[k] = X1[12 + k] - X0[12 + k];
        b[3 + k] = X1[15 + k] - X0[15 + k];
    }
    m.dt = dt;
    m.cost = 0.0;
    for (int h = 0; h < 2; h++) {
        const double q = h == 0 ? P.q_rot : P.q_trans;
        m.al[h] = 12.0 / (q * dt * dt * dt);
        m.be[h] = 6.0 / (q * dt * dt);
        m.ga[h] = 4.0 / (q * dt);
        m.de[h] = 2.0 / (q * dt);
        for (int k = 3 * h; k < 3 * h + 3; k++) {
            m.ma[k] = m.al[h] * a[k] - m.be[h] * b[k];
            m.mb[k] = m.ga[h] * b[k] - m.be[h] * a[k];
            m.cost += (m.al[h] * a[k] * a[k] - 2.0 * m.be[h] * a[k] * b[k]) + m.ga[h] * b[k] * b[k];
        }
    }
}

template <bool LIN>
__global__ __launch_bounds__(128) void k_track_lin(TrackWs ws, const double* __restrict__ times, TrackP P, int trial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ws.n_frames * ws.n_rigs) return;
    const int g = i / ws.n_frames, f = i - g * ws.n_frames;
    const int a = ws.pa[i], b = ws.pb[i];
    if (a < 0) return;
    if (trial && !ws.active[(size_t)g * ws.n_frames + a]) return;  // no trial was made for a piece that has stopped
    const double* XS = trial ? ws.XT : ws.X;
    const double* X = XS + (size_t)i * 18;
    double cost = 0.0, grad[12], Htt[9], Hrt[9], Hrr[9], Hrw[9];
    double dtt = 0.0, dtv = 0.0, dww = 0.0, dvv = 0.0;
    for (int k = 0; k < 12; k++) grad[k] = 0.0;
    for (int k = 0; k < 9; k++) Htt[k] = Hrt[k] = Hrr[k] = Hrw[k] = 0.0;
    double m2 = 0.0, wt = 1.0;
    if (ws.measured[i]) {
        const double* W = ws.W + (size_t)i * 36;
        double Rel[9], e[6], We[6], J[9], rho = 0.0;
        mat3_mul_nt(X, ws.Rm + (size_t)i * 9, Rel);
        so3_log(Rel, e);
        for (int k = 0; k < 3; k++) e[3 + k] = X[9 + k] - ws.tm[(size_t)i * 3 + k];
        for (int r = 0; r < 6; r++) {
            double s = 0.0;
            for (int c = 0; c < 6; c++) s += W[r * 6 + c] * e[c];
            We[r] = s;
            m2 += e[r] * s;
        }
        if (P.loss == CTAG_TRACK_LOSS_NONE) rho = m2;
        else robust_loss(P.loss, P.a, P.a2, m2, rho, wt);
        cost += rho;
        if (LIN) {
            so3_jlinv(e, J);
            double T[9];  // Wrr J
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) T[r * 3 + c] = W[r * 6] * J[c] + W[r * 6 + 1] * J[3 + c] + W[r * 6 + 2] * J[6 + c];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) {
                    Hrr[r * 3 + c] = wt * (J[r] * T[c] + J[3 + r] * T[3 + c] + J[6 + r] * T[6 + c]);
                    Hrt[r * 3 + c] = wt * (J[r] * W[3 + c] + J[3 + r] * W[6 + 3 + c] + J[6 + r] * W[12 + 3 + c]);
                    Htt[r * 3 + c] = wt * W[(3 + r) * 6 + 3 + c];
                }
            for (int r = 0; r < 3; r++) {
                grad[r] = wt * (J[r] * We[0] + J[3 + r] * We[1] + J[6 + r] * We[2]);
                grad[3 + r] = wt * We[3 + r];
            }
        }
    }
    if (f == a) {
        for (int k = 0; k < 3; k++) {
            cost += P.ivr2 * X[12 + k] * X[12 + k] + P.ivt2 * X[15 + k] * X[15 + k];
            grad[6 + k] += P.ivr2 * X[12 + k];
            grad[9 + k] += P.ivt2 * X[15 + k];
        }
        dww += P.ivr2;
        dvv += P.ivt2;
    }
    double* C = ws.C + (size_t)i * 144;
    if (LIN)
        for (int k = 0; k < 144; k++) C[k] = 0.0;
    if (f < b) {  // the term to the next frame: this frame is its first
        Motion m;
        motion_term(X, X + 18, times[f + 1] - times[f], P, m);
        cost += m.cost;
        if (LIN) {
            double At[9], AAt[9], AtAt[9];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) At[r * 3 + c] = m.A[c * 3 + r];
            mat3_mul_nt(m.A, m.A, AAt);
            mat3_mul(At, At, AtAt);
            for (int r = 0; r < 3; r++) {
                grad[r] -= m.A[r * 3] * m.ma[0] + m.A[r * 3 + 1] * m.ma[1] + m.A[r * 3 + 2] * m.ma[2];
                grad[3 + r] -= m.ma[3 + r];
                grad[6 + r] -= m.dt * m.ma[r] + m.mb[r];
                grad[9 + r] -= m.dt * m.ma[3 + r] + m.mb[3 + r];
            }
            for (int k = 0; k < 9; k++) {
                Hrr[k] += m.al[0] * AAt[k];
                Hrw[k] += m.be[0] * m.A[k];
            }
            dtt += m.al[1];
            dtv += m.be[1];
            dww += m.ga[0];
            dvv += m.ga[1];
            const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            put3_one(C, 0, 0, AtAt, -m.al[0]);  // rows: the next frame's theta, t, w, v; columns: this frame's
            put3_one(C, 0, 2, At, -m.be[0]);
            put3_one(C, 2, 0, At, m.be[0]);
            put3_one(C, 2, 2, I3, m.de[0]);
            put3_one(C, 1, 1, I3, -m.al[1]);
            put3_one(C, 1, 3, I3, -m.be[1]);
            put3_one(C, 3, 1, I3, m.be[1]);
            put3_one(C, 3, 3, I3, m.de[1]);
        }
    }
    if (LIN && f > a) {  // the term from the previous frame: this frame is its second
        Motion m;
        motion_term(X - 18, X, times[f] - times[f - 1], P, m);
        double At[9], AtA[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) At[r * 3 + c] = m.A[c * 3 + r];
        mat3_mul(At, m.A, AtA);
        for (int r = 0; r < 3; r++) {
            grad[r] += At[r * 3] * m.ma[0] + At[r * 3 + 1] * m.ma[1] + At[r * 3 + 2] * m.ma[2];
            grad[3 + r] += m.ma[3 + r];
            grad[6 + r] += m.mb[r];
            grad[9 + r] += m.mb[3 + r];
        }
        for (int k = 0; k < 9; k++) {
            Hrr[k] += m.al[0] * AtA[k];
            Hrw[k] -= m.be[0] * At[k];
        }
        dtt += m.al[1];
        dtv -= m.be[1];
        dww += m.ga[0];
        dvv += m.ga[1];
    }
    if (trial) {
        ws.cterm_t[i] = 0.5 * cost;
        return;
    }
    ws.cterm[i] = 0.5 * cost;
    ws.m2[i] = m2;
    ws.wt[i] = wt;
    if (LIN) {
        double* D = ws.D + (size_t)i * 144;
        for (int k = 0; k < 144; k++) D[k] = 0.0;
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int k = 0; k < 9; k++) Htt[k] += dtt * I3[k];
        // Hrr and Htt are symmetric up to rounding: the lower triangle is what the factorisation reads
        put3_one(D, 0, 0, Hrr, 1.0);
        put3_one(D, 1, 1, Htt, 1.0);
        put3(D, 0, 1, Hrt, 1.0);
        put3(D, 0, 2, Hrw, 1.0);
        put3(D, 1, 3, I3, dtv);
        put3_one(D, 2, 2, I3, dww);
        put3_one(D, 3, 3, I3, dvv);
        for (int k = 0; k < 12; k++) ws.g[(size_t)i * 12 + k] = -grad[k];
    }
}

// ---- 12x12 blocks in LDS: entry e of a block belongs to lane e % 64; one wavefront per block of threads --------------------------------------
struct SegLds {
    M12 Dm, F[2], Z[2], acc, tmp, P, Pnn, Pns, Pss;
    double y[2][12], gacc[12], tv[12], ds[12], dn[12];
};

// ---- a segment: the frames between separator s (local frame k L of its piece) and the next one -------------------------------------------------
__global__ __launch_bounds__(64) void k_track_seg_factor(TrackWs ws, int L, int final_pass, int per_rig) {
    __shared__ SegLds S;
    const int g = blockIdx.x / per_rig, lane = threadIdx.x;  // per_rig blocks a rig, striding over its list
    const size_t base = (size_t)g * ws.n_frames;
    const int n_seps = ws.n_seps[g];
    for (int q = blockIdx.x % per_rig; q < n_seps; q += per_rig) {
        const int s = ws.seplist[base + q];
        const int a = ws.pa[base + s], b = ws.pb[base + s];
        if (!final_pass && !ws.active[base + a]) continue;
        const double damp = final_pass ? 1.0 : 1.0 + ws.lambda[base + a];
        const int last = min(s + L - 1, b);  // the last interior frame
        const bool right = s + L <= b;
        bool ok = true;
        tsync();
        m_zero(S.acc, lane);
        if (lane < 12) S.gacc[lane] = 0.0;
        int cur = 0;
        for (int f = s + 1; f <= last; f++, cur ^= 1) {
            const size_t i = base + f;
            tsync();
            m_load(S.Dm, ws.D + i * 144, lane, damp);
            m_load_t(S.Z[cur], ws.C + i * 144, lane);  // A[x_f, x_f+1] = C_f^T
            if (lane < 12) S.y[cur][lane] = ws.g[i * 12 + lane];
            if (f == s + 1) {
                m_load(S.F[cur], ws.C + (i - 1) * 144, lane);  // A[x_1, s] = C_s
                tsync();
            } else {
                tsync();
                m_mul<true, false>(S.tmp, S.Z[cur ^ 1], S.Z[cur ^ 1], -1.0, &S.Dm, lane);
                m_mul<true, false>(S.F[cur], S.Z[cur ^ 1], S.F[cur ^ 1], -1.0, nullptr, lane);
                m_vec<true>(S.y[cur], S.Z[cur ^ 1], S.y[cur ^ 1], -1.0, S.y[cur], lane);
                tsync();
                for (int e = lane; e < 144; e += 64) S.Dm.v[e] = S.tmp.v[e];
            }
            ok = m_chol(S.Dm, lane) && ok;
            m_solve<true>(S.Dm, &S.F[cur], &S.Z[cur], S.y[cur], lane);
            tsync();
            m_mul<true, false>(S.tmp, S.F[cur], S.F[cur], 1.0, &S.acc, lane);
            m_vec<true>(S.tv, S.F[cur], S.y[cur], 1.0, S.gacc, lane);
            m_store(ws.D + i * 144, S.Dm, lane);
            m_store(ws.C + i * 144, S.Z[cur], lane);
            m_store(ws.Y + i * 144, S.F[cur], lane);
            if (lane < 12) ws.g[i * 12 + lane] = S.y[cur][lane];
            tsync();
            for (int e = lane; e < 144; e += 64) S.acc.v[e] = S.tmp.v[e];
            if (lane < 12) S.gacc[lane] = S.tv[lane];
        }
        tsync();
        m_store(ws.SA + (base + s) * 144, S.acc, lane);
        if (lane < 12) ws.gA[(base + s) * 12 + lane] = S.gacc[lane];
        if (right) {  // last == s + L - 1 >= s + 1: the loop ran, cur ^ 1 is its last frame
            const int c = cur ^ 1;
            const size_t r = base + s + L;
            m_mul<true, false>(S.tmp, S.Z[c], S.Z[c], 1.0, nullptr, lane);
            m_store(ws.SB + r * 144, S.tmp, lane);
            tsync();
            m_mul<true, false>(S.tmp, S.Z[c], S.F[c], -1.0, nullptr, lane);  // A[s', s]
            m_vec<true>(S.tv, S.Z[c], S.y[c], 1.0, nullptr, lane);
            m_store(ws.ST + r * 144, S.tmp, lane);
            if (lane < 12) ws.gB[r * 12 + lane] = S.tv[lane];
        }
        if (!ok && lane == 0) atomicOr(&ws.sing[base + a], 1);
    }
}

// ---- a piece's separators: factor the chain, solve it, and in the last pass its selected inverse -----------------------------------------------
__global__ __launch_bounds__(64) void k_track_sep(TrackWs ws, int L, int final_pass, int per_rig) {
    __shared__ SegLds S;
    const int g = blockIdx.x / per_rig, lane = threadIdx.x;  // per_rig blocks a rig, striding over its list
    const size_t base = (size_t)g * ws.n_frames;
    const int n_pieces = ws.n_pieces[g];
    for (int q = blockIdx.x % per_rig; q < n_pieces; q += per_rig) {
        const int a = ws.piecelist[base + q], b = ws.pb[base + a];
        if (!final_pass && !ws.active[base + a]) continue;
        const double damp = final_pass ? 1.0 : 1.0 + ws.lambda[base + a];
        const int K = (b - a) / L + 1;
        bool ok = true;
        int cur = 0;
        for (int k = 0; k < K; k++, cur ^= 1) {  // Z[cur]: Ls_k^-1 T_k^T, y[cur]: ys_k
            const size_t i = base + a + (size_t)k * L;
            tsync();
            m_load(S.Dm, ws.D + i * 144, lane, damp);
            m_load(S.F[0], ws.SA + i * 144, lane);
            if (lane < 12) S.tv[lane] = ws.g[i * 12 + lane] - ws.gA[i * 12 + lane];
            if (k > 0) {
                m_load(S.F[1], ws.SB + i * 144, lane);
                if (lane < 12) S.tv[lane] = S.tv[lane] - ws.gB[i * 12 + lane];
            }
            tsync();
            for (int e = lane; e < 144; e += 64) S.Dm.v[e] = k > 0 ? (S.Dm.v[e] - S.F[0].v[e]) - S.F[1].v[e] : S.Dm.v[e] - S.F[0].v[e];
            tsync();
            if (k > 0) {
                m_mul<true, false>(S.tmp, S.Z[cur ^ 1], S.Z[cur ^ 1], -1.0, &S.Dm, lane);
                m_vec<true>(S.y[cur], S.Z[cur ^ 1], S.y[cur ^ 1], -1.0, S.tv, lane);
                tsync();
                for (int e = lane; e < 144; e += 64) S.Dm.v[e] = S.tmp.v[e];
            } else if (lane < 12) {
                S.y[cur][lane] = S.tv[lane];
            }
            if (k + 1 < K) m_load_t(S.Z[cur], ws.ST + (i + L) * 144, lane);  // T_k^T: rows s_k, columns s_k+1
            ok = m_chol(S.Dm, lane) && ok;
            m_solve<true>(S.Dm, nullptr, k + 1 < K ? &S.Z[cur] : nullptr, S.y[cur], lane);
            tsync();
            m_store(ws.SA + i * 144, S.Dm, lane);
            if (lane < 12) ws.gA[i * 12 + lane] = S.y[cur][lane];
            if (k + 1 < K) m_store(ws.ST + (i + L) * 144, S.Z[cur], lane);
        }
        if (!ok && lane == 0) atomicOr(&ws.sing[base + a], 1);
        // backwards: delta_k = Ls^-T (ys - Zs_k delta_k+1); P = Sigma_k, Pnn = Sigma_k+1
        for (int k = K - 1; k >= 0; k--) {
            const size_t i = base + a + (size_t)k * L;
            tsync();
            m_load(S.Dm, ws.SA + i * 144, lane);
            if (k + 1 < K) m_load(S.Z[0], ws.ST + (i + L) * 144, lane);
            if (lane < 12) S.tv[lane] = ws.gA[i * 12 + lane];
            tsync();
            if (k + 1 < K) {
                m_vec<false>(S.ds, S.Z[0], S.dn, -1.0, S.tv, lane);
            } else if (lane < 12) {
                S.ds[lane] = S.tv[lane];
            }
            tsync();
            m_solve<false>(S.Dm, nullptr, nullptr, S.ds, lane);
            tsync();
            if (lane < 12) {
                ws.delta[i * 12 + lane] = S.ds[lane];
                S.dn[lane] = S.ds[lane];
            }
            if (final_pass) {
                m_identity(S.F[0], lane);
                tsync();
                m_solve<true>(S.Dm, &S.F[0], nullptr, nullptr, lane);  // Ls^-1
                if (k + 1 < K) m_solve<false>(S.Dm, nullptr, &S.Z[0], nullptr, lane);  // G = Ls^-T Zs_k
                tsync();
                m_mul<true, false>(S.tmp, S.F[0], S.F[0], 1.0, nullptr, lane);
                if (k + 1 < K) {
                    m_mul<false, false>(S.F[1], S.Z[0], S.Pnn, 1.0, nullptr, lane);  // U = G Sigma_k+1 = -Sigma_k,k+1
                    tsync();
                    m_mul<false, true>(S.P, S.F[1], S.Z[0], 1.0, &S.tmp, lane);
                    for (int e = lane; e < 144; e += 64) ws.ST[(i + L) * 144 + e] = -S.F[1].v[e];  // Sigma_k,k+1: rows s_k, columns s_k+1
                } else {
                    tsync();
                    for (int e = lane; e < 144; e += 64) S.P.v[e] = S.tmp.v[e];
                }
                tsync();
                m_sym(S.Pnn, S.P, lane);
                tsync();
                m_store(ws.SA + i * 144, S.Pnn, lane);
                marg_store(ws.marg + i * 42, S.Pnn, lane);
            }
        }
    }
}

// ---- a segment again: back-substitution and, in the last pass, the interiors' marginals conditioned on the two separators ---------------------
__global__ __launch_bounds__(64) void k_track_seg_back(TrackWs ws, int L, int final_pass, int per_rig) {
    __shared__ SegLds S;
    const int g = blockIdx.x / per_rig, lane = threadIdx.x;  // per_rig blocks a rig, striding over its list
    const size_t base = (size_t)g * ws.n_frames;
    const int n_seps = ws.n_seps[g];
    for (int q = blockIdx.x % per_rig; q < n_seps; q += per_rig) {
        const int s = ws.seplist[base + q];
        const int a = ws.pa[base + s], b = ws.pb[base + s];
        if (!final_pass && !ws.active[base + a]) continue;
        const int last = min(s + L - 1, b);
        const bool right = s + L <= b;
        tsync();
        if (lane < 12) {
            S.ds[lane] = ws.delta[(base + s) * 12 + lane];
            S.dn[lane] = right ? ws.delta[(base + s + L) * 12 + lane] : 0.0;
        }
        if (final_pass) {
            m_load(S.Pss, ws.SA + (base + s) * 144, lane);
            if (right) {
                m_load(S.Pnn, ws.SA + (base + s + L) * 144, lane);
                m_load_t(S.Pns, ws.ST + (base + s + L) * 144, lane);  // rows s', columns s
            } else {
                m_zero(S.Pnn, lane);
                m_zero(S.Pns, lane);
            }
        }
        for (int f = last; f > s; f--) {
            const size_t i = base + f;
            tsync();
            m_load(S.Dm, ws.D + i * 144, lane);
            m_load(S.Z[0], ws.C + i * 144, lane);
            m_load(S.F[0], ws.Y + i * 144, lane);
            if (lane < 12) S.tv[lane] = ws.g[i * 12 + lane];
            tsync();
            m_vec<false>(S.y[0], S.Z[0], S.dn, -1.0, S.tv, lane);
            tsync();
            m_vec<false>(S.y[1], S.F[0], S.ds, -1.0, S.y[0], lane);
            tsync();
            m_solve<false>(S.Dm, nullptr, nullptr, S.y[1], lane);
            tsync();
            if (lane < 12) {
                ws.delta[i * 12 + lane] = S.y[1][lane];
                S.dn[lane] = S.y[1][lane];
            }
            if (final_pass) {
                m_identity(S.Z[1], lane);
                tsync();
                m_solve<false>(S.Dm, &S.Z[0], &S.F[0], nullptr, lane);  // Ga = L^-T Z, Gb = L^-T Y
                tsync();
                m_solve<true>(S.Dm, &S.Z[1], nullptr, nullptr, lane);   // L^-1
                tsync();
                m_mul<false, false>(S.tmp, S.Z[0], S.Pnn, 1.0, nullptr, lane);
                m_mul<false, false>(S.acc, S.Z[0], S.Pns, 1.0, nullptr, lane);
                m_mul<true, false>(S.P, S.Z[1], S.Z[1], 1.0, nullptr, lane);
                tsync();
                m_mul<false, true>(S.F[1], S.F[0], S.Pns, 1.0, &S.tmp, lane);   // U = Ga Pnn + Gb Pns^T
                m_mul<false, false>(S.tmp, S.F[0], S.Pss, 1.0, &S.acc, lane);   // V = Ga Pns + Gb Pss  (tmp is read entry-wise only: its own entry)
                tsync();
                m_mul<false, true>(S.acc, S.F[1], S.Z[0], 1.0, &S.P, lane);     // + U Ga^T
                tsync();
                m_mul<false, true>(S.P, S.tmp, S.F[0], 1.0, &S.acc, lane);      // + V Gb^T
                tsync();
                m_sym(S.Pnn, S.P, lane);
                for (int e = lane; e < 144; e += 64) S.Pns.v[e] = -S.tmp.v[e];  // Sigma_f,s
                tsync();
                marg_store(ws.marg + i * 42, S.Pnn, lane);
            }
        }
    }
}

// ---- the trial state: X (+) delta ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_trial(TrackWs ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ws.n_frames * ws.n_rigs) return;
    const int a = ws.pa[i];
    if (a < 0) return;
    const int g = i / ws.n_frames;
    if (!ws.active[(size_t)g * ws.n_frames + a]) return;
    const double* X = ws.X + (size_t)i * 18;
    const double* d = ws.delta + (size_t)i * 12;
    double* T = ws.XT + (size_t)i * 18;
    double E[9];
    ctl::angle_axis_rot(d, E, nullptr);
    mat3_mul(E, X, T);
    for (int k = 0; k < 9; k++) T[9 + k] = X[9 + k] + d[3 + k];
}

// ---- a piece's cost and decision: mode 0 takes the start's cost, mode 1 decides the round -----------------------------------------------------
__global__ __launch_bounds__(64) void k_track_decide(TrackWs ws, TrackP P, int mode, int per_rig) {
    const int g = blockIdx.x / per_rig, lane = threadIdx.x;  // per_rig blocks a rig, striding over its list
    const size_t base = (size_t)g * ws.n_frames;
    const int n_pieces = ws.n_pieces[g];
    for (int q = blockIdx.x % per_rig; q < n_pieces; q += per_rig) {
        const int a = ws.piecelist[base + q], b = ws.pb[base + a];
        if (mode == 1 && !ws.active[base + a]) continue;
        const double* term = mode == 0 ? ws.cterm : ws.cterm_t;
        double c = 0.0;
        for (int f = a + lane; f <= b; f += 64) c += term[base + f];
        c = wave_sum_f64(c);
        if (mode == 0) {
            if (lane == 0) {
                ws.cost0[base + a] = c;
                ws.cost[base + a] = c;
                ws.lambda[base + a] = P.lambda0;
                ws.active[base + a] = 1;
                ws.rounds[base + a] = 0;
                ws.sing[base + a] = 0;
            }
            continue;
        }
        LmState st{ws.lambda[base + a], ws.cost[base + a], 1, ws.rounds[base + a]};
        const bool usable = ws.sing[base + a] == 0 && ctl::finite64(c);
        const bool accept = lm_decide(st, usable, c, kTrackRelTol, kTrackLambdaMax, P.max_iterations);
        if (accept)
            for (size_t k = (base + a) * 18 + lane; k < (base + b + 1) * 18; k += 64) ws.X[k] = ws.XT[k];
        if (lane == 0) {
            ws.lambda[base + a] = st.lambda;
            ws.cost[base + a] = st.cost;
            ws.active[base + a] = st.active;
            ws.rounds[base + a] = st.rounds;
            ws.sing[base + a] = 0;
        }
    }
}

// ---- the records --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_write(TrackWs ws, ctag_track_rec* __restrict__ out) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= ws.n_frames * ws.n_rigs) return;
    const int f = w / ws.n_rigs, g = w - f * ws.n_rigs;
    const size_t i = (size_t)g * ws.n_frames + f;
    ctag_track_rec r;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(&r);
    for (int k = 0; k < (int)(sizeof(r) / 8); k++) words[k] = 0ull;
    r.rig = g;
    r.frame = f;
    const int a = ws.pa[i];
    if (ws.bad[g]) {
        r.status = CTAG_TRACK_BAD_INPUT;
    } else if (a < 0) {
        r.status = CTAG_TRACK_NOT_TRACKED;
    } else {
        const size_t pa = (size_t)g * ws.n_frames + a;
        const bool sing = ws.sing[pa] != 0 || !ctl::finite64(ws.cost[pa]);
        r.status = sing ? CTAG_TRACK_SINGULAR : CTAG_TRACK_OK;
        const double* X = ws.X + i * 18;
        so3_log(X, r.rvec);
        for (int k = 0; k < 3; k++) {
            r.tvec[k] = X[9 + k];
            r.w[k] = X[12 + k];
            r.v[k] = X[15 + k];
        }
        if (!sing) {
            for (int k = 0; k < 36; k++) r.cov[k] = ws.marg[i * 42 + k];
            for (int k = 0; k < 6; k++) r.vel_sigma[k] = ws.marg[i * 42 + 36 + k];
        }
        r.weight = 1.0;
        if (ws.measured[i]) {
            r.mahalanobis2 = ws.m2[i];
            r.weight = ws.wt[i];
            r.flags = CTAG_TRACK_FLAG_MEASURED | (ws.wt[i] < 1.0 ? CTAG_TRACK_FLAG_DOWNWEIGHTED : 0u);
        }
    }
    out[w] = r;
}

__global__ __launch_bounds__(64) void k_track_stat(TrackWs ws, ctag_track_stat* __restrict__ out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ws.n_rigs) return;
    const size_t base = (size_t)g * ws.n_frames;
    ctag_track_stat s;
    s.status = ws.bad[g] ? CTAG_TRACK_BAD_INPUT : CTAG_TRACK_OK;
    s.n_measured = s.n_pieces = s.n_tracked = s.longest_piece = s.rounds = 0;
    s.cost0 = s.cost = 0.0;
    if (!ws.bad[g]) {
        s.n_measured = ws.rig_stat[g * 3];
        s.n_tracked = ws.rig_stat[g * 3 + 1];
        s.longest_piece = ws.rig_stat[g * 3 + 2];
        s.n_pieces = ws.n_pieces[g];
        for (int q = 0; q < s.n_pieces; q++) {  // piece order
            const size_t pa = base + ws.piecelist[base + q];
            s.rounds += ws.rounds[pa];
            s.cost0 += ws.cost0[pa];
            s.cost += ws.cost[pa];
        }
    }
    out[g] = s;
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
namespace {

struct TrackState {
    ctag::DevBuf<double> d_ws, d_times;
    ctag::DevBuf<int32_t> d_int;
    ctag::DevBuf<unsigned char> d_in;          // the host forms' records
    ctag::DevBuf<ctag_pose_cov_rec> d_cov;
    ctag::DevBuf<ctag_track_rec> d_out;
    ctag::DevBuf<ctag_track_stat> d_stat;
    std::vector<double> times;                 // the times of the call in flight: the caller's array may go once the call returns
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t done = nullptr;                 // behind the last smoothing call's kernels: the workspace and `times` are free again
    bool in_flight = false;
    bool timed = false;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
};

void track_state_free(void* p) {
    TrackState* s = static_cast<TrackState*>(p);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->done) (void)hipEventDestroy(s->done);
    delete s;
}

TrackState* track_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kTrackState, track_state_free);
    if (!*slot) {
        TrackState* s = new (std::nothrow) TrackState();
        if (!s) return nullptr;
        for (auto& e : s->ev)
            if (hipEventCreate(&e) != hipSuccess) {
                track_state_free(s);
                return nullptr;
            }
        if (hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess) {
            track_state_free(s);
            return nullptr;
        }
        *slot = s;
    }
    return static_cast<TrackState*>(*slot);
}

bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }

int track_opts(const ctag_track_opts* o, ctag::TrackP& p, double& dt) {
    ctag_track_opts d;
    ctag_track_opts_default(&d);
    if (!o) o = &d;
    if (o->struct_size != sizeof(ctag_track_opts)) return CTAG_ERR_ARG;
    if (o->loss != CTAG_LOSS_HUBER && o->loss != CTAG_LOSS_CAUCHY && o->loss != CTAG_TRACK_LOSS_NONE) return CTAG_ERR_ARG;
    if (o->max_iterations < 1 || o->max_gap < 1) return CTAG_ERR_ARG;
    const int L = o->segment_frames;
    if (L != 0 && L != 8 && L != 16 && L != 32 && L != 64) return CTAG_ERR_ARG;
    for (double v : {o->dt, o->q_rot, o->q_trans, o->vel0_sigma_rot, o->vel0_sigma_trans, o->loss_scale})
        if (!pos_finite(v)) return CTAG_ERR_ARG;
    if (!std::isfinite(o->lambda0) || o->lambda0 < 0.0) return CTAG_ERR_ARG;
    p.loss = o->loss;
    p.max_iterations = o->max_iterations;
    p.max_gap = o->max_gap;
    p.L = L ? L : ctag::kTrackDefaultSegment;
    p.q_rot = o->q_rot;
    p.q_trans = o->q_trans;
    p.ivr2 = 1.0 / (o->vel0_sigma_rot * o->vel0_sigma_rot);
    p.ivt2 = 1.0 / (o->vel0_sigma_trans * o->vel0_sigma_trans);
    p.a = o->loss_scale;
    p.a2 = o->loss_scale * o->loss_scale;
    p.lambda0 = o->lambda0;
    dt = o->dt;
    return CTAG_OK;
}

// the workspace of n_items items carved out of the two buffers
void track_carve(TrackState* st, int n_frames, int n_rigs, ctag::TrackWs& ws) {
    const size_t n = (size_t)n_frames * n_rigs;
    double* d = st->d_ws.p;
    auto take = [&](size_t per) {
        double* r = d;
        d += per * n;
        return r;
    };
    ws.Rm = take(9), ws.tm = take(3), ws.W = take(36), ws.X = take(18), ws.XT = take(18);
    ws.D = take(144), ws.C = take(144), ws.Y = take(144), ws.g = take(12);
    ws.SA = take(144), ws.SB = take(144), ws.ST = take(144), ws.gA = take(12), ws.gB = take(12);
    ws.delta = take(12), ws.marg = take(42);
    ws.cterm = take(1), ws.cterm_t = take(1), ws.m2 = take(1), ws.wt = take(1);
    ws.lambda = take(1), ws.cost = take(1), ws.cost0 = take(1);
    int32_t* q = st->d_int.p;
    auto itake = [&](size_t count) {
        int32_t* r = q;
        q += count;
        return r;
    };
    ws.measured = itake(n), ws.pa = itake(n), ws.pb = itake(n), ws.prevm = itake(n), ws.nextm = itake(n);
    ws.active = itake(n), ws.rounds = itake(n), ws.sing = itake(n), ws.seplist = itake(n), ws.piecelist = itake(n);
    ws.n_seps = itake(n_rigs), ws.n_pieces = itake(n_rigs), ws.bad = itake(n_rigs), ws.rig_stat = itake(3 * (size_t)n_rigs);
    ws.n_frames = n_frames;
    ws.n_rigs = n_rigs;
}

template <class Rec>
int track_device(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs_dev, const ctag_pose_cov_rec* cov_dev, int n_frames, const double* times,
                 const ctag_track_opts* opts, ctag_track_rec* out_dev, ctag_track_stat* stat_dev) {
    if (!h || !rigs || !recs_dev || !cov_dev || n_frames < 1 || !out_dev || !stat_dev) return CTAG_ERR_ARG;
    ctag::TrackP P;
    double dt = 0.0;
    if (track_opts(opts, P, dt) != CTAG_OK) return CTAG_ERR_ARG;
    const int n_rigs = rigs->n_rigs;
    const long long n_items = (long long)n_frames * n_rigs;
    if (n_rigs < 1 || n_items > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    if (times) {
        for (int f = 0; f < n_frames; f++)
            if (!std::isfinite(times[f]) || (f > 0 && !(times[f] > times[f - 1]))) return CTAG_ERR_ARG;
    }
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    TrackState* st = track_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    // an earlier smoothing call's kernels may still read the workspace and the times: that call is waited for, nothing else on the stream is
    if (st->in_flight && hipEventSynchronize(st->done) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = false;
    const size_t n = (size_t)n_items;
    if (st->d_ws.grow(n * ctag::kTrackItemDoubles) != hipSuccess || st->d_int.grow(n * ctag::kTrackItemInts + 6 * (size_t)n_rigs) != hipSuccess ||
        st->d_times.grow((size_t)n_frames) != hipSuccess)
        return CTAG_ERR_HIP;
    st->times.resize(n_frames);
    for (int f = 0; f < n_frames; f++) st->times[f] = times ? times[f] : (double)f * dt;
    if (hipMemcpyAsync(st->d_times.p, st->times.data(), sizeof(double) * (size_t)n_frames, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    ctag::TrackWs ws;
    track_carve(st, n_frames, n_rigs, ws);
    if (hipMemsetAsync(ws.bad, 0, sizeof(int32_t) * (size_t)n_rigs, s) != hipSuccess) return CTAG_ERR_HIP;
    const bool timing = ctag::handle_timing(h);
    st->timed = timing;
    auto mark = [&](int k) { return !timing || hipEventRecord(st->ev[k], s) == hipSuccess; };
    const int L = P.L;
    const dim3 per_item((unsigned)((n + 255) / 256)), per_item128((unsigned)((n + 127) / 128));
    // blocks a rig for the segment and the piece kernels (they stride over the rig's lists): a rig of one piece has n_frames / L + 1 segments
    const int seg_rig = std::min(n_frames, n_frames / L + 16), piece_rig = std::min(n_frames, 16);
    const dim3 per_seg((unsigned)seg_rig * (unsigned)n_rigs), per_piece((unsigned)piece_rig * (unsigned)n_rigs);
    const double* T = st->d_times.p;
    if (!mark(0)) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_track_gather<Rec>, per_item, dim3(256), 0, s, recs_dev, cov_dev, ws);
    hipLaunchKernelGGL(ctag::k_track_pieces, dim3(n_rigs), dim3(64), 0, s, ws, P.max_gap, L);
    hipLaunchKernelGGL(ctag::k_track_start_pose, per_item, dim3(256), 0, s, ws, T);
    hipLaunchKernelGGL(ctag::k_track_start_vel, per_item, dim3(256), 0, s, ws, T);
    hipLaunchKernelGGL(ctag::k_track_lin<true>, per_item128, dim3(128), 0, s, ws, T, P, 0);
    hipLaunchKernelGGL(ctag::k_track_decide, per_piece, dim3(64), 0, s, ws, P, 0, piece_rig);
    if (!mark(1)) return CTAG_ERR_HIP;
    for (int round = 0; round < P.max_iterations; round++) {
        if (round > 0) hipLaunchKernelGGL(ctag::k_track_lin<true>, per_item128, dim3(128), 0, s, ws, T, P, 0);
        hipLaunchKernelGGL(ctag::k_track_seg_factor, per_seg, dim3(64), 0, s, ws, L, 0, seg_rig);
        hipLaunchKernelGGL(ctag::k_track_sep, per_piece, dim3(64), 0, s, ws, L, 0, piece_rig);
        hipLaunchKernelGGL(ctag::k_track_seg_back, per_seg, dim3(64), 0, s, ws, L, 0, seg_rig);
        hipLaunchKernelGGL(ctag::k_track_trial, per_item, dim3(256), 0, s, ws);
        hipLaunchKernelGGL(ctag::k_track_lin<false>, per_item128, dim3(128), 0, s, ws, T, P, 1);
        hipLaunchKernelGGL(ctag::k_track_decide, per_piece, dim3(64), 0, s, ws, P, 1, piece_rig);
    }
    if (!mark(2)) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_track_lin<true>, per_item128, dim3(128), 0, s, ws, T, P, 0);
    hipLaunchKernelGGL(ctag::k_track_seg_factor, per_seg, dim3(64), 0, s, ws, L, 1, seg_rig);
    hipLaunchKernelGGL(ctag::k_track_sep, per_piece, dim3(64), 0, s, ws, L, 1, piece_rig);
    hipLaunchKernelGGL(ctag::k_track_seg_back, per_seg, dim3(64), 0, s, ws, L, 1, seg_rig);
    hipLaunchKernelGGL(ctag::k_track_write, per_item, dim3(256), 0, s, ws, out_dev);
    hipLaunchKernelGGL(ctag::k_track_stat, dim3((n_rigs + 63) / 64), dim3(64), 0, s, ws, stat_dev);
    if (hipGetLastError() != hipSuccess || !mark(3)) return CTAG_ERR_HIP;
    if (hipEventRecord(st->done, s) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = true;
    return CTAG_OK;
}

template <class Rec>
int track_host(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
               const ctag_track_opts* opts, ctag_track_rec* out, ctag_track_stat* stat) {
    if (!h || !rigs || !recs || !cov || n_frames < 1 || !out || !stat) return CTAG_ERR_ARG;
    const long long n_items = (long long)n_frames * rigs->n_rigs;
    if (rigs->n_rigs < 1 || n_items > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    TrackState* st = track_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const size_t n = (size_t)n_items;  // every earlier host form has waited for its own work: the buffers are free
    if (st->d_in.grow(sizeof(Rec) * n) != hipSuccess || st->d_cov.grow(n) != hipSuccess || st->d_out.grow(n) != hipSuccess ||
        st->d_stat.grow((size_t)rigs->n_rigs) != hipSuccess)
        return CTAG_ERR_HIP;
    if (hipMemcpyAsync(st->d_in.p, recs, sizeof(Rec) * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(st->d_cov.p, cov, sizeof(ctag_pose_cov_rec) * n, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    const int rc = track_device<Rec>(h, rigs, reinterpret_cast<const Rec*>(st->d_in.p), st->d_cov.p, n_frames, times, opts, st->d_out.p, st->d_stat.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_track_rec) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(stat, st->d_stat.p, sizeof(ctag_track_stat) * (size_t)rigs->n_rigs, hipMemcpyDeviceToHost, s) != hipSuccess)
        return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_track_opts_default(ctag_track_opts* o) {
    if (!o) return;
    o->struct_size = (uint32_t)sizeof(ctag_track_opts);
    o->loss = CTAG_TRACK_LOSS_NONE;
    o->max_iterations = 10;
    o->max_gap = 5;
    o->segment_frames = 0;
    o->reserved = 0;
    o->dt = 1.0 / 30.0;
    o->q_rot = 0.1;       // tools/track_study.py, DESIGN.md section 21: a hand-held rig, a model in millimetres
    o->q_trans = 3000.0;
    o->vel0_sigma_rot = 10.0;
    o->vel0_sigma_trans = 1000.0;
    o->loss_scale = 4.0;
    o->lambda0 = 1e-3;
}

int ctag_rig_track_smooth_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                 int n_frames, const double* times, const ctag_track_opts* opts, ctag_track_rec* out_dev, ctag_track_stat* stat_dev) {
    return track_device<ctag_rig_pose_rec>(h, rigs, rig_poses_dev, cov_dev, n_frames, times, opts, out_dev, stat_dev);
}

int ctag_mv_rig_track_smooth_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                    int n_frames, const double* times, const ctag_track_opts* opts, ctag_track_rec* out_dev, ctag_track_stat* stat_dev) {
    return track_device<ctag_mv_pose_rec>(h, rigs, mv_poses_dev, cov_dev, n_frames, times, opts, out_dev, stat_dev);
}

int ctag_rig_track_smooth(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                          const double* times, const ctag_track_opts* opts, ctag_track_rec* out, ctag_track_stat* stat) {
    return track_host<ctag_rig_pose_rec>(h, rigs, rig_poses, cov, n_frames, times, opts, out, stat);
}

int ctag_mv_rig_track_smooth(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                             const double* times, const ctag_track_opts* opts, ctag_track_rec* out, ctag_track_stat* stat) {
    return track_host<ctag_mv_pose_rec>(h, rigs, mv_poses, cov, n_frames, times, opts, out, stat);
}

int ctag_track_last_ms(ctag_handle* h, float* out4) {
    if (!h || !out4) return CTAG_ERR_ARG;
    TrackState* st = track_state(h);
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
