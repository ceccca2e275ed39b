// k_track_filter.hip -- the causal counterpart of k_track.hip: per rig an extended Kalman filter on (R, t, w, v) under the smoother's
// constant-velocity model, whose state stays in device memory between calls.  The semantics are stated in include/ctag_pose.h (track
// filtering, rules 1-10).
//
// Mapping.  One launch a call, one wavefront a rig.  The frames of the call are taken 64 at a time:
//   (a) lane = frame: rule 1 for 64 frames side by side (angle_axis_rot and the covariance's validity factorisation), Rm, tm and cov_f
//       into LDS (48 doubles a frame), the measured mask by a ballot; bad input is found by a scan over the whole call before that;
//   (b) the wave walks the 64 frames in order.  The pose, the velocities and every 3x3 / 6x6 quantity (E, Jl, phi, Jl^-1, S and its
//       factorisation) are wave-uniform: every lane computes the same value in registers.  The 12x12 P and the blocks derived from it
//       live in LDS under ctag_m12.h's convention: entry e belongs to lane e % 64, one order of summation, symmetric results computed
//       at (min, max).  F is 3x3-block sparse (six terms a row, not twelve), I - K H differs from I in six columns, S is 6x6;
//   (c) a record's 58 doubles are written by 58 lanes.
// A block is one wave: the phases are ordered by lds_wait(), not by a block barrier.  Everything is FP64 VALU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_linalg.h"
#include "ctag_loss.h"
#include "ctag_m12.h"
#include "ctag_so3.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_track_rec) == 464, "ctag_track_rec layout");
static_assert(sizeof(ctag_track_filter_opts) == 72, "ctag_track_filter_opts layout");

namespace ctag {

constexpr int kTfStateDoubles = 164;  // P 144, R 9, t 3, w 3, v 3, t_prev, one spare
constexpr int kTfStateInts = 2;       // tracking, consecutive frames without an update
constexpr int kTfRecWords = 58;       // a ctag_track_rec in 8-byte words
constexpr double kTfMinPivot = 1e-12;

struct TfP {
    int loss, max_gap;
    double q_rot, q_trans, vr2, vt2, a, a2, gate2;
};

// CTAG_TF_CLOCKS=1 (a measurement build, tools/track_filter_clocks.py): the wave reads the 100 MHz clock at the phase boundaries of the walk and
// block 0 prints the sums when it ends.  The product is built without it.
#ifndef CTAG_TF_CLOCKS
#define CTAG_TF_CLOCKS 0
#endif
#if CTAG_TF_CLOCKS
#define TF_CLK(k)                            \
    do {                                     \
        const long long now_ = wall_clock64(); \
        clk[k] += now_ - clk_last;           \
        clk_last = now_;                     \
    } while (0)
#else
#define TF_CLK(k) \
    do {          \
    } while (0)
#endif

struct TfLds {
    double meas[48 * 64];  // [k][lane]: Rm 9, tm 3, cov_f 36 (mirrored from its upper triangle) of the chunk's frames
    M12 P, T, F;
    double K[72], M[72], KC[72], G[36], J[9], delta[12], rec[16];
};

// inv = A^-1 for a symmetric 6x6 A, scaled to unit diagonal and factored with pivots above kTfMinPivot (rule 4)
__device__ __forceinline__ bool sym6_inverse(const double* A, double* inv) {
    double d[6], Cm[36], ci[36], mp = 0.0;
    bool good = true;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double h = A[a * 6 + a];
        good = good && ctl::finite64(h) && h > 0.0;
        d[a] = 1.0 / ctm::sqrt64(h);
    }
    if (!good) return false;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) Cm[a * 6 + b] = d[a] * A[a * 6 + b] * d[b];
    if (!ctl::chol6_inverse_factor(Cm, ci, nullptr, kTfMinPivot, mp)) return false;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) inv[a * 6 + b] = d[a] * ci[a * 6 + b] * d[b];
    return true;
}

__device__ __forceinline__ double words_as_double(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }

// rule 3 on P: S.P <- F P F^T + Q for the step D with E = Exp(D w) and DJ = D Jl(D w)
__device__ __forceinline__ void tf_predict_cov(TfLds& S, const double* E, const double* DJ, double D, const TfP& p, int lane) {
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                S.F.v[r * 12 + c] = E[r * 3 + c];
                S.F.v[r * 12 + 6 + c] = DJ[r * 3 + c];
            }
#pragma unroll
        for (int r = 0; r < 3; r++) S.F.v[(3 + r) * 12 + 9 + r] = D;
    }
    lds_wait();
    for (int e = lane; e < 144; e += 64) {  // T = F P: row i of F has its diagonal block and, for theta and t, the block two to the right
        const int i = e / 12, j = e % 12, c0 = 3 * (i / 3);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += S.F.v[i * 12 + c0 + k] * S.P.v[(c0 + k) * 12 + j];
        if (i < 6) {
#pragma unroll
            for (int k = 0; k < 3; k++) s += S.F.v[i * 12 + c0 + 6 + k] * S.P.v[(c0 + 6 + k) * 12 + j];
        }
        S.T.v[e] = s;
    }
    lds_wait();
    const double D2 = D * D;
    for (int e = lane; e < 144; e += 64) {  // P- = T F^T + Q at (a <= b)
        const int i = e / 12, j = e % 12, a = min(i, j), b = max(i, j), c0 = 3 * (b / 3);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += S.T.v[a * 12 + c0 + k] * S.F.v[b * 12 + c0 + k];
        if (b < 6) {
#pragma unroll
            for (int k = 0; k < 3; k++) s += S.T.v[a * 12 + c0 + 6 + k] * S.F.v[b * 12 + c0 + 6 + k];
        }
        const double q = (a % 6) < 3 ? p.q_rot : p.q_trans;
        double Q = 0.0;
        if (a == b) Q = a < 6 ? q * (D2 * D) / 3.0 : q * D;
        else if (b == a + 6) Q = q * D2 / 2.0;
        S.P.v[e] = s + Q;
    }
    lds_wait();
}

// one record: words 0-13 and 56, 57 from S.rec (lane 0 wrote them), the covariance and the velocity sigmas from S.P when `full`
__device__ __forceinline__ void tf_write_rec(TfLds& S, double* __restrict__ out, bool full, int lane) {
    lds_wait();
    if (lane < kTfRecWords) {
        double val;
        if (lane < 14) {
            val = S.rec[lane];
        } else if (lane < 50) {
            const int r = (lane - 14) / 6, c = (lane - 14) % 6;
            val = full ? S.P.v[min(r, c) * 12 + max(r, c)] : 0.0;
        } else if (lane < 56) {
            const int d = lane - 44;
            val = full ? ctm::sqrt64(S.P.v[d * 12 + d]) : 0.0;
        } else {
            val = S.rec[lane - 42];
        }
        out[lane] = val;
    }
    lds_wait();
}

// predict_only: rule 7 -- one unmeasured frame at t0 for every rig, nothing stored
template <class Rec>
__global__ __launch_bounds__(64) void k_track_filter(const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov, int n_frames, int n_rigs,
                                                     const double* __restrict__ times, double t0, TfP p, double* __restrict__ state,
                                                     int32_t* __restrict__ istate, ctag_track_rec* __restrict__ out_recs, int predict_only) {
    __shared__ TfLds S;
    const int g = blockIdx.x, lane = threadIdx.x;
    double* __restrict__ out = reinterpret_cast<double*>(out_recs);
    // ---- rule 1's bad input, over the whole call ----
    if (!predict_only) {
        bool bad = false;
        for (int f = lane; f < n_frames; f += 64) {
            const size_t w = (size_t)f * n_rigs + g;
            bad = bad || misplaced_or_rvec(recs[w], cov[w], f, g);
        }
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {
            for (long long idx = lane; idx < (long long)n_frames * kTfRecWords; idx += 64) {
                const int f = (int)(idx / kTfRecWords), wd = (int)(idx % kTfRecWords);
                const double val = wd == 0 ? words_as_double((uint32_t)CTAG_TRACK_BAD_INPUT, (uint32_t)g) : (wd == 1 ? words_as_double((uint32_t)f, 0u) : 0.0);
                out[((size_t)f * n_rigs + g) * kTfRecWords + wd] = val;
            }
            return;
        }
    }
    // ---- the state: P into LDS, the rest wave-uniform ----
    double* __restrict__ st = state + (size_t)g * kTfStateDoubles;
    m_load(S.P, st, lane);
    m_identity(S.F, lane);
    double R[9], t[3], w[3], v[3], tprev;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = st[144 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = st[153 + k], w[k] = st[156 + k], v[k] = st[159 + k];
    tprev = st[162];
    int tracking = istate[g * kTfStateInts], misses = istate[g * kTfStateInts + 1];
    lds_wait();

#if CTAG_TF_CLOCKS
    long long clk[6] = {0, 0, 0, 0, 0, 0}, clk_last = wall_clock64();  // pre-pass, predict, innovation, gain, Joseph form, record
#endif
    for (int f0 = 0; f0 < n_frames; f0 += 64) {  // wave-uniform
        // ---- (a) lane = frame ----
        const int fl = f0 + lane;
        bool m = false;
        if (!predict_only && fl < n_frames) {
            const size_t wi = (size_t)fl * n_rigs + g;
            double Rm[9], tm[3], W[36];
            m = measured_sample(recs[wi], cov[wi], kTfMinPivot, Rm, tm, W);
            if (m) {
#pragma unroll
                for (int k = 0; k < 9; k++) S.meas[k * 64 + lane] = Rm[k];
#pragma unroll
                for (int k = 0; k < 3; k++) S.meas[(9 + k) * 64 + lane] = tm[k];
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b < 6; b++) S.meas[(12 + a * 6 + b) * 64 + lane] = cov[wi].cov[min(a, b) * 6 + max(a, b)];
            }
        }
        const unsigned long long Mmask = __builtin_amdgcn_ballot_w64(m);
        lds_wait();
        const int cnt = min(64, n_frames - f0);
        TF_CLK(0);
        // ---- (b) the walk ----
        for (int kk = 0; kk < cnt; kk++) {  // wave-uniform
            const int f = f0 + kk;
            const double tf = times ? times[f] : t0;
            const bool meas = ((Mmask >> kk) & 1ull) != 0ull;
            int status = CTAG_TRACK_OK;
            uint32_t flags = meas ? CTAG_TRACK_FLAG_MEASURED : 0u;
            double m2 = 0.0, wt = 1.0;
            bool full = true;  // the record carries a state
            double Rm[9], tm[3], cv[36];
            if (meas) {
#pragma unroll
                for (int k = 0; k < 9; k++) Rm[k] = S.meas[k * 64 + kk];
#pragma unroll
                for (int k = 0; k < 3; k++) tm[k] = S.meas[(9 + k) * 64 + kk];
#pragma unroll
                for (int k = 0; k < 36; k++) cv[k] = S.meas[(12 + k) * 64 + kk];
            }
            if (!tracking) {
                if (!meas) {  // rule 2
                    status = CTAG_TRACK_NOT_TRACKED;
                    full = false;
                } else {      // rule 2: the track starts
#pragma unroll
                    for (int k = 0; k < 9; k++) R[k] = Rm[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) t[k] = tm[k], w[k] = 0.0, v[k] = 0.0;
                    for (int e = lane; e < 144; e += 64) {
                        const int i = e / 12, j = e % 12;
                        double val = 0.0;
                        if (i < 6 && j < 6) val = S.meas[(12 + i * 6 + j) * 64 + kk];
                        else if (i == j) val = i < 9 ? p.vr2 : p.vt2;
                        S.P.v[e] = val;
                    }
                    tracking = 1;
                    misses = 0;
                    tprev = tf;
                    flags |= CTAG_TRACK_FLAG_STARTED;
                }
            } else {
                // ---- rule 3 ----
                const double D = tf - tprev;
                double dw[3], E[9], DJ[9], Rp[9], tp[3];
#pragma unroll
                for (int k = 0; k < 3; k++) dw[k] = D * w[k];
                ctl::angle_axis_rot(dw, E, nullptr);
                so3_jl(dw, DJ);
#pragma unroll
                for (int k = 0; k < 9; k++) DJ[k] = D * DJ[k];
                mat3_mul(E, R, Rp);
#pragma unroll
                for (int k = 0; k < 3; k++) tp[k] = t[k] + D * v[k];
                tf_predict_cov(S, E, DJ, D, p, lane);
                TF_CLK(1);
                bool update = false, singular = false;
                double e6[6], J[9], Si[36], om = 1.0;
                if (meas) {
                    // ---- rule 4 ----
                    double Rel[9], Pp[36], A1[9], HPH[36], Sm[36];
                    mat3_mul_nt(Rp, Rm, Rel);
                    so3_log(Rel, e6);
                    so3_jlinv(e6, J);
#pragma unroll
                    for (int k = 0; k < 3; k++) e6[3 + k] = tp[k] - tm[k];
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int b = a; b < 6; b++) Pp[a * 6 + b] = Pp[b * 6 + a] = S.P.v[a * 12 + b];
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = 0; c < 3; c++) A1[r * 3 + c] = J[r * 3] * Pp[c] + J[r * 3 + 1] * Pp[6 + c] + J[r * 3 + 2] * Pp[12 + c];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int c = r; c < 3; c++)
                            HPH[r * 6 + c] = HPH[c * 6 + r] = A1[r * 3] * J[c * 3] + A1[r * 3 + 1] * J[c * 3 + 1] + A1[r * 3 + 2] * J[c * 3 + 2];
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            HPH[r * 6 + 3 + c] = HPH[(3 + c) * 6 + r] = J[r * 3] * Pp[3 + c] + J[r * 3 + 1] * Pp[6 + 3 + c] + J[r * 3 + 2] * Pp[12 + 3 + c];
                            HPH[(3 + r) * 6 + 3 + c] = Pp[(3 + r) * 6 + 3 + c];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 36; k++) Sm[k] = HPH[k] + cv[k];
                    bool ok = sym6_inverse(Sm, Si);
                    if (ok) {
                        for (int a = 0; a < 6; a++) {
                            double s = 0.0;
                            for (int b = 0; b < 6; b++) s += Si[a * 6 + b] * e6[b];
                            m2 += e6[a] * s;
                        }
                        ok = ctl::finite64(m2);
                    }
                    if (!ok) {
                        singular = true;
                    } else if (p.gate2 > 0.0 && m2 > p.gate2) {
                        flags |= CTAG_TRACK_FLAG_GATED;
                        wt = 0.0;
                        m2 = 0.0;
                    } else {
                        if (p.loss != CTAG_TRACK_LOSS_NONE) {
                            double rho;
                            robust_loss(p.loss, p.a, p.a2, m2, rho, om);
                        }
                        if (om < 1.0) {
#pragma unroll
                            for (int k = 0; k < 36; k++) Sm[k] = HPH[k] + cv[k] / om;
                            singular = !sym6_inverse(Sm, Si);
                        }
                        update = !singular;
                    }
                }
                TF_CLK(2);
                if (singular) {
                    status = CTAG_TRACK_SINGULAR;
                    full = false;
                    tracking = 0;
                    m2 = 0.0;
                } else if (update) {
                    wt = om;
                    if (om < 1.0) flags |= CTAG_TRACK_FLAG_DOWNWEIGHTED;
                    if (lane == 0) {  // G = Hs^T Si, Hs = blockdiag(Jl^-1, I)
#pragma unroll
                        for (int r = 0; r < 6; r++)
#pragma unroll
                            for (int c = 0; c < 6; c++)
                                S.G[r * 6 + c] = r < 3 ? J[r] * Si[c] + J[3 + r] * Si[6 + c] + J[6 + r] * Si[12 + c] : Si[r * 6 + c];
#pragma unroll
                        for (int k = 0; k < 9; k++) S.J[k] = J[k];
                    }
                    lds_wait();
                    for (int e = lane; e < 72; e += 64) {  // K = P-[:, 0:6] G
                        const int i = e / 6, c = e % 6;
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; k++) s += S.P.v[i * 12 + k] * S.G[k * 6 + c];
                        S.K[e] = s;
                    }
                    lds_wait();
                    for (int e = lane; e < 72; e += 64) {  // M = K Hs, KC = K C with C = cov_f / omega
                        const int i = e / 6, c = e % 6;
                        double s = S.K[e];
                        if (c < 3) s = S.K[i * 6] * S.J[c] + S.K[i * 6 + 1] * S.J[3 + c] + S.K[i * 6 + 2] * S.J[6 + c];
                        S.M[e] = s;
                        double s2 = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; k++) s2 += S.K[i * 6 + k] * (S.meas[(12 + k * 6 + c) * 64 + kk] / om);
                        S.KC[e] = s2;
                    }
                    if (lane < 12) {
                        double s = 0.0;
#pragma unroll
                        for (int c = 0; c < 6; c++) s += S.K[lane * 6 + c] * e6[c];
                        S.delta[lane] = -s;
                    }
                    lds_wait();
                    TF_CLK(3);
                    for (int e = lane; e < 144; e += 64) {  // T = (I - K H) P- = P- - M P-[0:6, :]
                        const int i = e / 12, j = e % 12;
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; k++) s += S.M[i * 6 + k] * S.P.v[k * 12 + j];
                        S.T.v[e] = S.P.v[e] - s;
                    }
                    lds_wait();
                    for (int e = lane; e < 144; e += 64) {  // P = T (I - K H)^T + K C K^T at (a <= b)
                        const int i = e / 12, j = e % 12, a = min(i, j), b = max(i, j);
                        double s1 = 0.0, s2 = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; k++) s1 += S.T.v[a * 12 + k] * S.M[b * 6 + k];
#pragma unroll
                        for (int k = 0; k < 6; k++) s2 += S.KC[a * 6 + k] * S.K[b * 6 + k];
                        S.P.v[e] = (S.T.v[a * 12 + b] - s1) + s2;
                    }
                    double dl[12], E2[9];
#pragma unroll
                    for (int k = 0; k < 12; k++) dl[k] = S.delta[k];
                    ctl::angle_axis_rot(dl, E2, nullptr);
                    mat3_mul(E2, Rp, R);
#pragma unroll
                    for (int k = 0; k < 3; k++) t[k] = tp[k] + dl[3 + k], w[k] = w[k] + dl[6 + k], v[k] = v[k] + dl[9 + k];
                    if (!predict_only) tprev = tf, misses = 0;
                    TF_CLK(4);
                } else {
                    // ---- rule 5: the prediction is the state ----
                    const bool drop = !predict_only && misses + 1 >= p.max_gap;
                    if (drop) {
                        status = CTAG_TRACK_NOT_TRACKED;
                        full = false;
                        tracking = 0;
                        wt = (flags & CTAG_TRACK_FLAG_GATED) ? 0.0 : 1.0;
                    } else {
#pragma unroll
                        for (int k = 0; k < 9; k++) R[k] = Rp[k];
#pragma unroll
                        for (int k = 0; k < 3; k++) t[k] = tp[k];
                        tprev = tf;
                        misses++;
                    }
                }
            }
            // ---- (c) the record ----
            if (lane == 0) {
                double rv[3] = {0.0, 0.0, 0.0};
                if (full) so3_log(R, rv);
                S.rec[0] = words_as_double((uint32_t)status, (uint32_t)g);
                S.rec[1] = words_as_double((uint32_t)(predict_only ? 0 : f), flags);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    S.rec[2 + k] = rv[k];
                    S.rec[5 + k] = full ? t[k] : 0.0;
                    S.rec[8 + k] = full ? w[k] : 0.0;
                    S.rec[11 + k] = full ? v[k] : 0.0;
                }
                S.rec[14] = full ? m2 : 0.0;
                S.rec[15] = full ? wt : 0.0;
            }
            tf_write_rec(S, out + ((size_t)(predict_only ? 0 : f) * n_rigs + g) * kTfRecWords, full, lane);
            TF_CLK(5);
        }
    }
#if CTAG_TF_CLOCKS
    if (g == 0 && lane == 0)
        printf("tf_clocks frames %d prepass %lld predict %lld innovation %lld gain %lld joseph %lld record %lld\n", n_frames, clk[0], clk[1], clk[2], clk[3],
               clk[4], clk[5]);
#endif
    if (predict_only) return;
    lds_wait();
    m_store(st, S.P, lane);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) st[144 + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) st[153 + k] = t[k], st[156 + k] = w[k], st[159 + k] = v[k];
        st[162] = tprev;
        istate[g * kTfStateInts] = tracking;
        istate[g * kTfStateInts + 1] = misses;
    }
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
struct ctag_track_filter {
    ctag_handle* h = nullptr;
    int n_rigs = 0;
    ctag::TfP P;
    double dt = 0.0;
    ctag::DevBuf<double> d_state, d_times[2];
    ctag::DevBuf<int32_t> d_istate;
    ctag::DevBuf<unsigned char> d_in;  // the host forms' records
    ctag::DevBuf<ctag_pose_cov_rec> d_cov;
    ctag::DevBuf<ctag_track_rec> d_out;
    std::vector<double> times[2];      // the times of the last two multi-frame calls, in turn: the caller's array may go once the call returns
    hipEvent_t done[2] = {nullptr, nullptr}, ev[2] = {nullptr, nullptr};  // done[k]: behind the call that used slot k
    bool in_flight[2] = {false, false}, timed = false, has_last = false;
    int slot = 0;
    float ms = 0.f;
    long long frames_given = 0;
    double last_time = 0.0;
};

namespace {

bool tf_pos_finite(double v) { return std::isfinite(v) && v > 0.0; }

hipStream_t tf_stream(ctag_track_filter* F) { return static_cast<hipStream_t>(ctag_stream(F->h)); }

int tf_clear(ctag_track_filter* F) {
    hipStream_t s = tf_stream(F);
    if (hipMemsetAsync(F->d_state.p, 0, sizeof(double) * (size_t)F->n_rigs * ctag::kTfStateDoubles, s) != hipSuccess ||
        hipMemsetAsync(F->d_istate.p, 0, sizeof(int32_t) * (size_t)F->n_rigs * ctag::kTfStateInts, s) != hipSuccess)
        return CTAG_ERR_HIP;
    F->frames_given = 0;
    F->has_last = false;
    return CTAG_OK;
}

// rule 9 for a step call's sizes and times, on the host and before anything is enqueued
int tf_step_args(const ctag_track_filter* F, int n_frames, const double* times) {
    if (n_frames < 1 || (long long)n_frames * F->n_rigs > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    if (times) {
        for (int f = 0; f < n_frames; f++) {
            if (!std::isfinite(times[f])) return CTAG_ERR_ARG;
            if (f > 0 ? !(times[f] > times[f - 1]) : (F->has_last && !(times[0] > F->last_time))) return CTAG_ERR_ARG;
        }
    } else if (F->has_last && !((double)F->frames_given * F->dt > F->last_time)) {
        return CTAG_ERR_ARG;
    }
    return CTAG_OK;
}

template <class Rec>
int tf_step_device(ctag_track_filter* F, const Rec* recs_dev, const ctag_pose_cov_rec* cov_dev, int n_frames, const double* times, ctag_track_rec* out_dev) {
    if (!F || !recs_dev || !cov_dev || !out_dev) return CTAG_ERR_ARG;
    if (tf_step_args(F, n_frames, times) != CTAG_OK) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = tf_stream(F);
    const double* T = nullptr;
    double t0 = 0.0, t_last;
    if (n_frames == 1) {  // a single time travels as a kernel argument
        t0 = times ? times[0] : (double)F->frames_given * F->dt;
        t_last = t0;
    } else {
        const int k = F->slot;  // two staging slots in turn: only the multi-frame call before the previous one is waited for
        if (F->in_flight[k] && hipEventSynchronize(F->done[k]) != hipSuccess) return CTAG_ERR_HIP;
        F->in_flight[k] = false;
        if (F->d_times[k].grow((size_t)n_frames) != hipSuccess) return CTAG_ERR_HIP;
        std::vector<double>& tt = F->times[k];
        tt.resize(n_frames);
        for (int f = 0; f < n_frames; f++) tt[f] = times ? times[f] : (double)(F->frames_given + f) * F->dt;
        if (hipMemcpyAsync(F->d_times[k].p, tt.data(), sizeof(double) * (size_t)n_frames, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
        T = F->d_times[k].p;
        t_last = tt[n_frames - 1];
    }
    const bool timing = ctag::handle_timing(F->h);
    F->timed = timing;
    if (timing && hipEventRecord(F->ev[0], s) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_track_filter<Rec>, dim3(F->n_rigs), dim3(64), 0, s, recs_dev, cov_dev, n_frames, F->n_rigs, T, t0, F->P, F->d_state.p,
                       F->d_istate.p, out_dev, 0);
    if (hipGetLastError() != hipSuccess) return CTAG_ERR_HIP;
    if (timing && hipEventRecord(F->ev[1], s) != hipSuccess) return CTAG_ERR_HIP;
    if (n_frames > 1) {
        if (hipEventRecord(F->done[F->slot], s) != hipSuccess) return CTAG_ERR_HIP;
        F->in_flight[F->slot] = true;
        F->slot ^= 1;
    }
    F->frames_given += n_frames;
    F->last_time = t_last;
    F->has_last = true;
    return CTAG_OK;
}

template <class Rec>
int tf_step_host(ctag_track_filter* F, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, const double* times, ctag_track_rec* out) {
    if (!F || !recs || !cov || !out) return CTAG_ERR_ARG;
    if (tf_step_args(F, n_frames, times) != CTAG_OK) return CTAG_ERR_ARG;  // a refused call enqueues nothing
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = tf_stream(F);
    const size_t n = (size_t)n_frames * F->n_rigs;  // every earlier host form has waited for its own work: the buffers are free
    if (F->d_in.grow(sizeof(Rec) * n) != hipSuccess || F->d_cov.grow(n) != hipSuccess || F->d_out.grow(n) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpyAsync(F->d_in.p, recs, sizeof(Rec) * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(F->d_cov.p, cov, sizeof(ctag_pose_cov_rec) * n, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    const int rc = tf_step_device<Rec>(F, reinterpret_cast<const Rec*>(F->d_in.p), F->d_cov.p, n_frames, times, F->d_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, F->d_out.p, sizeof(ctag_track_rec) * n, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_track_filter_opts_default(ctag_track_filter_opts* o) {
    if (!o) return;
    ctag_track_opts t;
    ctag_track_opts_default(&t);
    o->struct_size = (uint32_t)sizeof(ctag_track_filter_opts);
    o->loss = CTAG_TRACK_LOSS_NONE;
    o->max_gap = 5;
    o->reserved = 0;
    o->dt = 1.0 / 30.0;
    o->q_rot = t.q_rot;
    o->q_trans = t.q_trans;
    o->vel0_sigma_rot = t.vel0_sigma_rot;
    o->vel0_sigma_trans = t.vel0_sigma_trans;
    o->loss_scale = t.loss_scale;
    o->gate = 0.0;  // off: tools/track_filter_study.py found no gate of 3 .. 8 that spares every good frame at these q
}

int ctag_track_filter_create(ctag_handle* h, const ctag_rigs* rigs, const ctag_track_filter_opts* opts, ctag_track_filter** filter) {
    if (!h || !rigs || !filter) return CTAG_ERR_ARG;
    *filter = nullptr;
    ctag_track_filter_opts d;
    ctag_track_filter_opts_default(&d);
    const ctag_track_filter_opts* o = opts ? opts : &d;
    if (o->struct_size != sizeof(ctag_track_filter_opts)) return CTAG_ERR_ARG;
    if (o->loss != CTAG_LOSS_HUBER && o->loss != CTAG_LOSS_CAUCHY && o->loss != CTAG_TRACK_LOSS_NONE) return CTAG_ERR_ARG;
    if (o->max_gap < 1 || rigs->n_rigs < 1 || rigs->n_rigs > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    for (double v : {o->dt, o->q_rot, o->q_trans, o->vel0_sigma_rot, o->vel0_sigma_trans, o->loss_scale})
        if (!tf_pos_finite(v)) return CTAG_ERR_ARG;
    if (!std::isfinite(o->gate) || o->gate < 0.0) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    ctag_track_filter* F = new (std::nothrow) ctag_track_filter();
    if (!F) return CTAG_ERR_HIP;
    F->h = h;
    F->n_rigs = rigs->n_rigs;
    F->dt = o->dt;
    F->P.loss = o->loss;
    F->P.max_gap = o->max_gap;
    F->P.q_rot = o->q_rot;
    F->P.q_trans = o->q_trans;
    F->P.vr2 = o->vel0_sigma_rot * o->vel0_sigma_rot;
    F->P.vt2 = o->vel0_sigma_trans * o->vel0_sigma_trans;
    F->P.a = o->loss_scale;
    F->P.a2 = o->loss_scale * o->loss_scale;
    F->P.gate2 = o->gate * o->gate;
    bool ok = F->d_state.grow((size_t)F->n_rigs * ctag::kTfStateDoubles) == hipSuccess && F->d_istate.grow((size_t)F->n_rigs * ctag::kTfStateInts) == hipSuccess &&
              F->d_out.grow((size_t)F->n_rigs) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&F->done[0], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&F->done[1], hipEventDisableTiming) == hipSuccess && hipEventCreate(&F->ev[0]) == hipSuccess &&
         hipEventCreate(&F->ev[1]) == hipSuccess && tf_clear(F) == CTAG_OK;
    if (!ok) {
        ctag_track_filter_free(F);
        return CTAG_ERR_HIP;
    }
    *filter = F;
    return CTAG_OK;
}

void ctag_track_filter_free(ctag_track_filter* F) {
    if (!F) return;
    (void)hipSetDevice(ctag::handle_device(F->h));
    (void)hipStreamSynchronize(tf_stream(F));  // nothing may still read the state or the times
    for (auto& e : F->done)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : F->ev)
        if (e) (void)hipEventDestroy(e);
    delete F;
}

int ctag_track_filter_reset(ctag_track_filter* F) {
    if (!F) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    return tf_clear(F);
}

int ctag_rig_track_filter_device(ctag_track_filter* F, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev, int n_frames,
                                 const double* times, ctag_track_rec* out_dev) {
    return tf_step_device<ctag_rig_pose_rec>(F, rig_poses_dev, cov_dev, n_frames, times, out_dev);
}

int ctag_mv_rig_track_filter_device(ctag_track_filter* F, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev, int n_frames,
                                    const double* times, ctag_track_rec* out_dev) {
    return tf_step_device<ctag_mv_pose_rec>(F, mv_poses_dev, cov_dev, n_frames, times, out_dev);
}

int ctag_rig_track_filter(ctag_track_filter* F, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                          ctag_track_rec* out) {
    return tf_step_host<ctag_rig_pose_rec>(F, rig_poses, cov, n_frames, times, out);
}

int ctag_mv_rig_track_filter(ctag_track_filter* F, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                             ctag_track_rec* out) {
    return tf_step_host<ctag_mv_pose_rec>(F, mv_poses, cov, n_frames, times, out);
}

int ctag_track_filter_predict_device(ctag_track_filter* F, double t, ctag_track_rec* out_dev) {
    if (!F || !out_dev || !std::isfinite(t) || (F->has_last && !(t > F->last_time))) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_track_filter<ctag_rig_pose_rec>, dim3(F->n_rigs), dim3(64), 0, tf_stream(F), (const ctag_rig_pose_rec*)nullptr,
                       (const ctag_pose_cov_rec*)nullptr, 1, F->n_rigs, (const double*)nullptr, t, F->P, F->d_state.p, F->d_istate.p, out_dev, 1);
    return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

int ctag_track_filter_predict(ctag_track_filter* F, double t, ctag_track_rec* out) {
    if (!F || !out) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = tf_stream(F);
    if (hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;  // d_out is the host forms' buffer: nothing reads it now
    if (F->d_out.grow((size_t)F->n_rigs) != hipSuccess) return CTAG_ERR_HIP;
    const int rc = ctag_track_filter_predict_device(F, t, F->d_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, F->d_out.p, sizeof(ctag_track_rec) * (size_t)F->n_rigs, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

int ctag_track_filter_last_ms(ctag_track_filter* F, float* out1) {
    if (!F || !out1) return CTAG_ERR_ARG;
    if (F->timed) {
        F->timed = false;
        F->ms = 0.f;
        if (hipEventSynchronize(F->ev[1]) == hipSuccess) (void)hipEventElapsedTime(&F->ms, F->ev[0], F->ev[1]);
    }
    *out1 = F->ms;
    return CTAG_OK;
}

}  // extern "C"
