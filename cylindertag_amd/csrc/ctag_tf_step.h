// ctag_tf_step.h -- the track filter's walk, stated once for the two kernels that run it: k_track_filter (k_track_filter.hip), which
// keeps the state between calls and writes a record a frame, and k_track_noise (k_track_noise.hip), which runs it from an EMPTY track
// for many candidate noise levels and keeps four sums.  Rule numbers are those of include/ctag_pose.h, track filtering.
//   tf_bad_input   rule 1's bad input over a whole call (lane = frame)
//   tf_prepass     rule 1 for 64 frames side by side into LDS: Rm, tm and cov_scale * cov_f, the measured mask by a ballot
//   tf_step        rules 2-5 for one frame, wave-uniform: the pose, the velocities, the clock and the two counters in registers, P in LDS under ctag_m12.h's
//                  convention.  It hands back what rule 4 produced (TfOut) and, with LOGDET, log det S from the same factorisation.
// A block is one wave: the phases are ordered by lds_wait(), not by a block barrier.  Everything is FP64 VALU.  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ctag_pose.h"
#include "ctag_linalg.h"
#include "ctag_loss.h"
#include "ctag_m12.h"
#include "ctag_so3.h"
#include "ctag_wave.h"

namespace ctag {

constexpr double kTfMinPivot = 1e-12;

struct TfP {
    int loss, max_gap;
    double q_rot, q_trans, vr2, vt2, a, a2, gate2;
    double cov_scale;  // every cov_f is read as cov_scale * cov_f (1 unless ctag_track_filter_set_cov_scale or a noise candidate says otherwise)
};

// CTAG_TF_CLOCKS=1 (a measurement build, tools/track_filter_clocks.py): the wave reads the 100 MHz clock at the phase boundaries of the walk and
// block 0 prints the sums when it ends.  The product is built without it.
#ifndef CTAG_TF_CLOCKS
#define CTAG_TF_CLOCKS 0
#endif
#if CTAG_TF_CLOCKS
struct TfClk {
    long long c[6] = {0, 0, 0, 0, 0, 0}, last = 0;  // pre-pass, predict, innovation, gain, Joseph form, record
};
#define TF_CLK(clk, k)                         \
    do {                                       \
        const long long now_ = wall_clock64(); \
        (clk).c[k] += now_ - (clk).last;       \
        (clk).last = now_;                     \
    } while (0)
#else
struct TfClk {};
#define TF_CLK(clk, k) \
    do {               \
    } while (0)
#endif

struct TfLds {
    double meas[48 * 64];  // [k][lane]: Rm 9, tm 3, cov_scale * cov_f 36 (mirrored from its upper triangle) of the chunk's frames
    M12 P, T, F;
    double K[72], M[72], KC[72], G[36], J[9], delta[12], rec[16];
};

// what one frame produced
struct TfOut {
    int status;
    uint32_t flags;
    double m2, wt;
    double logdet;  // log det S of rule 4 (LOGDET only), valid when `updated`
    bool full;      // the record carries a state
    bool updated;   // rule 4 updated the state at this frame
};

// inv = A^-1 for a symmetric 6x6 A, scaled to unit diagonal and factored with pivots above kTfMinPivot (rule 4).  With LOGDET,
// logdet = sum_a log A_aa + 2 sum_j log L_jj, L the Cholesky factor of the unit-diagonal matrix.
template <bool LOGDET = false>
__device__ __forceinline__ bool sym6_inverse(const double* A, double* inv, double* logdet = nullptr) {
    double d[6], Cm[36], ci[36], Ld[6], mp = 0.0;
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
    if (!ctl::chol6_inverse_factor_diag(Cm, ci, nullptr, kTfMinPivot, mp, LOGDET ? Ld : nullptr)) return false;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) inv[a * 6 + b] = d[a] * ci[a * 6 + b] * d[b];
    if (LOGDET) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) s1 += ctm::log64(A[a * 6 + a]);
#pragma unroll
        for (int a = 0; a < 6; a++) s2 += ctm::log64(Ld[a]);
        *logdet = s1 + 2.0 * s2;
    }
    return true;
}

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

// rule 1's bad input for rig g over the n_frames of a call: the same answer in every lane
template <class Rec>
__device__ __forceinline__ bool tf_bad_input(const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov, int n_frames, int n_rigs, int g, int lane) {
    bool bad = false;
    for (int f = lane; f < n_frames; f += 64) {
        const size_t w = (size_t)f * n_rigs + g;
        bad = bad || misplaced_or_rvec(recs[w], cov[w], f, g);
    }
    return __builtin_amdgcn_ballot_w64(bad) != 0ull;
}

// (a) lane = frame for frames f0 .. f0 + 63 of rig g: rule 1, the measured frames' Rm, tm and cov_scale * cov_f into S.meas; returns the measured mask
template <class Rec>
__device__ __forceinline__ unsigned long long tf_prepass(TfLds& S, const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov, int f0, int n_frames,
                                                         int n_rigs, int g, double cov_scale, bool active, int lane) {
    const int fl = f0 + lane;
    bool m = false;
    if (active && fl < n_frames) {
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
                for (int b = 0; b < 6; b++) S.meas[(12 + a * 6 + b) * 64 + lane] = cov_scale * cov[wi].cov[min(a, b) * 6 + max(a, b)];
        }
    }
    const unsigned long long Mmask = __builtin_amdgcn_ballot_w64(m);
    lds_wait();
    return Mmask;
}

// (b) rules 2-5 for the frame at slot kk of the chunk in S.meas, at time tf.  R, t, w, v, tprev, tracking, misses: the part of the track that lives
// in registers (separate arrays: as one struct the filter kernel keeps it in scratch).  `meas`: the frame is measured.  predict_only: rule 7 (the
// state's clock and its count of unmeasured frames stay).
template <bool LOGDET>
__device__ __forceinline__ void tf_step(TfLds& S, double* R, double* t, double* w, double* v, double& tprev, int& tracking, int& misses, const TfP& p, bool meas, int kk, double tf, bool predict_only, int lane, TfClk& clk, TfOut& o) {
    o.status = CTAG_TRACK_OK;
    o.flags = meas ? CTAG_TRACK_FLAG_MEASURED : 0u;
    o.m2 = 0.0;
    o.wt = 1.0;
    o.logdet = 0.0;
    o.full = true;
    o.updated = false;
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
            o.status = CTAG_TRACK_NOT_TRACKED;
            o.full = false;
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
            o.flags |= CTAG_TRACK_FLAG_STARTED;
        }
        return;
    }
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
    TF_CLK(clk, 1);
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
        bool ok = sym6_inverse<LOGDET>(Sm, Si, &o.logdet);
        if (ok) {
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double s = 0.0;
#pragma unroll
                for (int b = 0; b < 6; b++) s += Si[a * 6 + b] * e6[b];
                o.m2 += e6[a] * s;
            }
            ok = ctl::finite64(o.m2);
        }
        if (!ok) {
            singular = true;
        } else if (p.gate2 > 0.0 && o.m2 > p.gate2) {
            o.flags |= CTAG_TRACK_FLAG_GATED;
            o.wt = 0.0;
            o.m2 = 0.0;
        } else {
            if (p.loss != CTAG_TRACK_LOSS_NONE) {
                double rho;
                robust_loss(p.loss, p.a, p.a2, o.m2, rho, om);
            }
            if (om < 1.0) {
#pragma unroll
                for (int k = 0; k < 36; k++) Sm[k] = HPH[k] + cv[k] / om;
                singular = !sym6_inverse(Sm, Si);
            }
            update = !singular;
        }
    }
    TF_CLK(clk, 2);
    if (singular) {
        o.status = CTAG_TRACK_SINGULAR;
        o.full = false;
        tracking = 0;
        o.m2 = 0.0;
    } else if (update) {
        o.updated = true;
        o.wt = om;
        if (om < 1.0) o.flags |= CTAG_TRACK_FLAG_DOWNWEIGHTED;
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
        TF_CLK(clk, 3);
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
        TF_CLK(clk, 4);
    } else {
        // ---- rule 5: the prediction is the state ----
        const bool drop = !predict_only && misses + 1 >= p.max_gap;
        if (drop) {
            o.status = CTAG_TRACK_NOT_TRACKED;
            o.full = false;
            tracking = 0;
            o.wt = (o.flags & CTAG_TRACK_FLAG_GATED) ? 0.0 : 1.0;
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

}  // namespace ctag
