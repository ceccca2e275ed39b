// k_model_fit.hip -- reconstruction of the marker models themselves (the 3-D corner lists every pose call takes) from the
// detection records of many frames and a rough seed model, on the device.  The semantics are stated in include/ctag_pose.h
// (model reconstruction, rules 1-8).
//
// Mapping.  The reprojection problem over corners and per-record poses separates: given the model a
// record's pose is the solve k_pose already does, so a round is
//   pose      ctag_pose_batch_device on the call's working copy of the model (k_pose.hip, untouched);
//   record    k_mfit_record: one wavefront per observation record, grid-stride, lane = point.  The walk, corner_point and the
//             residual are k_pose_cov's; the 21 entries of U = sum Jp^T Jp and the 6 of sum Jp^T r go through wave_sum_f64, every
//             lane factors U = L L^T and writes, per point, Z = L^-1 (Jp^T Jx) (6x3), Jx^T Jx (6) and Jx^T r - Z^T y (3): 27 doubles,
//             plus the record's corner -> local index table (int16, -1 where the corner is absent);
//   assemble  k_mfit_assemble: for model m one thread per corner pair a <= b with its 3x3 block of S in registers; it walks the
//             records in record order (other models' records skipped by a block-uniform branch), subtracts Za^T Zb and adds
//             Jxa^T Jxa on the diagonal; g the same way, one thread per corner.  The running sums live in global memory between
//             passes of the record workspace, so the result does not depend on the pass size;
//   solve     k_mfit_solve: one block per model, the damped system (S + lambda diag S) in global memory (1.8 MB at 160 corners:
//             it stays in L2), right-looking column Cholesky with the current column in LDS, held corners as identity rows with a
//             zero right-hand side, the two triangular solves, delta and a flag for a pivot that is not positive.
// The host decides (accept / reject, lambda, stop, gauge, metric scale) per model between the launches.  FP64 VALU like the pose
// kernels; the largest system is 480 x 480, nothing here is MFMA-shaped enough to pay for a second arithmetic.
//
// What this fit shares with the rig assembly (k_rig_fit.hip) is not here: the pose block of a record (pass 1 of the record kernel, a
// column through L^-1, the point Jacobian) is ctag_schur6.h's, the point descriptor and load_state6 are ctag_pose_dev.h's, and the
// host side of a fit -- timed state, call context, working model, systems with their pass loop and solve, the accept / reject rule
// -- is ctag_fit_host.h's.  This file keeps its kernels' own walk, tables and pass 2, find_held, gauge_to_seed,
// metric_scale, the probe, and its round loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_fit_host.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"
#include "ctag_schur6.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_model_fit_stat) == 56, "ctag_model_fit_stat layout");
static_assert(sizeof(ctag_model_fit_opts) == 40, "ctag_model_fit_opts layout");

namespace ctag {

constexpr int kMfitGrid = 256;           // wavefronts of one k_mfit_record launch at most
constexpr int kMfitPassRecords = 2048;   // observation records one pass of the workspace holds
constexpr int kMfitDoubles = 27;         // per point of a record: Z (18), Jx^T Jx (6), Jx^T r - Z^T y (3)
constexpr int kMfitMaxN = 3 * kPoseMaxPts;  // 480 unknowns per model at most
constexpr int kMfitSolveThreads = 1024;
// flags of a record: kRecLeftOut (it is not an observation: rule 1; set on its first visit, never changes) and kRecSingular

struct MfitLds {
    int32_t src[kPoseMaxPts];    // point i: its descriptor (point_desc, ctag_pose_dev.h; camera 0)
    int16_t table[kPoseMaxPts];  // model corner -> local point index, -1 where absent
};

// corner k (0 .. 7) of a feature that an emit's lane q stands for: 0 1 4 5 2 3 6 7
__device__ __forceinline__ int mfit_corner_of(int q) { return q < 2 ? q : q < 4 ? q + 2 : q < 6 ? q - 2 : q; }

// Observation records r0 .. r1-1 (indices into ok_list, which holds pose-record indices): workspace slot r - r0 gets the 27
// doubles of every point, table row r the corner -> local index map, flags[r] the record's state.
__global__ __launch_bounds__(64) void k_mfit_record(const ctag_frame_result* __restrict__ res, int n_frames, const ctag_pose_rec* __restrict__ poses,
                                                    const int32_t* __restrict__ ok_list, int r0, int r1, PoseModelDev model, PoseCam cam,
                                                    double* __restrict__ ws, int16_t* __restrict__ table, int32_t* __restrict__ flags) {
    __shared__ MfitLds L;
    const int lane = threadIdx.x;
    const int pm = model.model_size * 8;  // <= kPoseMaxPts (checked by the host)
    for (int r = r0 + (int)blockIdx.x; r < r1; r += gridDim.x) {
        const ctag_pose_rec& P = poses[ok_list[r]];
        wave_sync();  // the previous record's LDS reads are done
        for (int c = lane; c < pm; c += 64) L.table[c] = -1;
        wave_sync();
        int n = 0;
        bool ok = P.status == CTAG_POSE_OK && P.frame >= 0 && P.frame < n_frames && P.model_index >= 0 && P.model_index < model.n_models;
        if (ok) {
            const ctag_frame_result& FR = res[P.frame];
            ok = FR.status == CTAG_OK && P.marker >= 0 && P.marker < min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
            if (ok) {
                const ctag_feature_rec* F0 = FR.features;
                const int st = marker_points(FR, FR.markers[P.marker], model.model_size, kPoseMaxPts, n, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
                    if (lane < cnt) {
                        L.src[i0 + lane] = point_desc((int)(&F - F0), lane, 0, pos);
                        L.table[pos * 8 + mfit_corner_of(lane)] = (int16_t)(i0 + lane);
                    }
                });
                ok = st == CTAG_POSE_OK && n == P.n_points && n >= 4;
            }
        }
        wave_sync();
        if (ok) {  // two features at one model position: the later one owns the table entry, the earlier one finds it out here
            int dup = 0;
            for (int i = lane; i < n; i += 64) {
                const int s = L.src[i];
                dup += L.table[desc_pos(s) * 8 + mfit_corner_of(desc_q(s))] != i ? 1 : 0;
            }
            ok = sg_sum<64>(dup) == 0;
        }
        double x[6];
        ok = load_state6(P, x) && ok;
        int16_t* T = table + (size_t)r * pm;
        if (!ok) {  // wave-uniform
            for (int c = lane; c < pm; c += 64) T[c] = -1;
            if (lane == 0) flags[r] = kRecLeftOut;
            continue;
        }
        for (int c = lane; c < pm; c += 64) T[c] = L.table[c];
        const ctag_frame_result& FR = res[P.frame];
        const float* __restrict__ corners = model.corners + (size_t)P.model_index * pm * 3;
        double R[9], dR[27];
        ctl::angle_axis_rot(x, R, dR);
        // ---- pass 1: U and sum Jp^T r over the record's points, lane l owning points l, l + 64, l + 128
        double H[21], b[6];
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) b[a] = 0.0;
        for (int i = lane; i < n; i += 64) {
            const int s = L.src[i];
            double xn, yn, ob[2], X[3], q0, q1, j0[6], j1[6];
            corner_point(cam, corners, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, X);
            point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, X, ob, q0, q1, j0, j1, true);
            gram6_add(j0, j1, H);
            grad6_add(j0, j1, q0, q1, b);
        }
        double Lc[36];
        const bool pd = pose_block6(H, b, Lc);  // the same in every lane; b is y from here on
        if (lane == 0) flags[r] = pd ? 0 : kRecSingular;
        if (!pd) continue;
        // ---- pass 2: the 27 doubles of every point
        double* W = ws + (size_t)(r - r0) * pm * kMfitDoubles;
        for (int i = lane; i < n; i += 64) {
            const int s = L.src[i];
            double xn, yn, ob[2], X[3], q0, q1, j0[6], j1[6];
            corner_point(cam, corners, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, X);
            point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, X, ob, q0, q1, j0, j1, true);
            double x0[3], x1[3];
            point_dX(R, j0, j1, x0, x1);
            double* O = W + (size_t)i * kMfitDoubles;
            double gi[3];
#pragma unroll
            for (int m = 0; m < 3; m++) {
                double z[6];
#pragma unroll
                for (int a = 0; a < 6; a++) z[a] = j0[a] * x0[m] + j1[a] * x1[m];
                const double zy = forward6_dot(Lc, z, b);
#pragma unroll
                for (int a = 0; a < 6; a++) O[a * 3 + m] = z[a];
                gi[m] = (x0[m] * q0 + x1[m] * q1) - zy;
            }
            O[18] = x0[0] * x0[0] + x1[0] * x1[0];
            O[19] = x0[0] * x0[1] + x1[0] * x1[1];
            O[20] = x0[0] * x0[2] + x1[0] * x1[2];
            O[21] = x0[1] * x0[1] + x1[1] * x1[1];
            O[22] = x0[1] * x0[2] + x1[1] * x1[2];
            O[23] = x0[2] * x0[2] + x1[2] * x1[2];
            O[24] = gi[0];
            O[25] = gi[1];
            O[26] = gi[2];
        }
    }
}

// Adds records r0 .. r1-1 to S and g of model blockIdx.y.  Thread t < pairs: the corner pair (a <= b) number t in row order;
// pairs <= t < pairs + pm: corner t - pairs of g.  S: [n_models][3 pm][3 pm] row-major, both triangles; g: [n_models][3 pm].
__global__ __launch_bounds__(256) void k_mfit_assemble(const double* __restrict__ ws, const int16_t* __restrict__ table, const int32_t* __restrict__ rec_model,
                                                       const int32_t* __restrict__ flags, int r0, int r1, int pm, double* __restrict__ S, double* __restrict__ g) {
    const int m = blockIdx.y;
    const int pairs = pm * (pm + 1) / 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int N = 3 * pm;
    const bool is_pair = t < pairs, is_g = t >= pairs && t < pairs + pm;
    int a = 0, b = 0;
    if (is_pair) {  // row a starts at a * pm - a (a - 1) / 2
        a = (int)(((double)(2 * pm + 1) - ctm::sqrt64((double)(2 * pm + 1) * (double)(2 * pm + 1) - 8.0 * (double)t)) * 0.5);
        a = min(max(a, 0), pm - 1);
        while (a > 0 && a * pm - a * (a - 1) / 2 > t) a--;
        while (a + 1 < pm && (a + 1) * pm - (a + 1) * a / 2 <= t) a++;
        b = a + (t - (a * pm - a * (a - 1) / 2));
    } else if (is_g) {
        a = b = t - pairs;
    }
    double acc[9];
    double* Sm = S + (size_t)m * N * N;
    double* gm = g + (size_t)m * N;
    if (is_pair) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = 0; q < 3; q++) acc[p * 3 + q] = Sm[(size_t)(3 * a + p) * N + 3 * b + q];
    } else if (is_g) {
#pragma unroll
        for (int p = 0; p < 3; p++) acc[p] = gm[3 * a + p];
    }
    for (int r = r0; r < r1; r++) {
        if (rec_model[r] != m || flags[r] != 0) continue;  // the same for the whole block
        if (!is_pair && !is_g) continue;
        const int la = table[(size_t)r * pm + a], lb = table[(size_t)r * pm + b];
        if (la < 0 || lb < 0) continue;
        const double* za = ws + ((size_t)(r - r0) * pm + la) * kMfitDoubles;
        if (is_g) {
#pragma unroll
            for (int p = 0; p < 3; p++) acc[p] += za[24 + p];
            continue;
        }
        const double* zb = ws + ((size_t)(r - r0) * pm + lb) * kMfitDoubles;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) s += za[k * 3 + p] * zb[k * 3 + q];
                acc[p * 3 + q] -= s;
            }
        if (a == b) {
            acc[0] += za[18];
            acc[1] += za[19];
            acc[2] += za[20];
            acc[3] += za[19];
            acc[4] += za[21];
            acc[5] += za[22];
            acc[6] += za[20];
            acc[7] += za[22];
            acc[8] += za[23];
        }
    }
    if (is_pair) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = 0; q < 3; q++) {
                Sm[(size_t)(3 * a + p) * N + 3 * b + q] = acc[p * 3 + q];
                if (a != b) Sm[(size_t)(3 * b + q) * N + 3 * a + p] = acc[p * 3 + q];
            }
    } else if (is_g) {
#pragma unroll
        for (int p = 0; p < 3; p++) gm[3 * a + p] = acc[p];
    }
}

// (S + lambda diag S) delta = -g of model blockIdx.x by Cholesky, held corners as identity rows with a zero right-hand side.
// A: [n_models][N][N] scratch (its lower triangle is used).  bad[m] = 1 and delta = 0 for a pivot that is not positive.
__global__ __launch_bounds__(kMfitSolveThreads) void k_mfit_solve(const double* __restrict__ S, const double* __restrict__ g, const uint8_t* __restrict__ held,
                                                                  const double* __restrict__ lambda, const int32_t* __restrict__ active, int pm,
                                                                  double* __restrict__ A, double* __restrict__ delta, int32_t* __restrict__ bad) {
    __shared__ double rhs[kMfitMaxN], z[kMfitMaxN], diag[kMfitMaxN], col[kMfitMaxN];
    const int m = blockIdx.x, tid = threadIdx.x, N = 3 * pm;
    if (!active[m]) return;  // block-uniform
    const double* Sm = S + (size_t)m * N * N;
    double* Am = A + (size_t)m * N * N;
    const uint8_t* hm = held + (size_t)m * pm;
    const double lam = lambda[m];
    for (int e = tid; e < N * N; e += kMfitSolveThreads) {
        const int i = e / N, k = e - i * N;
        if (k > i) continue;
        double v;
        if (hm[i / 3] || hm[k / 3]) v = i == k ? 1.0 : 0.0;
        else {
            v = Sm[e];
            if (i == k) v += lam * v;
        }
        Am[e] = v;
    }
    for (int i = tid; i < N; i += kMfitSolveThreads) rhs[i] = hm[i / 3] ? 0.0 : -g[(size_t)m * N + i];
    __syncthreads();
    bool ok = true;
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int kWaves = kMfitSolveThreads / 64;
    for (int j = 0; j < N; j++) {
        const double d = Am[(size_t)j * N + j];  // written before the last barrier; not written again
        if (!(d > 0.0) || !ctl::finite64(d)) {   // the same in every thread
            ok = false;
            break;
        }
        const double sd = ctm::sqrt64(d);
        if (tid == 0) diag[j] = sd;
        for (int i = j + 1 + tid; i < N; i += kMfitSolveThreads) {
            const double v = Am[(size_t)i * N + j] / sd;
            Am[(size_t)i * N + j] = v;
            col[i] = v;
        }
        __syncthreads();
        for (int i = j + 1 + wave; i < N; i += kWaves) {  // row i of the trailing block, lanes along the row
            const double lij = col[i];
            double* row = Am + (size_t)i * N;
            for (int k = j + 1 + lane; k <= i; k += 64) row[k] -= lij * col[k];
        }
        __syncthreads();
    }
    if (!ok) {
        for (int i = tid; i < N; i += kMfitSolveThreads) delta[(size_t)m * N + i] = 0.0;
        if (tid == 0) bad[m] = 1;
        return;
    }
    for (int j = 0; j < N; j++) {  // L z = rhs, column by column
        const double zj = rhs[j] / diag[j];
        if (tid == 0) z[j] = zj;
        for (int i = j + 1 + tid; i < N; i += kMfitSolveThreads) rhs[i] -= Am[(size_t)i * N + j] * zj;
        __syncthreads();
    }
    for (int j = N - 1; j >= 0; j--) {  // L^T delta = z, row j of L is column j of L^T
        const double dj = z[j] / diag[j];
        if (tid == 0) rhs[j] = dj;
        for (int k = tid; k < j; k += kMfitSolveThreads) z[k] -= Am[(size_t)j * N + k] * dj;
        __syncthreads();
    }
    for (int i = tid; i < N; i += kMfitSolveThreads) delta[(size_t)m * N + i] = hm[i / 3] ? 0.0 : rhs[i];
    if (tid == 0) bad[m] = 0;
}

}  // namespace ctag

// =====================================================================================================
// host side: the parts a fit shares with the rig assembly are ctag_fit_host.h's (namespace ctag::fit)
// =====================================================================================================
namespace {

namespace fit = ctag::fit;

// The device side of one call: the models' systems (a group is a model), the record workspace, and which corners do not move.
struct FitWork : fit::Systems {
    fit::Call c;
    int pm = 0;
    std::vector<int16_t> table;  // [R][pm]
    std::vector<uint8_t> held;   // [n_models][pm]
    ctag::DevBuf<int16_t> d_table;
    ctag::DevBuf<double> d_ws, d_A;
    ctag::DevBuf<uint8_t> d_held;

    int setup(int n_models, int pm_, int pass_records) {
        pm = pm_;
        const size_t nn = (size_t)n_models * 9 * pm * pm;
        if (nn * 16 > ((size_t)6 << 30)) return CTAG_ERR_LIMIT;
        const int rc = Systems::setup(c, n_models, 3 * pm, pass_records, ctag::kMfitPassRecords);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_table.grow((size_t)R * pm));
        FIT_HIP(d_ws.grow((size_t)pass * pm * ctag::kMfitDoubles));
        FIT_HIP(d_A.grow(nn));
        FIT_HIP(d_held.grow((size_t)n_models * pm));
        table.assign((size_t)R * pm, -1);
        return CTAG_OK;
    }

    // S and g of every model at (corners_dev, poses_dev); slot 1 times the record kernel, slot 2 the assemble kernel.  Waits.
    int build_system(const float* corners_dev, const int32_t* ids_dev, const ctag_pose_rec* poses_dev, bool fetch_table) {
        const ctag::PoseModelDev md{n_groups, pm / 8, ids_dev, corners_dev};
        const int pairs = pm * (pm + 1) / 2;
        const int rc = build(c, [&](int r0, int r1) {
            if (c.mark(0) != CTAG_OK) return CTAG_ERR_HIP;
            hipLaunchKernelGGL(ctag::k_mfit_record, dim3(std::min(r1 - r0, ctag::kMfitGrid)), dim3(64), 0, c.s, c.res, c.n_frames, poses_dev, d_obs.p, r0, r1, md, c.cam,
                               d_ws.p, d_table.p, d_flags.p);
            if (c.mark(1) != CTAG_OK) return CTAG_ERR_HIP;
            hipLaunchKernelGGL(ctag::k_mfit_assemble, dim3((pairs + pm + 255) / 256, n_groups), dim3(256), 0, c.s, d_ws.p, d_table.p, d_rec_group.p, d_flags.p, r0,
                               r1, pm, d_S.p, d_g.p);
            if (fit::launched() != CTAG_OK || c.mark(2) != CTAG_OK || c.reached(2) != CTAG_OK) return CTAG_ERR_HIP;
            c.add_ms(1, 0);
            c.add_ms(2, 1);
            return CTAG_OK;
        });
        if (rc != CTAG_OK || !fetch_table) return rc;
        FIT_HIP(hipMemcpyAsync(table.data(), d_table.p, sizeof(int16_t) * (size_t)R * pm, hipMemcpyDeviceToHost, c.s));
        FIT_HIP(hipStreamSynchronize(c.s));
        return CTAG_OK;
    }

    // held[m][c] = corner c of model m is seen by fewer than min_obs observation records
    void find_held(int min_obs, std::vector<int>& n_records, std::vector<int>& n_fitted) {
        std::vector<int> count((size_t)n_groups * pm, 0);
        n_records.assign(n_groups, 0);
        n_fitted.assign(n_groups, 0);
        for (int r = 0; r < R; r++) {
            if (flags[r] & ctag::kRecLeftOut) continue;
            const int m = rec_group[r];
            n_records[m]++;
            for (int c = 0; c < pm; c++) count[(size_t)m * pm + c] += table[(size_t)r * pm + c] >= 0 ? 1 : 0;
        }
        held.assign((size_t)n_groups * pm, 1);
        for (int m = 0; m < n_groups; m++)
            for (int c = 0; c < pm; c++)
                if (count[(size_t)m * pm + c] >= min_obs) {
                    held[(size_t)m * pm + c] = 0;
                    n_fitted[m]++;
                }
    }

    int upload_held() { return hipMemcpyAsync(d_held.p, held.data(), held.size(), hipMemcpyHostToDevice, c.s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP; }

    // a model with a singular record is bad; a left-out record is no observation and says nothing
    int solve(const std::vector<double>& lambda, const std::vector<int32_t>& active, std::vector<double>& delta, std::vector<int32_t>& bad) {
        return Systems::solve(c, lambda, active, ctag::kRecSingular, delta, bad, [&]() {
            hipLaunchKernelGGL(ctag::k_mfit_solve, dim3(n_groups), dim3(ctag::kMfitSolveThreads), 0, c.s, d_S.p, d_g.p, d_held.p, d_lambda.p, d_active.p, pm, d_A.p,
                               d_delta.p, d_bad.p);
        });
    }
};

// Rule 5: the similarity (Umeyama) that best carries the fitted corners X onto the seed's Y, applied to X in place.  X, Y: n x 3.
void gauge_to_seed(std::vector<double>& X, const std::vector<double>& Y) {
    const int n = (int)X.size() / 3;
    if (n < 3) return;
    double mx[3] = {0, 0, 0}, my[3] = {0, 0, 0};
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            mx[k] += X[3 * i + k];
            my[k] += Y[3 * i + k];
        }
    for (int k = 0; k < 3; k++) {
        mx[k] /= n;
        my[k] /= n;
    }
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, vx = 0.0;  // C = sum (y - my)(x - mx)^T
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const double xa = X[3 * i + a] - mx[a];
            vx += xa * xa;
            for (int b = 0; b < 3; b++) C[b * 3 + a] += (Y[3 * i + b] - my[b]) * xa;
        }
    if (!(vx > 0.0)) return;
    double sv[3], Rm[9];
    const double sg = fit::nearest_rotation(C, Rm, sv);
    const double scale = (sv[0] + sv[1] + sg * sv[2]) / vx;
    if (!std::isfinite(scale) || !(scale > 0.0)) return;
    for (int i = 0; i < n; i++) {
        const double p[3] = {X[3 * i] - mx[0], X[3 * i + 1] - mx[1], X[3 * i + 2] - mx[2]};
        for (int a = 0; a < 3; a++) X[3 * i + a] = scale * (Rm[a * 3] * p[0] + Rm[a * 3 + 1] * p[1] + Rm[a * 3 + 2] * p[2]) + my[a];
    }
}

// Rule 6: the factor that brings the mean length of the straight vertical edges (0,5) and (1,4) of the features whose four ends
// were fitted to strip_height, and the centroid of the fitted corners; false when there is no such edge.
bool metric_scale(const float* corners, const uint8_t* held, int pm, double strip_height, double& factor, double* centroid) {
    double sum = 0.0;
    int edges = 0;
    for (int f = 0; f < pm / 8; f++) {
        const int c0 = f * 8;
        if (held[c0] || held[c0 + 1] || held[c0 + 4] || held[c0 + 5]) continue;
        for (int e = 0; e < 2; e++) {
            const float* p = corners + (size_t)(c0 + e) * 3;
            const float* q = corners + (size_t)(c0 + (e == 0 ? 5 : 4)) * 3;
            const double d0 = (double)p[0] - q[0], d1 = (double)p[1] - q[1], d2 = (double)p[2] - q[2];
            sum += std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            edges++;
        }
    }
    if (!edges || !(sum > 0.0)) return false;
    factor = strip_height / (sum / edges);
    int n = 0;
    centroid[0] = centroid[1] = centroid[2] = 0.0;
    for (int c = 0; c < pm; c++)
        if (!held[c]) {
            for (int k = 0; k < 3; k++) centroid[k] += (double)corners[(size_t)c * 3 + k];
            n++;
        }
    for (int k = 0; k < 3; k++) centroid[k] /= n;
    return std::isfinite(factor) && factor > 0.0;
}

int fit_opts(const ctag_model_fit_opts* o, ctag_model_fit_opts& r) {
    ctag_model_fit_opts_default(&r);
    if (o) r = *o;
    if (r.max_rounds < 0 || r.min_obs < 1 || !fit::lm_opts_ok(r)) return CTAG_ERR_ARG;
    if (!std::isfinite(r.strip_height)) return CTAG_ERR_ARG;
    return CTAG_OK;
}

}  // namespace

namespace ctag {

int mfit_record_grid() { return kMfitGrid; }
int mfit_pass_records() { return kMfitPassRecords; }

// The reduced system of one model, for the probe of libctag_testkit.so (include/ctag_testkit.h: ctag_testkit_model_fit_system).
int mfit_probe_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_pose_rec* poses, int n_poses, const ctag_model* model_c,
                      const ctag_camera* camera, int model_index, double lambda, int min_obs, int pass_records, double* S, double* g, double* delta,
                      int32_t* held, int32_t* bad_pivot) {
    if (!h || !results || n_frames < 1 || !poses || n_poses < 1 || !model_c || !S || !g || !delta || !held || !bad_pivot || min_obs < 1) return CTAG_ERR_ARG;
    if (model_index < 0 || model_index >= model_c->n_models || model_c->model_size > CTAG_MAX_CODE_POS || !std::isfinite(lambda)) return CTAG_ERR_ARG;
    if (!camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    FitWork w;
    int rc = w.c.prepare(h, kFitState, nullptr, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    if (model_to_device(model, handle_device(h)) != CTAG_OK) return CTAG_ERR_HIP;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<ctag_pose_rec> d_poses;
    rc = fit::upload_probe_inputs(w.c, results, d_res, poses, (size_t)n_poses, d_poses);
    if (rc != CTAG_OK) return rc;
    for (int i = 0; i < n_poses; i++)
        if (poses[i].status == CTAG_POSE_OK && poses[i].model_index >= 0 && poses[i].model_index < model->n_models) {
            w.obs.push_back(i);
            w.rec_group.push_back(poses[i].model_index);
        }
    const int pm = model->model_size * 8, N = 3 * pm;
    if (w.obs.empty()) return CTAG_ERR_ARG;
    rc = w.setup(model->n_models, pm, pass_records);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(model->d_corners.p, model->d_ids.p, d_poses.p, true);
    if (rc != CTAG_OK) return rc;
    std::vector<int> n_records, n_fitted;
    w.find_held(min_obs, n_records, n_fitted);
    rc = w.upload_held();
    if (rc != CTAG_OK) return rc;
    std::vector<double> lam(model->n_models, lambda), d;
    std::vector<int32_t> active(model->n_models, 0), bad;
    active[model_index] = 1;
    rc = w.solve(lam, active, d, bad);
    if (rc != CTAG_OK) return rc;
    FIT_HIP(hipMemcpy(S, w.d_S.p + (size_t)model_index * N * N, sizeof(double) * (size_t)N * N, hipMemcpyDeviceToHost));
    FIT_HIP(hipMemcpy(g, w.d_g.p + (size_t)model_index * N, sizeof(double) * N, hipMemcpyDeviceToHost));
    std::memcpy(delta, d.data() + (size_t)model_index * N, sizeof(double) * N);
    for (int c = 0; c < pm; c++) held[c] = w.held[(size_t)model_index * pm + c];
    *bad_pivot = bad[model_index];
    return CTAG_OK;
}

}  // namespace ctag

extern "C" {

void ctag_model_fit_opts_default(ctag_model_fit_opts* o) {
    if (!o) return;
    o->max_rounds = 30;
    o->min_obs = 2;
    o->lambda0 = 1e-3;
    o->lambda_max = 1e6;
    o->rel_tol = 2.416e-7;  // 4 x 6.04e-8: what float32 rounding of the model alone does to the cost
    o->strip_height = 0.0;
}

int ctag_model_fit_last_ms(ctag_handle* h, float* out4) { return fit::last_ms(h, ctag::kFitState, out4); }  // pose, record, assemble, solve

int ctag_model_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* seed, const ctag_camera* camera,
                          const ctag_model_fit_opts* opts_in, ctag_model** out, ctag_model_fit_stat* stats) {
    if (!h || !results_dev || n_frames < 1 || !seed || !camera || !out || !stats) return CTAG_ERR_ARG;
    ctag_model_fit_opts opts;
    if (fit_opts(opts_in, opts) != CTAG_OK) return CTAG_ERR_ARG;
    if (seed->model_size != ctag::handle_dict_cols(h) || seed->model_size > CTAG_MAX_CODE_POS) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    if ((long long)n_frames * CTAG_MAX_MARKERS > (1ll << 30)) return CTAG_ERR_LIMIT;
    FitWork w;
    int rc = w.c.prepare(h, ctag::kFitState, results_dev, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    fit::ModelGuard guard;
    rc = fit::clone_model(seed, &guard.m);
    if (rc != CTAG_OK) return rc;
    ctag_model* W = guard.m;
    const int nm = W->n_models, pm = W->model_size * 8, N = 3 * pm;
    for (int m = 0; m < nm; m++) {
        std::memset(&stats[m], 0, sizeof(stats[m]));
        stats[m].status = CTAG_POSE_NOT_SEEN;
        stats[m].n_points_held = pm;
        stats[m].lambda = opts.lambda0;
    }
    auto hand_out = [&]() {
        *out = guard.m;
        guard.m = nullptr;
        return CTAG_OK;
    };
    if (nm == 0) return hand_out();

    // ---- rule 1: the observation records are the CTAG_POSE_OK records under the seed
    ctag::DevBuf<int32_t> d_off;
    ctag::DevBuf<ctag_pose_rec> d_poses;
    std::vector<int32_t> off;
    rc = fit::count_pose_records(w.c, W, camera, d_off, d_poses, off);
    if (rc != CTAG_OK) return rc;
    const int32_t total = off[n_frames];
    if (total <= 0) return hand_out();
    std::vector<ctag_pose_rec> acc, trial;
    // pose records of W (its device corners are current) to the host, timed in slot 0
    auto pose_pass = [&](std::vector<ctag_pose_rec>& host) {
        return w.c.pose_pass(0, [&]() { return ctag_pose_batch_device(h, results_dev, n_frames, W, camera, d_off.p, d_poses.p, total); }, d_poses.p, (size_t)total, host);
    };
    rc = pose_pass(acc);
    if (rc != CTAG_OK) return rc;
    for (int i = 0; i < total; i++)
        if (acc[i].status == CTAG_POSE_OK) {
            w.obs.push_back(i);
            w.rec_group.push_back(acc[i].model_index);
        }
    if (w.obs.empty()) return hand_out();
    rc = w.setup(nm, pm, 0);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(W->d_corners.p, W->d_ids.p, d_poses.p, true);
    if (rc != CTAG_OK) return rc;
    const int R = w.R;
    std::vector<uint8_t> left_out(R);
    for (int r = 0; r < R; r++) left_out[r] = (w.flags[r] & ctag::kRecLeftOut) ? 1 : 0;

    // ---- rule 2
    std::vector<int> n_records, n_fitted;
    w.find_held(opts.min_obs, n_records, n_fitted);
    rc = w.upload_held();
    if (rc != CTAG_OK) return rc;

    fit::Lm lm;
    lm.start(nm, opts.lambda0);
    std::vector<uint8_t> ok_cur;
    w.costs_of(acc, &left_out, lm.cost, ok_cur);
    std::vector<long long> n_points(nm, 0);
    for (int r = 0; r < R; r++)
        if (!left_out[r]) n_points[w.rec_group[r]] += acc[w.obs[r]].n_points;
    for (int m = 0; m < nm; m++) {
        stats[m].n_records = n_records[m];
        stats[m].n_points_fitted = n_fitted[m];
        stats[m].n_points_held = pm - n_fitted[m];
        stats[m].cost0 = stats[m].cost = lm.cost[m];
        if (n_records[m] > 0 && n_fitted[m] > 0) {
            stats[m].status = CTAG_POSE_OK;
            lm.active[m] = opts.max_rounds > 0 ? 1 : 0;
        }
    }

    // ---- rules 3-5: the rounds.  `accepted` is the accepted state of every model; W carries the trial during a round.  The loop is
    // the rig assembly's (k_rig_fit.hip, rule 5) but for the steps marked "model"; the two are kept in step by hand
    std::vector<float> accepted = W->corners;
    const std::vector<float>& seed_corners = seed->corners;
    bool need_system = false;  // the system of the first round is the one built above
    std::vector<double> X, Y, delta, cost_trial(nm, 0.0);
    std::vector<uint8_t> ok_trial(nm, 0);
    std::vector<int32_t> bad;
    while (lm.any_active()) {
        if (need_system) {
            W->corners = accepted;
            if (fit::push_corners(w.c, W) != CTAG_OK) return CTAG_ERR_HIP;
            FIT_HIP(hipMemcpyAsync(d_poses.p, acc.data(), sizeof(ctag_pose_rec) * (size_t)total, hipMemcpyHostToDevice, w.c.s));
            rc = w.build_system(W->d_corners.p, W->d_ids.p, d_poses.p, false);
            if (rc != CTAG_OK) return rc;
            need_system = false;
        }
        rc = w.solve(lm.lambda, lm.active, delta, bad);
        if (rc != CTAG_OK) return rc;
        W->corners = accepted;
        bool any_trial = false;
        for (int m = 0; m < nm; m++) {  // model: the step on the corners that move, then rule 5
            if (!lm.active[m] || bad[m]) continue;
            X.clear();
            Y.clear();
            for (int c = 0; c < pm; c++) {
                if (w.held[(size_t)m * pm + c]) continue;
                for (int k = 0; k < 3; k++) {
                    X.push_back((double)accepted[((size_t)m * pm + c) * 3 + k] + delta[(size_t)m * N + 3 * c + k]);
                    Y.push_back((double)seed_corners[((size_t)m * pm + c) * 3 + k]);
                }
            }
            gauge_to_seed(X, Y);
            size_t i = 0;
            bool finite = true;
            for (double v : X) finite = finite && std::isfinite(v);
            if (!finite) {
                bad[m] = 1;
                continue;
            }
            for (int c = 0; c < pm; c++) {
                if (w.held[(size_t)m * pm + c]) continue;
                for (int k = 0; k < 3; k++) W->corners[((size_t)m * pm + c) * 3 + k] = (float)X[i++];
            }
            any_trial = true;
        }
        if (any_trial) {
            if (fit::push_corners(w.c, W) != CTAG_OK) return CTAG_ERR_HIP;
            rc = pose_pass(trial);
            if (rc != CTAG_OK) return rc;
            w.costs_of(trial, &left_out, cost_trial, ok_trial);
        }
        for (int m = 0; m < nm; m++) {
            if (!lm.active[m]) continue;
            // an active model that is not bad has made a trial, so `any_trial &&` (the rig loop's guard) changes no decision here
            if (!lm.decide(m, any_trial && !bad[m] && ok_trial[m], cost_trial[m], opts)) continue;
            std::memcpy(&accepted[(size_t)m * pm * 3], &W->corners[(size_t)m * pm * 3], sizeof(float) * (size_t)pm * 3);  // model
            w.take_records(m, trial, acc);
            need_system = true;
        }
    }

    // ---- rule 6
    W->corners = accepted;
    bool scaled = false;
    if (opts.strip_height > 0.0)
        for (int m = 0; m < nm; m++) {
            if (stats[m].status != CTAG_POSE_OK) continue;
            double f = 1.0, c0[3];
            if (!metric_scale(&W->corners[(size_t)m * pm * 3], &w.held[(size_t)m * pm], pm, opts.strip_height, f, c0)) continue;
            for (int c = 0; c < pm; c++) {
                if (w.held[(size_t)m * pm + c]) continue;
                for (int k = 0; k < 3; k++) {
                    float& v = W->corners[((size_t)m * pm + c) * 3 + k];
                    v = (float)(c0[k] + f * ((double)v - c0[k]));
                }
            }
            for (int k = 0; k < 3; k++) W->base[3 * m + k] = (float)(c0[k] + f * ((double)W->base[3 * m + k] - c0[k]));
            scaled = true;
        }
    if (scaled) {
        if (fit::push_corners(w.c, W) != CTAG_OK) return CTAG_ERR_HIP;
        rc = pose_pass(trial);
        if (rc != CTAG_OK) return rc;
        w.costs_of(trial, &left_out, lm.cost, ok_cur);
    }
    for (int m = 0; m < nm; m++) {
        if (stats[m].status != CTAG_POSE_OK) continue;
        stats[m].rounds = lm.rounds[m];
        stats[m].cost = lm.cost[m];
        stats[m].lambda = lm.lambda[m];
        stats[m].rms_px = n_points[m] > 0 ? std::sqrt(2.0 * lm.cost[m] / (double)n_points[m]) : 0.0;
    }
    fit::release_device_copies(W);
    return hand_out();
}

int ctag_model_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* seed, const ctag_camera* camera,
                   const ctag_model_fit_opts* opts, ctag_model** out, ctag_model_fit_stat* stats) {
    if (!h || !results || n_frames < 1 || !seed || !camera || !out || !stats) return CTAG_ERR_ARG;
    return fit::with_results_on_device(h, results, n_frames, [&](const ctag_frame_result* results_dev) {
        return ctag_model_fit_device(h, results_dev, n_frames, seed, camera, opts, out, stats);
    });
}

// CylinderTag.cpp:168-188 read backwards: "model_num model_size", then per model its id, base, axis and model_size * 8 lines
// "corner_id x y z"
int ctag_model_save(const ctag_model* m, const char* path) {
    if (!m || !path) return CTAG_ERR_ARG;
    FILE* f = std::fopen(path, "w");
    if (!f) return CTAG_ERR_ARG;
    bool ok = std::fprintf(f, "%d %d\n", m->n_models, m->model_size) > 0;
    for (int i = 0; i < m->n_models && ok; i++) {
        ok = std::fprintf(f, "%d\n%.9g %.9g %.9g\n%.9g %.9g %.9g\n", m->ids[i], (double)m->base[3 * i], (double)m->base[3 * i + 1], (double)m->base[3 * i + 2],
                          (double)m->axis[3 * i], (double)m->axis[3 * i + 1], (double)m->axis[3 * i + 2]) > 0;
        for (int c = 0; c < m->model_size * 8 && ok; c++) {
            const float* p = &m->corners[((size_t)i * m->model_size * 8 + c) * 3];
            ok = std::fprintf(f, "%d %.9g %.9g %.9g\n", c, (double)p[0], (double)p[1], (double)p[2]) > 0;
        }
    }
    ok = std::fclose(f) == 0 && ok;
    return ok ? CTAG_OK : CTAG_ERR_ARG;
}

}  // extern "C"
