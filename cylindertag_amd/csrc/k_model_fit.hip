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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
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
constexpr int kMfitLeftOut = 1;          // flags: the record is not an observation (rule 1; set on its first visit, never changes)
constexpr int kMfitSingular = 2;         // flags: U of the record has a pivot that is not positive at this state

struct MfitLds {
    int32_t src[kPoseMaxPts];    // point i: feature index in its frame record | corner q of the emit << 7 | model position << 13
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
                        L.src[i0 + lane] = (int32_t)(&F - F0) | (lane << 7) | (pos << 13);
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
                dup += L.table[(s >> 13) * 8 + mfit_corner_of((s >> 7) & 7)] != i ? 1 : 0;
            }
            ok = sg_sum<64>(dup) == 0;
        }
        double x[6];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            x[i] = P.rvec[i];
            x[3 + i] = P.tvec[i];
            ok = ok && ctl::finite64(x[i]) && ctl::finite64(x[3 + i]);
        }
        int16_t* T = table + (size_t)r * pm;
        if (!ok) {  // wave-uniform
            for (int c = lane; c < pm; c += 64) T[c] = -1;
            if (lane == 0) flags[r] = kMfitLeftOut;
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
            corner_point(cam, corners, FR.features[s & 127], s >> 13, (s >> 7) & 7, xn, yn, ob, X);
            point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, X, ob, q0, q1, j0, j1, true);
            int e = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int c = a; c < 6; c++) {
                    H[e] += j0[a] * j0[c];
                    H[e] += j1[a] * j1[c];
                    e++;
                }
                b[a] += j0[a] * q0;
                b[a] += j1[a] * q1;
            }
        }
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = wave_sum_f64(H[e]);
#pragma unroll
        for (int a = 0; a < 6; a++) b[a] = wave_sum_f64(b[a]);
        double Lc[36];
        const bool pd = mfit_chol6(H, Lc);  // the same in every lane
        if (lane == 0) flags[r] = pd ? 0 : kMfitSingular;
        if (!pd) continue;
        mfit_forward6(Lc, b);  // y
        // ---- pass 2: the 27 doubles of every point
        double* W = ws + (size_t)(r - r0) * pm * kMfitDoubles;
        for (int i = lane; i < n; i += 64) {
            const int s = L.src[i];
            double xn, yn, ob[2], X[3], q0, q1, j0[6], j1[6];
            corner_point(cam, corners, FR.features[s & 127], s >> 13, (s >> 7) & 7, xn, yn, ob, X);
            point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, X, ob, q0, q1, j0, j1, true);
            // d residual / d X = (a0 R0 - b0 R2, a1 R1 - b1 R2) with the a0, b0, a1, b1 of point_residual: j0[3] = a0, j0[5] = -b0, j1[4] = a1, j1[5] = -b1
            double x0[3], x1[3];
#pragma unroll
            for (int m = 0; m < 3; m++) {
                x0[m] = j0[3] * R[m] + j0[5] * R[6 + m];
                x1[m] = j1[4] * R[3 + m] + j1[5] * R[6 + m];
            }
            double* O = W + (size_t)i * kMfitDoubles;
            double gi[3];
#pragma unroll
            for (int m = 0; m < 3; m++) {
                double z[6];
#pragma unroll
                for (int a = 0; a < 6; a++) z[a] = j0[a] * x0[m] + j1[a] * x1[m];
                mfit_forward6(Lc, z);
                double zy = 0.0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    O[a * 3 + m] = z[a];
                    zy += z[a] * b[a];
                }
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
// host side
// =====================================================================================================
namespace {

struct FitState {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms[4] = {0.f, 0.f, 0.f, 0.f};  // pose, record, assemble, solve
};

void fit_state_free(void* p) {
    FitState* s = static_cast<FitState*>(p);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

FitState* fit_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kFitState, fit_state_free);
    if (!*slot) {
        FitState* s = new (std::nothrow) FitState();
        if (!s) return nullptr;
        for (auto& e : s->ev)
            if (hipEventCreate(&e) != hipSuccess) {
                fit_state_free(s);
                return nullptr;
            }
        *slot = s;
    }
    return static_cast<FitState*>(*slot);
}

#define FIT_HIP(call)                              \
    do {                                           \
        if ((call) != hipSuccess) return CTAG_ERR_HIP; \
    } while (0)

// The device side of one call: the observation list, the record workspace and the per-model systems.
struct FitWork {
    ctag_handle* h = nullptr;
    hipStream_t s = nullptr;
    FitState* st = nullptr;
    bool timing = false;
    const ctag_frame_result* res = nullptr;
    int n_frames = 0, n_models = 0, pm = 0, N = 0, R = 0, pass = 0;
    ctag::PoseCam cam{};
    std::vector<int32_t> ok, rec_model, flags;  // [R]
    std::vector<int16_t> table;                 // [R][pm]
    std::vector<uint8_t> held;                  // [n_models][pm]
    ctag::DevBuf<int32_t> d_ok, d_rec_model, d_flags, d_active, d_bad;
    ctag::DevBuf<int16_t> d_table;
    ctag::DevBuf<double> d_ws, d_S, d_g, d_A, d_delta, d_lambda;
    ctag::DevBuf<uint8_t> d_held;

    int setup(int n_models_, int pm_, int pass_records) {
        n_models = n_models_;
        pm = pm_;
        N = 3 * pm;
        R = (int)ok.size();
        pass = std::max(1, std::min(R, pass_records > 0 ? pass_records : ctag::kMfitPassRecords));
        const size_t nn = (size_t)n_models * N * N;
        if (nn * 16 > ((size_t)6 << 30)) return CTAG_ERR_LIMIT;
        FIT_HIP(d_ok.grow(R));
        FIT_HIP(d_rec_model.grow(R));
        FIT_HIP(d_flags.grow(R));
        FIT_HIP(d_table.grow((size_t)R * pm));
        FIT_HIP(d_ws.grow((size_t)pass * pm * ctag::kMfitDoubles));
        FIT_HIP(d_S.grow(nn));
        FIT_HIP(d_A.grow(nn));
        FIT_HIP(d_g.grow((size_t)n_models * N));
        FIT_HIP(d_delta.grow((size_t)n_models * N));
        FIT_HIP(d_lambda.grow(n_models));
        FIT_HIP(d_active.grow(n_models));
        FIT_HIP(d_bad.grow(n_models));
        FIT_HIP(d_held.grow((size_t)n_models * pm));
        FIT_HIP(hipMemcpyAsync(d_ok.p, ok.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, s));
        FIT_HIP(hipMemcpyAsync(d_rec_model.p, rec_model.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, s));
        flags.assign(R, 0);
        table.assign((size_t)R * pm, -1);
        return CTAG_OK;
    }

    // S and g of every model at (corners_dev, poses_dev), pass by pass; flags come back to the host.  Waits.
    int build_system(const float* corners_dev, const int32_t* ids_dev, const ctag_pose_rec* poses_dev, bool fetch_table) {
        const ctag::PoseModelDev md{n_models, pm / 8, ids_dev, corners_dev};
        FIT_HIP(hipMemsetAsync(d_S.p, 0, sizeof(double) * (size_t)n_models * N * N, s));
        FIT_HIP(hipMemsetAsync(d_g.p, 0, sizeof(double) * (size_t)n_models * N, s));
        const int pairs = pm * (pm + 1) / 2;
        for (int r0 = 0; r0 < R; r0 += pass) {
            const int r1 = std::min(R, r0 + pass);
            if (timing) FIT_HIP(hipEventRecord(st->ev[0], s));
            hipLaunchKernelGGL(ctag::k_mfit_record, dim3(std::min(r1 - r0, ctag::kMfitGrid)), dim3(64), 0, s, res, n_frames, poses_dev, d_ok.p, r0, r1, md, cam,
                               d_ws.p, d_table.p, d_flags.p);
            if (timing) FIT_HIP(hipEventRecord(st->ev[1], s));
            hipLaunchKernelGGL(ctag::k_mfit_assemble, dim3((pairs + pm + 255) / 256, n_models), dim3(256), 0, s, d_ws.p, d_table.p, d_rec_model.p, d_flags.p, r0,
                               r1, pm, d_S.p, d_g.p);
            FIT_HIP(hipGetLastError());
            if (timing) {
                FIT_HIP(hipEventRecord(st->ev[2], s));
                FIT_HIP(hipEventSynchronize(st->ev[2]));
                float a = 0.f, b = 0.f;
                (void)hipEventElapsedTime(&a, st->ev[0], st->ev[1]);
                (void)hipEventElapsedTime(&b, st->ev[1], st->ev[2]);
                st->ms[1] += a;
                st->ms[2] += b;
            }
        }
        FIT_HIP(hipMemcpyAsync(flags.data(), d_flags.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, s));
        if (fetch_table) FIT_HIP(hipMemcpyAsync(table.data(), d_table.p, sizeof(int16_t) * (size_t)R * pm, hipMemcpyDeviceToHost, s));
        FIT_HIP(hipStreamSynchronize(s));
        return CTAG_OK;
    }

    // held[m][c] = corner c of model m is seen by fewer than min_obs observation records
    void find_held(int min_obs, std::vector<int>& n_records, std::vector<int>& n_fitted) {
        std::vector<int> count((size_t)n_models * pm, 0);
        n_records.assign(n_models, 0);
        n_fitted.assign(n_models, 0);
        for (int r = 0; r < R; r++) {
            if (flags[r] & ctag::kMfitLeftOut) continue;
            const int m = rec_model[r];
            n_records[m]++;
            for (int c = 0; c < pm; c++) count[(size_t)m * pm + c] += table[(size_t)r * pm + c] >= 0 ? 1 : 0;
        }
        held.assign((size_t)n_models * pm, 1);
        for (int m = 0; m < n_models; m++)
            for (int c = 0; c < pm; c++)
                if (count[(size_t)m * pm + c] >= min_obs) {
                    held[(size_t)m * pm + c] = 0;
                    n_fitted[m]++;
                }
    }

    int upload_held() { return hipMemcpyAsync(d_held.p, held.data(), held.size(), hipMemcpyHostToDevice, s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP; }

    // delta[n_models][N] and bad[n_models] for the models with active[m] != 0.  Waits.
    int solve(const std::vector<double>& lambda, const std::vector<int32_t>& active, std::vector<double>& delta, std::vector<int32_t>& bad) {
        FIT_HIP(hipMemcpyAsync(d_lambda.p, lambda.data(), sizeof(double) * n_models, hipMemcpyHostToDevice, s));
        FIT_HIP(hipMemcpyAsync(d_active.p, active.data(), sizeof(int32_t) * n_models, hipMemcpyHostToDevice, s));
        FIT_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int32_t) * n_models, s));
        FIT_HIP(hipMemsetAsync(d_delta.p, 0, sizeof(double) * (size_t)n_models * N, s));
        if (timing) FIT_HIP(hipEventRecord(st->ev[0], s));
        hipLaunchKernelGGL(ctag::k_mfit_solve, dim3(n_models), dim3(ctag::kMfitSolveThreads), 0, s, d_S.p, d_g.p, d_held.p, d_lambda.p, d_active.p, pm, d_A.p,
                           d_delta.p, d_bad.p);
        FIT_HIP(hipGetLastError());
        if (timing) FIT_HIP(hipEventRecord(st->ev[1], s));
        delta.resize((size_t)n_models * N);
        bad.resize(n_models);
        FIT_HIP(hipMemcpyAsync(delta.data(), d_delta.p, sizeof(double) * delta.size(), hipMemcpyDeviceToHost, s));
        FIT_HIP(hipMemcpyAsync(bad.data(), d_bad.p, sizeof(int32_t) * n_models, hipMemcpyDeviceToHost, s));
        FIT_HIP(hipStreamSynchronize(s));
        if (timing) {
            float a = 0.f;
            (void)hipEventElapsedTime(&a, st->ev[0], st->ev[1]);
            st->ms[3] += a;
        }
        return CTAG_OK;
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
    double U[9], sv[3], V[9];
    ctl::svd3(C, U, sv, V);
    auto det3 = [](const double* M) {
        return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    };
    const double sg = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    double Rm[9];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) Rm[a * 3 + b] = U[a * 3] * V[b * 3] + U[a * 3 + 1] * V[b * 3 + 1] + sg * U[a * 3 + 2] * V[b * 3 + 2];
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
    if (r.max_rounds < 0 || r.min_obs < 1) return CTAG_ERR_ARG;
    for (double v : {r.lambda0, r.lambda_max, r.rel_tol})
        if (!std::isfinite(v) || !(v > 0.0)) return CTAG_ERR_ARG;
    if (!std::isfinite(r.strip_height)) return CTAG_ERR_ARG;
    return CTAG_OK;
}

int clone_model(const ctag_model* seed, ctag_model** out) {
    ctag_model_view v;
    if (ctag_model_get_view(seed, &v) != CTAG_OK) return CTAG_ERR_ARG;
    return ctag_model_create(&v, out);
}

struct ModelGuard {  // frees the working model unless it is handed out
    ctag_model* m = nullptr;
    ~ModelGuard() {
        if (m) ctag_model_free(m);
    }
};

// pose records of the working model W (its device corners are current) into poses_dev, then to the host.  Waits.
int pose_pass(FitWork& w, ctag_model* W, const ctag_camera* camera, int32_t* offsets_dev, ctag_pose_rec* poses_dev, int total, std::vector<ctag_pose_rec>& host) {
    if (w.timing) FIT_HIP(hipEventRecord(w.st->ev[0], w.s));
    const int rc = ctag_pose_batch_device(w.h, w.res, w.n_frames, W, camera, offsets_dev, poses_dev, total);
    if (rc != CTAG_OK) return rc;
    if (w.timing) FIT_HIP(hipEventRecord(w.st->ev[1], w.s));
    host.resize(total);
    FIT_HIP(hipMemcpyAsync(host.data(), poses_dev, sizeof(ctag_pose_rec) * (size_t)total, hipMemcpyDeviceToHost, w.s));
    FIT_HIP(hipStreamSynchronize(w.s));
    if (w.timing) {
        float a = 0.f;
        (void)hipEventElapsedTime(&a, w.st->ev[0], w.st->ev[1]);
        w.st->ms[0] += a;
    }
    return CTAG_OK;
}

// the working model's corners to its device copy, behind what is enqueued on the stream
int push_corners(FitWork& w, ctag_model* W) {
    return hipMemcpyAsync(W->d_corners.p, W->corners.data(), sizeof(float) * W->corners.size(), hipMemcpyHostToDevice, w.s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

int fit_prepare(FitWork& w, ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_camera* camera) {
    w.h = h;
    FIT_HIP(hipSetDevice(ctag::handle_device(h)));
    w.st = fit_state(h);
    if (!w.st) return CTAG_ERR_HIP;
    w.s = static_cast<hipStream_t>(ctag_stream(h));
    w.timing = ctag::handle_timing(h);
    for (float& v : w.st->ms) v = 0.f;
    w.res = results_dev;
    w.n_frames = n_frames;
    w.cam = ctag::make_pose_cam(camera);
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
    int rc = fit_prepare(w, h, nullptr, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    if (model_to_device(model, handle_device(h)) != CTAG_OK) return CTAG_ERR_HIP;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<ctag_pose_rec> d_poses;
    FIT_HIP(d_res.grow(n_frames));
    FIT_HIP(d_poses.grow(n_poses));
    FIT_HIP(hipMemcpyAsync(d_res.p, results, sizeof(ctag_frame_result) * (size_t)n_frames, hipMemcpyHostToDevice, w.s));
    FIT_HIP(hipMemcpyAsync(d_poses.p, poses, sizeof(ctag_pose_rec) * (size_t)n_poses, hipMemcpyHostToDevice, w.s));
    w.res = d_res.p;
    for (int i = 0; i < n_poses; i++)
        if (poses[i].status == CTAG_POSE_OK && poses[i].model_index >= 0 && poses[i].model_index < model->n_models) {
            w.ok.push_back(i);
            w.rec_model.push_back(poses[i].model_index);
        }
    const int pm = model->model_size * 8, N = 3 * pm;
    if (w.ok.empty()) return CTAG_ERR_ARG;
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
    for (int r = 0; r < w.R; r++)
        if (w.rec_model[r] == model_index && (w.flags[r] & kMfitSingular)) *bad_pivot = 1;
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

int ctag_model_fit_last_ms(ctag_handle* h, float* out4) {
    if (!h || !out4) return CTAG_ERR_ARG;
    FitState* st = fit_state(h);
    if (!st) return CTAG_ERR_HIP;
    for (int i = 0; i < 4; i++) out4[i] = st->ms[i];
    return CTAG_OK;
}

int ctag_model_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* seed, const ctag_camera* camera,
                          const ctag_model_fit_opts* opts_in, ctag_model** out, ctag_model_fit_stat* stats) {
    if (!h || !results_dev || n_frames < 1 || !seed || !camera || !out || !stats) return CTAG_ERR_ARG;
    ctag_model_fit_opts opts;
    if (fit_opts(opts_in, opts) != CTAG_OK) return CTAG_ERR_ARG;
    if (seed->model_size != ctag::handle_dict_cols(h) || seed->model_size > CTAG_MAX_CODE_POS) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    if ((long long)n_frames * CTAG_MAX_MARKERS > (1ll << 30)) return CTAG_ERR_LIMIT;
    FitWork w;
    int rc = fit_prepare(w, h, results_dev, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    ModelGuard guard;
    rc = clone_model(seed, &guard.m);
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
    FIT_HIP(d_off.grow((size_t)n_frames + 1));
    FIT_HIP(d_poses.grow(1));
    // capacity 1: the call is made for offsets[n_frames], the record count, and for W's device copy; the one pose it solves is discarded
    rc = ctag_pose_batch_device(h, results_dev, n_frames, W, camera, d_off.p, d_poses.p, 1);
    if (rc != CTAG_OK) return rc;
    int32_t total = 0;
    FIT_HIP(hipMemcpyAsync(&total, d_off.p + n_frames, sizeof(int32_t), hipMemcpyDeviceToHost, w.s));
    FIT_HIP(hipStreamSynchronize(w.s));
    if (total <= 0) return hand_out();
    FIT_HIP(d_poses.grow((size_t)total));
    std::vector<ctag_pose_rec> acc, trial;
    rc = pose_pass(w, W, camera, d_off.p, d_poses.p, total, acc);
    if (rc != CTAG_OK) return rc;
    for (int i = 0; i < total; i++)
        if (acc[i].status == CTAG_POSE_OK) {
            w.ok.push_back(i);
            w.rec_model.push_back(acc[i].model_index);
        }
    if (w.ok.empty()) return hand_out();
    rc = w.setup(nm, pm, 0);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(W->d_corners.p, W->d_ids.p, d_poses.p, true);
    if (rc != CTAG_OK) return rc;
    const int R = w.R;
    std::vector<uint8_t> left_out(R);
    for (int r = 0; r < R; r++) left_out[r] = (w.flags[r] & ctag::kMfitLeftOut) ? 1 : 0;

    // ---- rule 2
    std::vector<int> n_records, n_fitted;
    w.find_held(opts.min_obs, n_records, n_fitted);
    rc = w.upload_held();
    if (rc != CTAG_OK) return rc;

    // cost of model m over its observation records, in record order; false when one of them is not CTAG_POSE_OK
    std::vector<long long> n_points(nm, 0);
    auto costs_of = [&](const std::vector<ctag_pose_rec>& P, std::vector<double>& cost, std::vector<uint8_t>& all_ok) {
        cost.assign(nm, 0.0);
        all_ok.assign(nm, 1);
        for (int r = 0; r < R; r++) {
            if (left_out[r]) continue;
            const ctag_pose_rec& p = P[w.ok[r]];
            const int m = w.rec_model[r];
            if (p.status != CTAG_POSE_OK) all_ok[m] = 0;
            cost[m] += p.cost;
        }
    };
    std::vector<double> cost_cur, cost_trial, lambda(nm, opts.lambda0), delta;
    std::vector<uint8_t> ok_cur, ok_trial;
    std::vector<int32_t> active(nm, 0), bad;
    costs_of(acc, cost_cur, ok_cur);
    for (int r = 0; r < R; r++)
        if (!left_out[r]) n_points[w.rec_model[r]] += acc[w.ok[r]].n_points;
    bool any = false;
    for (int m = 0; m < nm; m++) {
        stats[m].n_records = n_records[m];
        stats[m].n_points_fitted = n_fitted[m];
        stats[m].n_points_held = pm - n_fitted[m];
        stats[m].cost0 = stats[m].cost = cost_cur[m];
        if (n_records[m] > 0 && n_fitted[m] > 0) {
            stats[m].status = CTAG_POSE_OK;
            active[m] = opts.max_rounds > 0 ? 1 : 0;
            any = any || active[m];
        }
    }

    // ---- rules 3-5: the rounds.  `accepted` is the accepted state of every model; W carries the trial during a round
    std::vector<float> accepted = W->corners;
    const std::vector<float>& seed_corners = seed->corners;
    bool need_system = false;
    std::vector<double> X, Y;
    while (any) {
        if (need_system) {
            W->corners = accepted;
            if (push_corners(w, W) != CTAG_OK) return CTAG_ERR_HIP;
            FIT_HIP(hipMemcpyAsync(d_poses.p, acc.data(), sizeof(ctag_pose_rec) * (size_t)total, hipMemcpyHostToDevice, w.s));
            rc = w.build_system(W->d_corners.p, W->d_ids.p, d_poses.p, false);
            if (rc != CTAG_OK) return rc;
            need_system = false;
        }
        rc = w.solve(lambda, active, delta, bad);
        if (rc != CTAG_OK) return rc;
        for (int r = 0; r < R; r++)
            if (!left_out[r] && (w.flags[r] & ctag::kMfitSingular)) bad[w.rec_model[r]] = 1;
        W->corners = accepted;
        bool any_trial = false;
        for (int m = 0; m < nm; m++) {
            if (!active[m] || bad[m]) continue;
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
            if (push_corners(w, W) != CTAG_OK) return CTAG_ERR_HIP;
            rc = pose_pass(w, W, camera, d_off.p, d_poses.p, total, trial);
            if (rc != CTAG_OK) return rc;
            costs_of(trial, cost_trial, ok_trial);
        }
        any = false;
        for (int m = 0; m < nm; m++) {
            if (!active[m]) continue;
            stats[m].rounds++;
            if (!bad[m] && ok_trial[m] && cost_trial[m] < cost_cur[m]) {
                const double drop = cost_cur[m] - cost_trial[m];
                cost_cur[m] = cost_trial[m];
                std::memcpy(&accepted[(size_t)m * pm * 3], &W->corners[(size_t)m * pm * 3], sizeof(float) * (size_t)pm * 3);
                for (int r = 0; r < R; r++)
                    if (w.rec_model[r] == m) acc[w.ok[r]] = trial[w.ok[r]];
                lambda[m] = std::max(lambda[m] / 3.0, 1e-9);
                need_system = true;
                if (drop < opts.rel_tol * cost_cur[m]) active[m] = 0;
            } else {
                lambda[m] *= 4.0;
                if (lambda[m] > opts.lambda_max) active[m] = 0;
            }
            if (stats[m].rounds >= opts.max_rounds) active[m] = 0;
            any = any || active[m];
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
        if (push_corners(w, W) != CTAG_OK) return CTAG_ERR_HIP;
        rc = pose_pass(w, W, camera, d_off.p, d_poses.p, total, trial);
        if (rc != CTAG_OK) return rc;
        costs_of(trial, cost_cur, ok_cur);
    }
    for (int m = 0; m < nm; m++) {
        if (stats[m].status != CTAG_POSE_OK) continue;
        stats[m].cost = cost_cur[m];
        stats[m].lambda = lambda[m];
        stats[m].rms_px = n_points[m] > 0 ? std::sqrt(2.0 * cost_cur[m] / (double)n_points[m]) : 0.0;
    }
    // the device copies belong to the trial states of the call: the model handed out makes its own at its first use
    W->d_ids.release();
    W->d_corners.release();
    W->d_base_axis.release();
    W->d_base = W->d_axis = nullptr;
    W->device = -1;
    return hand_out();
}

int ctag_model_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* seed, const ctag_camera* camera,
                   const ctag_model_fit_opts* opts, ctag_model** out, ctag_model_fit_stat* stats) {
    if (!h || !results || n_frames < 1 || !seed || !camera || !out || !stats) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    ctag::DevBuf<ctag_frame_result> d_res;
    FIT_HIP(d_res.grow((size_t)n_frames));
    FIT_HIP(hipMemcpy(d_res.p, results, sizeof(ctag_frame_result) * (size_t)n_frames, hipMemcpyHostToDevice));
    return ctag_model_fit_device(h, d_res.p, n_frames, seed, camera, opts, out, stats);
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
