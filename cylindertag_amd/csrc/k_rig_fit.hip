// k_rig_fit.hip -- assembly of the models of a rig into one common frame from the detection records of frames that show two or
// more of its markers together, on the device.  The semantics are stated in include/ctag_pose.h (rig assembly, rules 1-7).
//
// Mapping.  The reprojection problem over member transforms and per-frame rig poses separates: given the
// transforms a frame's rig pose is the solve k_rig_pose already does, so a round is
//   pose      ctag_rig_pose_batch_device on the call's working copy of the model (k_rig_pose.hip, untouched);
//   record    k_rfit_record: one wavefront per observation record, grid-stride.  The member walk is the builder's (marker_points
//             over the record's member_mask, as k_pose_cov's rig source has it), corner_point and point_residual are the pose
//             kernels'.  A member's points are one contiguous run of the record, lane l takes the points l, l + 64, ... of the run.
//             Pass 1: the 21 entries of U = sum Jp^T Jp and the 6 of sum Jp^T r over all points through wave_sum_f64, every lane
//             factors U = L L^T.  Pass 2, member by member: the 36 + 21 + 6 sums of Jp^T Jm, Jm^T Jm and Jm^T r over the member's
//             run through wave_sum_f64 (lanes without a point of the run add zeros: masked wave sums), then Z = L^-1 (Jp^T Jm) and
//             g = Jm^T r - Z^T y: 63 doubles per member slot, plus the record's model-slot -> member table (int8, -1 where absent);
//   assemble  k_rfit_assemble: for rig g one thread per entry (i <= j) of its 96 x 96 S; it walks the records in record order
//             (other rigs' records skipped by a block-uniform branch), subtracts Z_a^T Z_b and adds Jm^T Jm on the diagonal blocks;
//             g the same way.  The running sums live in global memory between passes of the record workspace, so the result does not
//             depend on the pass size;
//   solve     k_fit_solve<96> (ctag_fit_solve.h): one block per rig, the damped system (S + lambda diag S) as a packed lower triangle in LDS (at most
//             96 x 97 / 2 doubles, 37 KB), right-looking Cholesky, the dropped rows (the anchor's) as identity rows with a zero
//             right-hand side, the two triangular solves, delta and a flag for a pivot that is not positive.
// The host decides (initial assembly, accept / reject, lambda, stop) per rig between the launches.  FP64 VALU like the pose kernels;
// the largest system is 90 x 90, nothing here is MFMA-shaped.
//
// What the assembly shares with the model reconstruction (k_model_fit.hip) is not here: the pose block of a record (pass 1, a column
// through L^-1, the point Jacobian) is ctag_schur6.h's, the point descriptor and load_state6 are ctag_pose_dev.h's, and the host side
// of a fit -- timed state, call context, working model, systems with their pass loop and solve, the accept / reject rule --
// is ctag_fit_host.h's.  This file keeps its kernels' own walk, tables and pass 2, the initial assembly of rules 1-4,
// apply_rigid, report_transforms, the probe, and its round loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_fit_host.h"
#include "ctag_fit_solve.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"
#include "ctag_schur6.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_rig_fit_opts) == 32, "ctag_rig_fit_opts layout");
static_assert(sizeof(ctag_rig_fit_stat) == 64, "ctag_rig_fit_stat layout");
static_assert(sizeof(ctag_rig_fit_model_stat) == 72, "ctag_rig_fit_model_stat layout");

namespace ctag {

constexpr int kRfitGrid = 256;            // wavefronts of one k_rfit_record launch at most
constexpr int kRfitPassRecords = 512;     // observation records one pass of the workspace holds
constexpr int kRfitSlots = CTAG_RIG_FIT_MAX_MODELS;  // member slots of a record, model slots of a rig
constexpr int kRfitDoubles = 63;          // per member slot of a record: Z (36), Jm^T Jm (21, upper triangle in row order), g (6)
constexpr int kRfitN = 6 * kRfitSlots;    // 96: row stride of S, delta and g
constexpr int kRfitMaxPts = CTAG_RIG_MAX_POINTS;
// flags of a record: kRecLeftOut (it does not describe its detection record: never for records k_rig_solve wrote) and kRecSingular

struct RfitLds {
    int32_t src[kRfitMaxPts];        // point i: its descriptor (point_desc, ctag_pose_dev.h; camera 0)
    int32_t mstart[kRfitSlots + 1];  // member k owns the points mstart[k] .. mstart[k + 1] - 1
    int32_t mmodel[kRfitSlots];      // its model index
    int8_t table[kRfitSlots];        // model slot of the rig -> member, -1 where absent
};

// Observation records r0 .. r1-1 (indices into obs, which holds rig-pose record indices): workspace slot r - r0 gets the 63 doubles of
// every member, table row r the model-slot -> member map, flags[r] the record's state.
__global__ __launch_bounds__(64) void k_rfit_record(const ctag_frame_result* __restrict__ res, int n_frames, const ctag_rig_pose_rec* __restrict__ recs,
                                                    const int32_t* __restrict__ obs, int r0, int r1, PoseModelDev model,
                                                    const int32_t* __restrict__ slot_of_model, PoseCam cam, double* __restrict__ ws,
                                                    int8_t* __restrict__ table, int32_t* __restrict__ flags) {
    __shared__ RfitLds L;
    const int lane = threadIdx.x;
    for (int r = r0 + (int)blockIdx.x; r < r1; r += gridDim.x) {
        const ctag_rig_pose_rec& P = recs[obs[r]];
        int8_t* T = table + (size_t)r * kRfitSlots;
        wave_sync();  // the previous record's LDS reads are done
        if (lane < kRfitSlots) L.table[lane] = -1;
        wave_sync();
        int n = 0, nmem = 0;
        bool ok = P.status == CTAG_POSE_OK && P.frame >= 0 && P.frame < n_frames;
        if (ok) {
            const ctag_frame_result& FR = res[P.frame];
            ok = FR.status == CTAG_OK;
            const int nm = ok ? min(max(FR.n_markers, 0), CTAG_MAX_MARKERS) : 0;
            const ctag_feature_rec* F0 = FR.features;
            for (int k = 0; k < nm && ok; k++) {  // wave-uniform
                if (!((P.member_mask[k >> 5] >> (k & 31)) & 1u)) continue;
                const int mi = model_lookup(model, FR.markers[k].marker_id);
                if (mi < 0 || slot_of_model[mi] < 0 || nmem >= kRfitSlots) {
                    ok = false;
                    break;
                }
                const int base = n;
                int nl = 0;
                const int st = marker_points(FR, FR.markers[k], model.model_size, kPoseMaxPts, nl, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
                    if (lane < cnt && base + i0 + cnt <= kRfitMaxPts) L.src[base + i0 + lane] = point_desc((int)(&F - F0), lane, 0, pos);
                });
                if (st != CTAG_POSE_OK || base + nl > kRfitMaxPts) {
                    ok = false;
                    break;
                }
                if (lane == 0) {
                    L.mstart[nmem] = base;
                    L.mmodel[nmem] = mi;
                    L.table[slot_of_model[mi]] = (int8_t)nmem;
                }
                nmem++;
                n += nl;
            }
        }
        if (lane == 0) L.mstart[min(nmem, kRfitSlots)] = n;
        ok = ok && n == P.n_points && n >= 4 && nmem >= 2;
        double x[6];
        ok = load_state6(P, x) && ok;
        wave_sync();
        if (!ok) {  // wave-uniform
            if (lane < kRfitSlots) T[lane] = -1;
            if (lane == 0) flags[r] = kRecLeftOut;
            continue;
        }
        if (lane < kRfitSlots) T[lane] = L.table[lane];
        const ctag_frame_result& FR = res[P.frame];
        double R[9], dR[27];
        ctl::angle_axis_rot(x, R, dR);
        // ---- pass 1: U and sum Jp^T r over the record's points, member by member, lane l owning points l, l + 64, ... of a member's run
        double H[21], b[6];
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) b[a] = 0.0;
        for (int k = 0; k < nmem; k++) {
            const float* __restrict__ corners = model.corners + (size_t)L.mmodel[k] * model.model_size * 24;
            const int i1 = L.mstart[k + 1];
            for (int i = L.mstart[k] + lane; i < i1; i += 64) {
                const int s = L.src[i];
                double xn, yn, ob[2], X[3], q0, q1, j0[6], j1[6];
                corner_point(cam, corners, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, X);
                point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, X, ob, q0, q1, j0, j1, true);
                gram6_add(j0, j1, H);
                grad6_add(j0, j1, q0, q1, b);
            }
        }
        double Lc[36];
        const bool pd = pose_block6(H, b, Lc);  // the same in every lane; b is y from here on
        if (lane == 0) flags[r] = pd ? 0 : kRecSingular;
        if (!pd) continue;
        // ---- pass 2: the 63 doubles of every member
        double* W = ws + (size_t)(r - r0) * kRfitSlots * kRfitDoubles;
        for (int k = 0; k < nmem; k++) {
            const float* __restrict__ corners = model.corners + (size_t)L.mmodel[k] * model.model_size * 24;
            const int i1 = L.mstart[k + 1];
            double Z[36], A[21], gm[6];
#pragma unroll
            for (int e = 0; e < 36; e++) Z[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 21; e++) A[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) gm[e] = 0.0;
            for (int i = L.mstart[k] + lane; i < i1; i += 64) {
                const int s = L.src[i];
                double xn, yn, ob[2], Y[3], q0, q1, j0[6], j1[6];
                corner_point(cam, corners, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, Y);
                point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, Y, ob, q0, q1, j0, j1, true);
                double x0[3], x1[3], m0[6], m1[6];
                point_dX(R, j0, j1, x0, x1);  // d residual / d Y
                // Jm = (dr/dY) [-[Y]x | I]: the rotation columns are Y x (dr/dY)
                m0[0] = Y[1] * x0[2] - Y[2] * x0[1];
                m0[1] = Y[2] * x0[0] - Y[0] * x0[2];
                m0[2] = Y[0] * x0[1] - Y[1] * x0[0];
                m1[0] = Y[1] * x1[2] - Y[2] * x1[1];
                m1[1] = Y[2] * x1[0] - Y[0] * x1[2];
                m1[2] = Y[0] * x1[1] - Y[1] * x1[0];
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    m0[3 + m] = x0[m];
                    m1[3 + m] = x1[m];
                }
                int e = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int c = 0; c < 6; c++) {
                        Z[a * 6 + c] += j0[a] * m0[c];
                        Z[a * 6 + c] += j1[a] * m1[c];
                    }
#pragma unroll
                    for (int c = a; c < 6; c++) {
                        A[e] += m0[a] * m0[c];
                        A[e] += m1[a] * m1[c];
                        e++;
                    }
                    gm[a] += m0[a] * q0;
                    gm[a] += m1[a] * q1;
                }
            }
#pragma unroll
            for (int e = 0; e < 36; e++) Z[e] = wave_sum_f64(Z[e]);
#pragma unroll
            for (int e = 0; e < 21; e++) A[e] = wave_sum_f64(A[e]);
#pragma unroll
            for (int e = 0; e < 6; e++) gm[e] = wave_sum_f64(gm[e]);
#pragma unroll
            for (int c = 0; c < 6; c++) {  // column c of Z <- L^-1 (column c), g_c -= Z_c . y
                double z[6];
#pragma unroll
                for (int a = 0; a < 6; a++) z[a] = Z[a * 6 + c];
                gm[c] -= forward6_dot(Lc, z, b);
#pragma unroll
                for (int a = 0; a < 6; a++) Z[a * 6 + c] = z[a];
            }
            if (lane == 0) {
                double* O = W + (size_t)k * kRfitDoubles;
#pragma unroll
                for (int e = 0; e < 36; e++) O[e] = Z[e];
#pragma unroll
                for (int e = 0; e < 21; e++) O[36 + e] = A[e];
#pragma unroll
                for (int e = 0; e < 6; e++) O[57 + e] = gm[e];
            }
        }
    }
}

// Adds records r0 .. r1-1 to S and g of rig blockIdx.y.  Thread t < 96 x 96: entry (i, j) = (t / 96, t % 96) of S, the threads with
// i <= j work and write both triangles; 96 x 96 <= t < 96 x 96 + 96: entry t - 96 x 96 of g.  S: [n_rigs][96][96], g: [n_rigs][96]; model
// slot a of the rig owns rows 6a .. 6a + 5.
__global__ __launch_bounds__(256) void k_rfit_assemble(const double* __restrict__ ws, const int8_t* __restrict__ table, const int32_t* __restrict__ rec_rig,
                                                       const int32_t* __restrict__ flags, int r0, int r1, double* __restrict__ S, double* __restrict__ g) {
    const int rig = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    constexpr int NN = kRfitN * kRfitN;
    const int i = t < NN ? t / kRfitN : t - NN, j = t < NN ? t - i * kRfitN : 0;
    const bool is_s = t < NN && i <= j, is_g = t >= NN && t < NN + kRfitN;
    if (!is_s && !is_g) return;
    const int a = i / 6, p = i - 6 * a, bs = j / 6, q = j - 6 * bs;
    double* dst = is_s ? S + (size_t)rig * NN + (size_t)i * kRfitN + j : g + (size_t)rig * kRfitN + i;
    double acc = *dst;
    int ea = 0;  // index of (p, q) in the upper triangle's row order
    if (is_s && a == bs) ea = p * 6 - p * (p - 1) / 2 + (q - p);
    for (int r = r0; r < r1; r++) {
        if (rec_rig[r] != rig || flags[r] != 0) continue;  // the same for the whole block
        const int ka = table[(size_t)r * kRfitSlots + a];
        if (ka < 0) continue;
        const double* za = ws + ((size_t)(r - r0) * kRfitSlots + ka) * kRfitDoubles;
        if (is_g) {
            acc += za[57 + p];
            continue;
        }
        const int kb = table[(size_t)r * kRfitSlots + bs];
        if (kb < 0) continue;
        const double* zb = ws + ((size_t)(r - r0) * kRfitSlots + kb) * kRfitDoubles;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += za[k * 6 + p] * zb[k * 6 + q];
        acc -= s;
        if (a == bs) acc += za[36 + ea];
    }
    *dst = acc;
    if (is_s && i != j) S[(size_t)rig * NN + (size_t)j * kRfitN + i] = acc;
}

}  // namespace ctag

// =====================================================================================================
// host side: the parts the assembly shares with the model reconstruction are ctag_fit_host.h's (namespace ctag::fit)
// =====================================================================================================
namespace {

namespace fit = ctag::fit;

struct Rigid {  // X_rig = R X_in + t
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
};

void mat_mul(const double* A, const double* B, double* C) {  // C = A B, 3x3 row-major, sums in index order
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

void mat_vec(const double* A, const double* v, double* o) {
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}

// The device side of one call: the rigs' systems (a group is a rig), the record workspace, and the slots of the models in them.
struct RfitWork : fit::Systems {
    fit::Call c;
    std::vector<int32_t> slot_of_model;  // [n_models]: the model's slot in its rig's system, -1 outside every system
    std::vector<int32_t> n_slots, drop;  // [n_rigs]
    ctag::DevBuf<int32_t> d_slot, d_n_slots, d_drop;
    ctag::DevBuf<int8_t> d_table;
    ctag::DevBuf<double> d_ws;

    int setup(int pass_records) {
        const int n_rigs = (int)n_slots.size(), n_models = (int)slot_of_model.size();
        if ((size_t)n_rigs * ctag::kRfitN * ctag::kRfitN * 8 > ((size_t)2 << 30)) return CTAG_ERR_LIMIT;
        const int rc = Systems::setup(c, n_rigs, ctag::kRfitN, pass_records, ctag::kRfitPassRecords);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_table.grow((size_t)std::max(R, 1) * ctag::kRfitSlots));
        FIT_HIP(d_ws.grow((size_t)pass * ctag::kRfitSlots * ctag::kRfitDoubles));
        FIT_HIP(d_n_slots.grow(n_rigs));
        FIT_HIP(d_drop.grow(n_rigs));
        FIT_HIP(d_slot.grow(std::max(n_models, 1)));
        if (n_models > 0) FIT_HIP(hipMemcpyAsync(d_slot.p, slot_of_model.data(), sizeof(int32_t) * n_models, hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipMemcpyAsync(d_n_slots.p, n_slots.data(), sizeof(int32_t) * n_rigs, hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipMemcpyAsync(d_drop.p, drop.data(), sizeof(int32_t) * n_rigs, hipMemcpyHostToDevice, c.s));
        return CTAG_OK;
    }

    // S and g of every rig at (model, recs_dev); slot 2 times the record and the assemble kernel together.  Waits.
    int build_system(const ctag_model* model, const ctag_rig_pose_rec* recs_dev) {
        const ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
        constexpr int kThreads = ctag::kRfitN * ctag::kRfitN + ctag::kRfitN;
        return build(c, [&](int r0, int r1) {
            if (c.mark(0) != CTAG_OK) return CTAG_ERR_HIP;
            hipLaunchKernelGGL(ctag::k_rfit_record, dim3(std::min(r1 - r0, ctag::kRfitGrid)), dim3(64), 0, c.s, c.res, c.n_frames, recs_dev, d_obs.p, r0, r1, md,
                               d_slot.p, c.cam, d_ws.p, d_table.p, d_flags.p);
            hipLaunchKernelGGL(ctag::k_rfit_assemble, dim3((kThreads + 255) / 256, n_groups), dim3(256), 0, c.s, d_ws.p, d_table.p, d_rec_group.p, d_flags.p, r0, r1,
                               d_S.p, d_g.p);
            if (fit::launched() != CTAG_OK || c.mark(1) != CTAG_OK || c.reached(1) != CTAG_OK) return CTAG_ERR_HIP;
            c.add_ms(2, 0);
            return CTAG_OK;
        });
    }

    int solve(const std::vector<double>& lambda, const std::vector<int32_t>& active, int bad_flags, std::vector<double>& delta, std::vector<int32_t>& bad) {
        return Systems::solve(c, lambda, active, bad_flags, delta, bad, [&]() {
            hipLaunchKernelGGL(ctag::k_fit_solve<ctag::kRfitN>, dim3(n_groups), dim3(ctag::kFitSolveThreads), 0, c.s, d_S.p, d_g.p, d_n_slots.p, d_drop.p, d_lambda.p, d_active.p,
                               d_delta.p, d_bad.p);
        });
    }
};

int rfit_opts(const ctag_rig_fit_opts* o, ctag_rig_fit_opts& r) {
    ctag_rig_fit_opts_default(&r);
    if (o) r = *o;
    if (r.max_rounds < 0 || r.min_frames < 1) return CTAG_ERR_ARG;
    for (double v : {r.lambda0, r.lambda_max, r.rel_tol})
        if (!std::isfinite(v) || !(v > 0.0)) return CTAG_ERR_ARG;
    return CTAG_OK;
}

struct RigsGuard {
    ctag_rigs* r = nullptr;
    ~RigsGuard() {
        if (r) ctag_rigs_free(r);
    }
};

// rule 3: model m of W = T applied to model m of `in`, in double, rounded to float
void apply_rigid(const ctag_model* in, ctag_model* W, int m, const Rigid& T) {
    const int pm = in->model_size * 8;
    for (int c = 0; c < pm; c++) {
        const float* p = &in->corners[((size_t)m * pm + c) * 3];
        const double X[3] = {(double)p[0], (double)p[1], (double)p[2]};
        double Y[3];
        mat_vec(T.R, X, Y);
        for (int k = 0; k < 3; k++) W->corners[((size_t)m * pm + c) * 3 + k] = (float)(Y[k] + T.t[k]);
    }
    const double B[3] = {(double)in->base[3 * m], (double)in->base[3 * m + 1], (double)in->base[3 * m + 2]};
    const double Ax[3] = {(double)in->axis[3 * m], (double)in->axis[3 * m + 1], (double)in->axis[3 * m + 2]};
    double Y[3];
    mat_vec(T.R, B, Y);
    for (int k = 0; k < 3; k++) W->base[3 * m + k] = (float)(Y[k] + T.t[k]);
    mat_vec(T.R, Ax, Y);
    for (int k = 0; k < 3; k++) W->axis[3 * m + k] = (float)Y[k];
}

}  // namespace

namespace ctag {

int rfit_record_grid() { return kRfitGrid; }
int rfit_pass_records() { return kRfitPassRecords; }

// The reduced system of one rig, for the probe of libctag_testkit.so (include/ctag_testkit.h: ctag_testkit_rig_fit_system).
int rfit_probe_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* recs, const ctag_model* model_c,
                      const ctag_rigs* rigs, const ctag_camera* camera, int rig, double lambda, int pass_records, double* S, double* g, double* delta,
                      int32_t* n_unknowns, int32_t* bad_pivot) {
    if (!h || !results || n_frames < 1 || !recs || !model_c || !rigs || !S || !g || !delta || !n_unknowns || !bad_pivot) return CTAG_ERR_ARG;
    if (rigs->n_models != model_c->n_models || rig < 0 || rig >= rigs->n_rigs || !std::isfinite(lambda)) return CTAG_ERR_ARG;
    if ((long long)n_frames * rigs->n_rigs > (1ll << 28)) return CTAG_ERR_LIMIT;
    if (!camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    RfitWork w;
    int rc = w.c.prepare(h, kRigFitState, nullptr, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    const int n_rigs = rigs->n_rigs;
    w.slot_of_model.assign(model->n_models, -1);
    w.n_slots.assign(n_rigs, 0);
    w.drop.assign(n_rigs, 0);
    for (int m = 0; m < model->n_models; m++) {
        const int gi = rigs->rig_of_model[m];
        if (gi < 0) continue;
        if (w.n_slots[gi] >= kRfitSlots) return CTAG_ERR_ARG;
        w.slot_of_model[m] = w.n_slots[gi]++;
    }
    if (w.n_slots[rig] < 2) return CTAG_ERR_ARG;
    if (model_to_device(model, handle_device(h)) != CTAG_OK) return CTAG_ERR_HIP;
    const size_t n_items = (size_t)n_frames * n_rigs;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<ctag_rig_pose_rec> d_recs;
    rc = fit::upload_probe_inputs(w.c, results, d_res, recs, n_items, d_recs);
    if (rc != CTAG_OK) return rc;
    for (size_t i = 0; i < n_items; i++)
        if (recs[i].status == CTAG_POSE_OK && recs[i].n_members >= 2 && recs[i].rig >= 0 && recs[i].rig < n_rigs) {
            w.obs.push_back((int32_t)i);
            w.rec_group.push_back(recs[i].rig);
        }
    if (w.obs.empty()) return CTAG_ERR_ARG;
    rc = w.setup(pass_records);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(model, d_recs.p);
    if (rc != CTAG_OK) return rc;
    std::vector<double> lam(n_rigs, lambda), d;
    std::vector<int32_t> active(n_rigs, 0), bad;
    active[rig] = 1;
    rc = w.solve(lam, active, kRecSingular, d, bad);  // a caller's record may be left out; that does not make the rig bad here
    if (rc != CTAG_OK) return rc;
    const int N = 6 * w.n_slots[rig];
    std::vector<double> Sf((size_t)kRfitN * kRfitN), gf(kRfitN);
    FIT_HIP(hipMemcpy(Sf.data(), w.d_S.p + (size_t)rig * kRfitN * kRfitN, sizeof(double) * Sf.size(), hipMemcpyDeviceToHost));
    FIT_HIP(hipMemcpy(gf.data(), w.d_g.p + (size_t)rig * kRfitN, sizeof(double) * kRfitN, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; i++) {
        for (int j = 0; j < N; j++) S[(size_t)i * N + j] = Sf[(size_t)i * kRfitN + j];
        g[i] = gf[i];
        delta[i] = d[(size_t)rig * kRfitN + i];
    }
    *n_unknowns = N;
    *bad_pivot = bad[rig];
    return CTAG_OK;
}

}  // namespace ctag

extern "C" {

void ctag_rig_fit_opts_default(ctag_rig_fit_opts* o) {
    if (!o) return;
    o->max_rounds = 30;
    o->min_frames = 2;
    o->lambda0 = 1e-3;
    o->lambda_max = 1e6;
    o->rel_tol = 2.479e-5;  // 4 x 6.198e-6: what float32 rounding of the model alone does to the cost
}

int ctag_rig_fit_last_ms(ctag_handle* h, float* out4) { return fit::last_ms(h, ctag::kRigFitState, out4); }  // marker pose, rig pose, record + assemble, solve

int ctag_rig_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* in, const ctag_rigs* rigs,
                        const ctag_camera* camera, const ctag_rig_fit_opts* opts_in, ctag_model** out, ctag_rig_fit_stat* rig_stats,
                        ctag_rig_fit_model_stat* model_stats) {
    if (!h || !results_dev || n_frames < 1 || !in || !rigs || !camera || !out || !rig_stats || !model_stats) return CTAG_ERR_ARG;
    ctag_rig_fit_opts opts;
    if (rfit_opts(opts_in, opts) != CTAG_OK) return CTAG_ERR_ARG;
    if (in->model_size != ctag::handle_dict_cols(h) || in->model_size > CTAG_MAX_CODE_POS) return CTAG_ERR_ARG;
    if (rigs->n_models != in->n_models) return CTAG_ERR_ARG;
    const int nm = in->n_models, ng = rigs->n_rigs;
    std::vector<std::vector<int>> members(ng);  // models of every rig, ascending
    for (int m = 0; m < nm; m++)
        if (rigs->rig_of_model[m] >= 0) members[rigs->rig_of_model[m]].push_back(m);
    for (int g = 0; g < ng; g++)
        if ((int)members[g].size() > CTAG_RIG_FIT_MAX_MODELS) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    if ((long long)n_frames * CTAG_MAX_MARKERS > (1ll << 30) || (long long)n_frames * ng > (1ll << 28)) return CTAG_ERR_LIMIT;
    RfitWork w;
    int rc = w.c.prepare(h, ctag::kRigFitState, results_dev, n_frames, camera);
    if (rc != CTAG_OK) return rc;
    fit::ModelGuard guard;
    rc = fit::clone_model(in, &guard.m);
    if (rc != CTAG_OK) return rc;
    ctag_model* W = guard.m;
    for (int m = 0; m < nm; m++) {
        std::memset(&model_stats[m], 0, sizeof(model_stats[m]));
        model_stats[m].status = CTAG_POSE_NOT_SEEN;
        model_stats[m].rig = rigs->rig_of_model[m];
        model_stats[m].parent = -1;
    }
    for (int g = 0; g < ng; g++) {
        std::memset(&rig_stats[g], 0, sizeof(rig_stats[g]));
        rig_stats[g].status = CTAG_POSE_NOT_SEEN;
        rig_stats[g].anchor = -1;
        rig_stats[g].n_unplaced = (int)members[g].size();
        rig_stats[g].lambda = opts.lambda0;
    }
    auto hand_out = [&]() {
        fit::release_device_copies(W);
        *out = guard.m;
        guard.m = nullptr;
        return CTAG_OK;
    };
    if (nm == 0) return hand_out();

    // ---- rule 1: the per-marker poses under `in`
    ctag::DevBuf<int32_t> d_off;
    ctag::DevBuf<ctag_pose_rec> d_poses;
    std::vector<int32_t> off;
    rc = fit::count_pose_records(w.c, in, camera, d_off, d_poses, off);
    if (rc != CTAG_OK) return rc;
    const int32_t total = off[n_frames];
    if (total <= 0) return hand_out();
    std::vector<ctag_pose_rec> poses;
    rc = w.c.pose_pass(0, [&]() { return ctag_pose_batch_device(h, results_dev, n_frames, in, camera, d_off.p, d_poses.p, total); }, d_poses.p, (size_t)total, poses);
    if (rc != CTAG_OK) return rc;
    // seen[f][m]: the pose record of frame f that counts for model m, -1 if none
    std::vector<int32_t> seen((size_t)n_frames * nm, -1);
    {
        std::vector<uint8_t> claimed(nm);
        for (int f = 0; f < n_frames; f++) {
            std::fill(claimed.begin(), claimed.end(), 0);
            for (int i = off[f]; i < off[f + 1]; i++) {
                const int mi = poses[i].model_index;
                if (mi < 0 || mi >= nm || claimed[mi]) continue;
                claimed[mi] = 1;
                if (poses[i].status == CTAG_POSE_OK) seen[(size_t)f * nm + mi] = i;
            }
        }
    }

    // ---- rule 2: the initial assembly
    std::vector<Rigid> T(nm);
    std::vector<uint8_t> placed(nm, 0);
    w.slot_of_model.assign(nm, -1);
    w.n_slots.assign(ng, 0);
    w.drop.assign(ng, 0);
    for (int g = 0; g < ng; g++) {
        const std::vector<int>& M = members[g];
        const int k = (int)M.size();
        std::vector<int> cnt((size_t)k * k, 0);
        for (int f = 0; f < n_frames; f++)
            for (int a = 0; a < k; a++) {
                if (seen[(size_t)f * nm + M[a]] < 0) continue;
                for (int b = a + 1; b < k; b++)
                    if (seen[(size_t)f * nm + M[b]] >= 0) {
                        cnt[(size_t)a * k + b]++;
                        cnt[(size_t)b * k + a]++;
                    }
            }
        int anchor = -1;
        for (int a = 0; a < k && anchor < 0; a++)
            for (int b = 0; b < k; b++)
                if (cnt[(size_t)a * k + b] >= opts.min_frames) {
                    anchor = a;
                    break;
                }
        if (anchor < 0) continue;
        std::vector<uint8_t> in_tree(k, 0);
        in_tree[anchor] = 1;
        placed[M[anchor]] = 1;
        int n_placed = 1;
        for (;;) {
            int best = opts.min_frames - 1, ba = -1, bb = -1;
            for (int b = 0; b < k; b++) {  // ascending b, then ascending a: the first of equal counts stays
                if (in_tree[b]) continue;
                for (int a = 0; a < k; a++)
                    if (in_tree[a] && cnt[(size_t)a * k + b] > best) {
                        best = cnt[(size_t)a * k + b];
                        ba = a;
                        bb = b;
                    }
            }
            if (bb < 0) break;
            const int ma = M[ba], mb = M[bb];
            double sumR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sumt[3] = {0, 0, 0};
            for (int f = 0; f < n_frames; f++) {
                const int ia = seen[(size_t)f * nm + ma], ib = seen[(size_t)f * nm + mb];
                if (ia < 0 || ib < 0) continue;
                double Ra[9], Rb[9], RaT[9], Q[9], d[3], e[3];
                ctl::angle_axis_rot(poses[ia].rvec, Ra, nullptr);
                ctl::angle_axis_rot(poses[ib].rvec, Rb, nullptr);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) RaT[i * 3 + j] = Ra[j * 3 + i];
                mat_mul(RaT, Rb, Q);
                for (int i = 0; i < 9; i++) sumR[i] += Q[i];
                for (int i = 0; i < 3; i++) d[i] = poses[ib].tvec[i] - poses[ia].tvec[i];
                mat_vec(RaT, d, e);
                for (int i = 0; i < 3; i++) sumt[i] += e[i];
            }
            Rigid E;
            double sv[3];
            fit::nearest_rotation(sumR, E.R, sv);
            for (int i = 0; i < 3; i++) E.t[i] = sumt[i] / (double)best;
            Rigid& Tb = T[mb];
            const Rigid& Ta = T[ma];
            mat_mul(Ta.R, E.R, Tb.R);
            double e[3];
            mat_vec(Ta.R, E.t, e);
            for (int i = 0; i < 3; i++) Tb.t[i] = e[i] + Ta.t[i];
            in_tree[bb] = 1;
            placed[mb] = 1;
            n_placed++;
            model_stats[mb].parent = ma;
            model_stats[mb].n_frames_with_parent = best;
        }
        rig_stats[g].status = CTAG_POSE_OK;
        rig_stats[g].anchor = M[anchor];
        rig_stats[g].n_placed = n_placed;
        rig_stats[g].n_unplaced = k - n_placed;
        for (int a = 0; a < k; a++)
            if (in_tree[a]) {
                if (a == anchor) w.drop[g] = w.n_slots[g];
                w.slot_of_model[M[a]] = w.n_slots[g]++;
                model_stats[M[a]].status = CTAG_POSE_OK;
            }
    }
    auto moves = [&](int m) { return placed[m] && rig_stats[rigs->rig_of_model[m]].anchor != m; };  // placed and not its rig's anchor
    auto report_transforms = [&](const std::vector<Rigid>& TT) {
        for (int m = 0; m < nm; m++) {
            if (!moves(m)) continue;
            ctl::rodrigues_from_matrix(TT[m].R, model_stats[m].rvec);
            for (int i = 0; i < 3; i++) model_stats[m].tvec[i] = TT[m].t[i];
        }
    };
    // ---- rule 3: the working model at the initial assembly; rule 4: the rig set without the unplaced models
    for (int m = 0; m < nm; m++)
        if (moves(m)) apply_rigid(in, W, m, T[m]);
    report_transforms(T);
    std::vector<int32_t> rig_placed(nm);
    bool any_placed = false;
    for (int m = 0; m < nm; m++) {
        rig_placed[m] = placed[m] ? rigs->rig_of_model[m] : -1;
        any_placed = any_placed || placed[m];
    }
    if (!any_placed) return hand_out();
    RigsGuard rg;
    rc = ctag_rigs_create(W, rig_placed.data(), ng, &rg.r);
    if (rc != CTAG_OK) return rc;
    const size_t n_items = (size_t)n_frames * ng;
    ctag::DevBuf<ctag_rig_pose_rec> d_recs;
    FIT_HIP(d_recs.grow(n_items));
    std::vector<ctag_rig_pose_rec> acc, trial;
    // rig-pose records of W (its device corners are current) to the host, timed in slot 1
    auto rig_pose_pass = [&](std::vector<ctag_rig_pose_rec>& host) {
        return w.c.pose_pass(1, [&]() { return ctag_rig_pose_batch_device(h, results_dev, n_frames, W, rg.r, camera, d_recs.p); }, d_recs.p, n_items, host);
    };
    rc = rig_pose_pass(acc);
    if (rc != CTAG_OK) return rc;
    for (size_t i = 0; i < n_items; i++)
        if (acc[i].status == CTAG_POSE_OK && acc[i].n_members >= 2) {
            w.obs.push_back((int32_t)i);
            w.rec_group.push_back(acc[i].rig);
        }
    rc = w.setup(0);
    if (rc != CTAG_OK) return rc;
    const int R = w.R;
    fit::Lm lm;
    lm.start(ng, opts.lambda0);
    std::vector<uint8_t> ok_cur;
    w.costs_of(acc, nullptr, lm.cost, ok_cur);
    for (int r = 0; r < R; r++) {
        const ctag_rig_pose_rec& p = acc[w.obs[r]];
        ctag_rig_fit_stat& s = rig_stats[w.rec_group[r]];
        s.n_records++;
        s.n_points += p.n_points;
        for (int k = 0; k < CTAG_MAX_MARKERS; k++)  // pose record k of a frame is its marker k
            if ((p.member_mask[k >> 5] >> (k & 31)) & 1u) {
                const int i = off[p.frame] + k;
                if (i < off[p.frame + 1] && poses[i].model_index >= 0 && poses[i].model_index < nm) model_stats[poses[i].model_index].n_records++;
            }
    }
    for (int g = 0; g < ng; g++) {
        rig_stats[g].cost_init = rig_stats[g].cost = lm.cost[g];
        if (rig_stats[g].status == CTAG_POSE_OK && rig_stats[g].n_records > 0 && rig_stats[g].n_placed > 1) lm.active[g] = opts.max_rounds > 0 ? 1 : 0;
    }

    // ---- rule 5: the rounds.  T and acc_* are the accepted state of every model; W carries the trial during a round.  The loop is
    // the model reconstruction's (k_model_fit.hip, rules 3-5) but for the steps marked "rig"; the two are kept in step by hand
    std::vector<Rigid> Tt(nm);
    std::vector<float> acc_corners = W->corners, acc_base = W->base, acc_axis = W->axis;
    bool need_system = true;  // none has been built yet
    const int pm = W->model_size * 8;
    std::vector<double> delta, cost_trial(ng, 0.0);
    std::vector<uint8_t> ok_trial(ng, 0);
    std::vector<int32_t> bad;
    while (lm.any_active()) {
        if (need_system) {
            W->corners = acc_corners;
            if (fit::push_corners(w.c, W) != CTAG_OK) return CTAG_ERR_HIP;
            FIT_HIP(hipMemcpyAsync(d_recs.p, acc.data(), sizeof(ctag_rig_pose_rec) * n_items, hipMemcpyHostToDevice, w.c.s));
            rc = w.build_system(W, d_recs.p);
            if (rc != CTAG_OK) return rc;
            need_system = false;
        }
        // rig: every observation record was solved by k_rig_solve on this state, so one that is flagged at all makes its rig bad
        rc = w.solve(lm.lambda, lm.active, ~0, delta, bad);
        if (rc != CTAG_OK) return rc;
        W->corners = acc_corners;
        W->base = acc_base;
        W->axis = acc_axis;
        bool any_trial = false;
        for (int m = 0; m < nm; m++) {  // rig: T <- Exp(delta) T for the models that move
            if (!moves(m)) continue;
            const int g = rigs->rig_of_model[m];
            if (!lm.active[g] || bad[g]) continue;
            const double* d = &delta[(size_t)g * ctag::kRfitN + 6 * w.slot_of_model[m]];
            bool finite = true;
            for (int i = 0; i < 6; i++) finite = finite && std::isfinite(d[i]);
            if (!finite) {
                bad[g] = 1;
                continue;
            }
            double E[9], e[3];
            ctl::angle_axis_rot(d, E, nullptr);
            mat_mul(E, T[m].R, Tt[m].R);
            mat_vec(E, T[m].t, e);
            for (int i = 0; i < 3; i++) Tt[m].t[i] = e[i] + d[3 + i];
            apply_rigid(in, W, m, Tt[m]);
            any_trial = true;
        }
        if (any_trial) {
            if (fit::push_corners(w.c, W) != CTAG_OK) return CTAG_ERR_HIP;
            rc = rig_pose_pass(trial);
            if (rc != CTAG_OK) return rc;
            w.costs_of(trial, nullptr, cost_trial, ok_trial);
        }
        for (int g = 0; g < ng; g++) {
            if (!lm.active[g]) continue;
            // without a trial, cost_trial and ok_trial are an earlier round's
            if (!lm.decide(g, any_trial && !bad[g] && ok_trial[g], cost_trial[g], opts)) continue;
            for (int m : members[g]) {  // rig
                if (!moves(m)) continue;
                T[m] = Tt[m];
                std::memcpy(&acc_corners[(size_t)m * pm * 3], &W->corners[(size_t)m * pm * 3], sizeof(float) * (size_t)pm * 3);
                for (int k = 0; k < 3; k++) {
                    acc_base[3 * m + k] = W->base[3 * m + k];
                    acc_axis[3 * m + k] = W->axis[3 * m + k];
                }
            }
            w.take_records(g, trial, acc);
            need_system = true;
        }
    }
    W->corners = acc_corners;
    W->base = acc_base;
    W->axis = acc_axis;
    report_transforms(T);
    for (int g = 0; g < ng; g++) {
        if (rig_stats[g].status != CTAG_POSE_OK) continue;
        rig_stats[g].rounds = lm.rounds[g];
        rig_stats[g].cost = lm.cost[g];
        rig_stats[g].lambda = lm.lambda[g];
        rig_stats[g].rms_px = rig_stats[g].n_points > 0 ? std::sqrt(2.0 * lm.cost[g] / (double)rig_stats[g].n_points) : 0.0;
    }
    return hand_out();
}

int ctag_rig_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* in, const ctag_rigs* rigs, const ctag_camera* camera,
                 const ctag_rig_fit_opts* opts, ctag_model** out, ctag_rig_fit_stat* rig_stats, ctag_rig_fit_model_stat* model_stats) {
    if (!h || !results || n_frames < 1 || !in || !rigs || !camera || !out || !rig_stats || !model_stats) return CTAG_ERR_ARG;
    return fit::with_results_on_device(h, results, n_frames, [&](const ctag_frame_result* results_dev) {
        return ctag_rig_fit_device(h, results_dev, n_frames, in, rigs, camera, opts, out, rig_stats, model_stats);
    });
}

}  // extern "C"
