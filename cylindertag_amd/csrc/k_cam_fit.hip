// k_cam_fit.hip -- the poses of the cameras of a set in the frame of one of them, from the detection records of instants that two or
// more of them see together, on the device.  The semantics are stated in include/ctag_pose.h (camera set fit, rules 1-6).
//
// Mapping.  The reprojection problem over camera poses and per-instant rig poses separates: given the camera
// poses an instant's rig pose is the solve k_mv_solve already does, so a round is
//   pose      ctag_mv_rig_pose_batch_device under the trial camera set (k_mv_pose.hip, untouched);
//   record    k_cfit_record: one wavefront per observation record, grid-stride.  The walk is k_mv_count's / k_mv_solve's: camera,
//             marker, builder order (marker_points over member_mask[c]); corner_point and mv_point_residual are the pose kernels',
//             every camera's pixels undistorted with its own coefficients.  Lane l owns the points l, l + 64, ... of the record.
//             Pass 1: the 21 entries of U = sum Jp^T Jp and the 6 of sum Jp^T r over all points, pose_block6 (ctag_schur6.h).  Pass 2,
//             camera by camera: a camera's points are one contiguous run, so the 36 + 21 + 6 sums of Jp^T Jc, Jc^T Jc and Jc^T r over
//             it are wave sums in which the lanes without a point of the run add zeros; then Z = L^-1 (Jp^T Jc) and
//             g = Jc^T r - Z^T y: 63 doubles per camera slot, 8 slots, plus the record's mask of cameras with points;
//   assemble  k_cfit_assemble: one thread per entry (i <= j) of the 48 x 48 S and of g; it walks the records in record order,
//             subtracts Z_a^T Z_b and adds Jc^T Jc on the diagonal blocks.  The running sums live in global memory between passes of
//             the record workspace, so the result does not depend on the pass size;
//   solve     k_fit_solve<48> (ctag_fit_solve.h, the rig assembly's kernel): one block, at most 42 unknowns, the anchor's rows as
//             identity rows.
// The host decides (initial assembly, accept / reject, lambda, stop) between the launches.  FP64 VALU like the pose kernels.
// The pose block of a record is ctag_schur6.h's, the host side of a fit (timed state, call context, systems with their pass loop and
// solve, the accept / reject rule) is ctag_fit_host.h's.  This file keeps its kernels' walk and pass 2, the initial assembly of
// rule 2, the probe, and its round loop.
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

static_assert(sizeof(ctag_camera_fit_opts) == 40, "ctag_camera_fit_opts layout");
static_assert(sizeof(ctag_camera_fit_stat) == 64, "ctag_camera_fit_stat layout");
static_assert(sizeof(ctag_camera_fit_cam_stat) == 72, "ctag_camera_fit_cam_stat layout");

namespace ctag {

constexpr int kCfitGrid = 256;            // wavefronts of one k_cfit_record launch at most
constexpr int kCfitPassRecords = 512;     // observation records one pass of the workspace holds
constexpr int kCfitDoubles = 63;          // per camera slot of a record: Z (36), Jc^T Jc (21, upper triangle in row order), g (6)
constexpr int kCfitN = 6 * kMvCams;       // 48: row stride of S, delta and g
constexpr int kCfitMaxPts = CTAG_RIG_MAX_POINTS;

struct CfitLds {
    PoseCam cam[kMvCams];            // the camera table, once per block
    double R[kMvCams][9];
    double t[kMvCams][3];
    int32_t src[kCfitMaxPts];        // point i: its descriptor (point_desc, ctag_pose_dev.h)
    int16_t mdl[kCfitMaxPts];        // ... and its model index
    int32_t cstart[kMvCams + 1];     // camera c owns the points cstart[c] .. cstart[c + 1] - 1
};

// Observation records r0 .. r1-1 (indices into obs, which holds multi-view record indices): workspace slot r - r0 gets the 63 doubles
// of every camera with points, cmask[r] the mask of those cameras, flags[r] the record's state (kRec*).
__global__ __launch_bounds__(64) void k_cfit_record(MvResults res, int n_frames, const ctag_mv_pose_rec* __restrict__ recs, const int32_t* __restrict__ obs,
                                                    int r0, int r1, PoseModelDev model, MvCams cams, double* __restrict__ ws,
                                                    int32_t* __restrict__ cmask, int32_t* __restrict__ flags) {
    __shared__ CfitLds L;
    const int lane = threadIdx.x;
    for (int c = lane; c < kMvCams; c += 64) {
        L.cam[c] = cams.cam[c];
        for (int i = 0; i < 9; i++) L.R[c][i] = cams.R[c][i];
        for (int i = 0; i < 3; i++) L.t[c][i] = cams.t[c][i];
    }
    for (int r = r0 + (int)blockIdx.x; r < r1; r += gridDim.x) {
        const ctag_mv_pose_rec& P = recs[obs[r]];
        wave_sync();  // the previous record's LDS reads are done (and the cameras are in LDS)
        int n = 0;
        bool ok = P.status == CTAG_POSE_OK && P.frame >= 0 && P.frame < n_frames && model.n_models <= 32767;
        const int f = ok ? P.frame : 0;
        for (int c = 0; c < kMvCams; c++) {  // wave-uniform
            if (lane == 0) L.cstart[c] = n;
            const uint32_t* mask = P.member_mask[c];
            if (!ok || (mask[0] | mask[1] | mask[2] | mask[3]) == 0u) continue;
            if (c >= cams.n) {
                ok = false;
                break;
            }
            const ctag_frame_result& FR = res.p[c][f];
            if (FR.status != CTAG_OK) {
                ok = false;
                break;
            }
            const int nm = min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
            const ctag_feature_rec* F0 = FR.features;
            for (int k = 0; k < nm && ok; k++) {
                if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
                const int mi = model_lookup(model, FR.markers[k].marker_id);
                if (mi < 0) {
                    ok = false;
                    break;
                }
                const int base = n;
                int nl = 0;
                const int st = marker_points(FR, FR.markers[k], model.model_size, kPoseMaxPts, nl, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
                    if (lane < cnt && base + i0 + cnt <= kCfitMaxPts) {
                        L.src[base + i0 + lane] = point_desc((int)(&F - F0), lane, c, pos);
                        L.mdl[base + i0 + lane] = (int16_t)mi;
                    }
                });
                if (st != CTAG_POSE_OK || base + nl > kCfitMaxPts) {
                    ok = false;
                    break;
                }
                n += nl;
            }
        }
        if (lane == 0) L.cstart[kMvCams] = n;
        ok = ok && n == P.n_points && n >= 4;
        double x[6];
        ok = load_state6(P, x) && ok;
        wave_sync();
        if (!ok) {  // wave-uniform
            if (lane == 0) {
                flags[r] = kRecLeftOut;
                cmask[r] = 0;
            }
            continue;
        }
        double R[9], dR[27];
        ctl::angle_axis_rot(x, R, dR);
        // point i of the record: its residual and the rows of Jp; Q is the point in its camera's frame
        auto point = [&](int i, int& c, double* Q, double& q0, double& q1, double* j0, double* j1) {
            const int s = L.src[i];
            c = desc_cam(s);
            const float* __restrict__ corners = model.corners + (size_t)L.mdl[i] * model.model_size * 24;
            double xn, yn, ob[2], X[3];
            corner_point(L.cam[c], corners, res.p[c][f].features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, X);
            mv_point_residual(R, dR, x, L.cam[c], L.R[c], L.t[c], X, ob, q0, q1, j0, j1);
            const double* Rc = L.R[c];
            const double P0 = (R[0] * X[0] + R[1] * X[1] + R[2] * X[2]) + x[3];
            const double P1 = (R[3] * X[0] + R[4] * X[1] + R[5] * X[2]) + x[4];
            const double P2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + x[5];
            Q[0] = (Rc[0] * P0 + Rc[1] * P1 + Rc[2] * P2) + L.t[c][0];
            Q[1] = (Rc[3] * P0 + Rc[4] * P1 + Rc[5] * P2) + L.t[c][1];
            Q[2] = (Rc[6] * P0 + Rc[7] * P1 + Rc[8] * P2) + L.t[c][2];
        };
        // ---- pass 1: U and sum Jp^T r over the record's points
        double H[21], b[6];
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) b[a] = 0.0;
        for (int i = lane; i < n; i += 64) {
            int c;
            double Q[3], q0, q1, j0[6], j1[6];
            point(i, c, Q, q0, q1, j0, j1);
            gram6_add(j0, j1, H);
            grad6_add(j0, j1, q0, q1, b);
        }
        double Lc[36];
        const bool pd = pose_block6(H, b, Lc);  // the same in every lane; b is y from here on
        int present = 0;
        for (int c = 0; c < kMvCams; c++)
            if (L.cstart[c + 1] > L.cstart[c]) present |= 1 << c;
        if (lane == 0) {
            flags[r] = pd ? 0 : kRecSingular;
            cmask[r] = pd ? present : 0;
        }
        if (!pd) continue;
        // ---- pass 2: the 63 doubles of every camera with points
        double* W = ws + (size_t)(r - r0) * kMvCams * kCfitDoubles;
        for (int c = 0; c < kMvCams; c++) {
            if (!((present >> c) & 1)) continue;
            const int i0 = L.cstart[c], i1 = L.cstart[c + 1];
            const double fx = L.cam[c].fx, fy = L.cam[c].fy;
            double Z[36], A[21], gm[6];
#pragma unroll
            for (int e = 0; e < 36; e++) Z[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 21; e++) A[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) gm[e] = 0.0;
            for (int i = i0 + ((lane - i0) & 63); i < i1; i += 64) {  // the lane's own points (i = lane mod 64) inside the run
                int cc;
                double Q[3], q0, q1, j0[6], j1[6];
                point(i, cc, Q, q0, q1, j0, j1);
                // d residual / d Q = (a0, 0, -b0), (0, a1, -b1); Jc = (dr/dQ) [-[Q]x | I]: the rotation columns are Q x (dr/dQ)
                const double iz = 1.0 / Q[2];
                const double x0[3] = {fx * iz, 0.0, -(fx * Q[0] * iz * iz)};
                const double x1[3] = {0.0, fy * iz, -(fy * Q[1] * iz * iz)};
                double m0[6], m1[6];
                m0[0] = Q[1] * x0[2] - Q[2] * x0[1];
                m0[1] = Q[2] * x0[0] - Q[0] * x0[2];
                m0[2] = Q[0] * x0[1] - Q[1] * x0[0];
                m1[0] = Q[1] * x1[2] - Q[2] * x1[1];
                m1[1] = Q[2] * x1[0] - Q[0] * x1[2];
                m1[2] = Q[0] * x1[1] - Q[1] * x1[0];
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    m0[3 + m] = x0[m];
                    m1[3 + m] = x1[m];
                }
                int e = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int d = 0; d < 6; d++) {
                        Z[a * 6 + d] += j0[a] * m0[d];
                        Z[a * 6 + d] += j1[a] * m1[d];
                    }
#pragma unroll
                    for (int d = a; d < 6; d++) {
                        A[e] += m0[a] * m0[d];
                        A[e] += m1[a] * m1[d];
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
            for (int d = 0; d < 6; d++) {  // column d of Z <- L^-1 (column d), g_d -= Z_d . y
                double z[6];
#pragma unroll
                for (int a = 0; a < 6; a++) z[a] = Z[a * 6 + d];
                gm[d] -= forward6_dot(Lc, z, b);
#pragma unroll
                for (int a = 0; a < 6; a++) Z[a * 6 + d] = z[a];
            }
            if (lane == 0) {
                double* O = W + (size_t)c * kCfitDoubles;
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

// Adds records r0 .. r1-1 to S and g.  Thread t < 48 x 48: entry (i, j) = (t / 48, t % 48) of S, the threads with i <= j work and
// write both triangles; 48 x 48 <= t < 48 x 48 + 48: entry t - 48 x 48 of g.  Camera slot a owns rows 6a .. 6a + 5.
__global__ __launch_bounds__(256) void k_cfit_assemble(const double* __restrict__ ws, const int32_t* __restrict__ cmask, const int32_t* __restrict__ flags, int r0,
                                                       int r1, double* __restrict__ S, double* __restrict__ g) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    constexpr int NN = kCfitN * kCfitN;
    const int i = t < NN ? t / kCfitN : t - NN, j = t < NN ? t - i * kCfitN : 0;
    const bool is_s = t < NN && i <= j, is_g = t >= NN && t < NN + kCfitN;
    if (!is_s && !is_g) return;
    const int a = i / 6, p = i - 6 * a, bs = j / 6, q = j - 6 * bs;
    double* dst = is_s ? S + (size_t)i * kCfitN + j : g + i;
    double acc = *dst;
    int ea = 0;  // index of (p, q) in the upper triangle's row order
    if (is_s && a == bs) ea = p * 6 - p * (p - 1) / 2 + (q - p);
    const int need = is_g ? (1 << a) : ((1 << a) | (1 << bs));
    for (int r = r0; r < r1; r++) {
        if (flags[r] != 0 || (cmask[r] & need) != need) continue;
        const double* za = ws + ((size_t)(r - r0) * kMvCams + a) * kCfitDoubles;
        if (is_g) {
            acc += za[57 + p];
            continue;
        }
        const double* zb = ws + ((size_t)(r - r0) * kMvCams + bs) * kCfitDoubles;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += za[k * 6 + p] * zb[k * 6 + q];
        acc -= s;
        if (a == bs) acc += za[36 + ea];
    }
    *dst = acc;
    if (is_s && i != j) S[(size_t)j * kCfitN + i] = acc;
}

}  // namespace ctag

// =====================================================================================================
// host side: what the fits share is ctag_fit_host.h's (namespace ctag::fit)
// =====================================================================================================
namespace {

namespace fit = ctag::fit;

void mat_mul(const double* A, const double* B, double* C) {  // C = A B, 3x3 row-major, sums in index order
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

void mat_vec(const double* A, const double* v, double* o) {
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}

struct SetGuard {  // frees a camera set unless it is handed out
    ctag_camera_set* s = nullptr;
    ~SetGuard() { reset(nullptr); }
    void reset(ctag_camera_set* n) {
        if (s) ctag_camera_set_free(s);
        s = n;
    }
};

// The device side of one call: the one system (group 0), the record workspace and the cameras' detection records.
struct CfitWork : fit::Systems {
    fit::Call c;
    ctag::MvResults res{};
    int32_t n_slots = 0, drop = 0;  // cameras of the set; the anchor's slot
    ctag::DevBuf<int32_t> d_n_slots, d_drop, d_cmask;
    ctag::DevBuf<double> d_ws;

    int setup(int pass_records) {
        const int rc = Systems::setup(c, 1, ctag::kCfitN, pass_records, ctag::kCfitPassRecords);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_cmask.grow((size_t)std::max(R, 1)));
        FIT_HIP(d_ws.grow((size_t)pass * ctag::kMvCams * ctag::kCfitDoubles));
        FIT_HIP(d_n_slots.grow(1));
        FIT_HIP(d_drop.grow(1));
        FIT_HIP(hipMemcpyAsync(d_n_slots.p, &n_slots, sizeof(int32_t), hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipMemcpyAsync(d_drop.p, &drop, sizeof(int32_t), hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipStreamSynchronize(c.s));  // n_slots and drop are read from this object
        return CTAG_OK;
    }

    // S and g at (cams, recs_dev); slot 2 times the record and the assemble kernel together.  Waits.
    int build_system(const ctag_model* model, const ctag_camera_set* cams, const ctag_mv_pose_rec* recs_dev) {
        const ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
        constexpr int kThreads = ctag::kCfitN * ctag::kCfitN + ctag::kCfitN;
        return build(c, [&](int r0, int r1) {
            if (c.mark(0) != CTAG_OK) return CTAG_ERR_HIP;
            hipLaunchKernelGGL(ctag::k_cfit_record, dim3(std::min(r1 - r0, ctag::kCfitGrid)), dim3(64), 0, c.s, res, c.n_frames, recs_dev, d_obs.p, r0, r1, md,
                               cams->dev, d_ws.p, d_cmask.p, d_flags.p);
            hipLaunchKernelGGL(ctag::k_cfit_assemble, dim3((kThreads + 255) / 256), dim3(256), 0, c.s, d_ws.p, d_cmask.p, d_flags.p, r0, r1, d_S.p, d_g.p);
            if (fit::launched() != CTAG_OK || c.mark(1) != CTAG_OK || c.reached(1) != CTAG_OK) return CTAG_ERR_HIP;
            c.add_ms(2, 0);
            return CTAG_OK;
        });
    }

    int solve(const std::vector<double>& lambda, const std::vector<int32_t>& active, int bad_flags, std::vector<double>& delta, std::vector<int32_t>& bad) {
        return Systems::solve(c, lambda, active, bad_flags, delta, bad, [&]() {
            hipLaunchKernelGGL(ctag::k_fit_solve<ctag::kCfitN>, dim3(1), dim3(ctag::kFitSolveThreads), 0, c.s, d_S.p, d_g.p, d_n_slots.p, d_drop.p, d_lambda.p,
                               d_active.p, d_delta.p, d_bad.p);
        });
    }
};

int cfit_opts(const ctag_camera_fit_opts* o, ctag_camera_fit_opts& r) {
    ctag_camera_fit_opts_default(&r);
    if (o) r = *o;
    if (r.max_rounds < 0 || r.min_items < 1 || r.min_points < 1) return CTAG_ERR_ARG;
    for (double v : {r.lambda0, r.lambda_max, r.rel_tol})
        if (!std::isfinite(v) || !(v > 0.0)) return CTAG_ERR_ARG;
    return CTAG_OK;
}

}  // namespace

namespace ctag {

int cfit_record_grid() { return kCfitGrid; }
int cfit_pass_records() { return kCfitPassRecords; }

int cfit_probe_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_mv_pose_rec* recs, const ctag_model* model_c,
                      const ctag_rigs* rigs, const ctag_camera_set* cams, int anchor, double lambda, int pass_records, double* S, double* g, double* delta,
                      int32_t* n_unknowns, int32_t* bad_pivot) {
    if (!h || !results || n_frames < 1 || !recs || !model_c || !rigs || !cams || !S || !g || !delta || !n_unknowns || !bad_pivot) return CTAG_ERR_ARG;
    const int nc = cams->dev.n;
    if (rigs->n_models != model_c->n_models || nc < 2 || anchor < 0 || anchor >= nc || !std::isfinite(lambda)) return CTAG_ERR_ARG;
    if ((long long)n_frames * rigs->n_rigs > (1ll << 28) || (long long)n_frames * nc > (1ll << 24)) return CTAG_ERR_LIMIT;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    CfitWork w;
    int rc = w.c.prepare(h, kCamFitState, nullptr, n_frames, &cams->cameras[0]);
    if (rc != CTAG_OK) return rc;
    if (model_to_device(model, handle_device(h)) != CTAG_OK) return CTAG_ERR_HIP;
    const size_t n_items = (size_t)n_frames * rigs->n_rigs;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<ctag_mv_pose_rec> d_recs;
    FIT_HIP(d_res.grow((size_t)n_frames * nc));
    FIT_HIP(d_recs.grow(n_items));
    FIT_HIP(hipMemcpyAsync(d_res.p, results, sizeof(ctag_frame_result) * (size_t)n_frames * nc, hipMemcpyHostToDevice, w.c.s));
    FIT_HIP(hipMemcpyAsync(d_recs.p, recs, sizeof(ctag_mv_pose_rec) * n_items, hipMemcpyHostToDevice, w.c.s));
    for (int c = 0; c < kMvCams; c++) w.res.p[c] = c < nc ? d_res.p + (size_t)c * n_frames : nullptr;
    for (size_t i = 0; i < n_items; i++)
        if (recs[i].status == CTAG_POSE_OK && recs[i].n_cameras >= 2) {
            w.obs.push_back((int32_t)i);
            w.rec_group.push_back(0);
        }
    if (w.obs.empty()) return CTAG_ERR_ARG;
    w.n_slots = nc;
    w.drop = anchor;
    rc = w.setup(pass_records);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(model, cams, d_recs.p);
    if (rc != CTAG_OK) return rc;
    std::vector<double> lam(1, lambda), d;
    std::vector<int32_t> active(1, 1), bad;
    rc = w.solve(lam, active, kRecSingular, d, bad);  // a caller's record may be left out; that does not make the system bad here
    if (rc != CTAG_OK) return rc;
    const int N = 6 * nc;
    std::vector<double> Sf((size_t)kCfitN * kCfitN), gf(kCfitN);
    FIT_HIP(hipMemcpy(Sf.data(), w.d_S.p, sizeof(double) * Sf.size(), hipMemcpyDeviceToHost));
    FIT_HIP(hipMemcpy(gf.data(), w.d_g.p, sizeof(double) * kCfitN, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; i++) {
        for (int j = 0; j < N; j++) S[(size_t)i * N + j] = Sf[(size_t)i * kCfitN + j];
        g[i] = gf[i];
        delta[i] = d[i];
    }
    *n_unknowns = N;
    *bad_pivot = bad[0];
    return CTAG_OK;
}

}  // namespace ctag

extern "C" {

void ctag_camera_fit_opts_default(ctag_camera_fit_opts* o) {
    if (!o) return;
    o->max_rounds = 30;
    o->min_items = 2;
    o->min_points = 8;
    o->reserved = 0;
    o->lambda0 = 1e-3;
    o->lambda_max = 1e6;
    o->rel_tol = 6.14e-13;  // 4 x 1.535e-13: what a one-ulp change of a camera pose does to the cost through the inner solves
}

int ctag_camera_fit_last_ms(ctag_handle* h, float* out4) { return fit::last_ms(h, ctag::kCamFitState, out4); }  // per-camera rig pose, mv pose, record + assemble, solve

int ctag_camera_fit_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_cameras, int n_frames, const ctag_model* model_c,
                           const ctag_rigs* rigs, const ctag_camera* cameras, const ctag_camera_fit_opts* opts_in, ctag_camera_set** out,
                           ctag_camera_fit_stat* stat, ctag_camera_fit_cam_stat* cam_stats) {
    if (out) *out = nullptr;  // on every return but a full set
    if (!h || !results_dev || n_frames < 1 || !model_c || !rigs || !cameras || !out || !stat || !cam_stats) return CTAG_ERR_ARG;
    if (n_cameras < 2 || n_cameras > CTAG_MV_MAX_CAMERAS) return CTAG_ERR_ARG;
    for (int c = 0; c < n_cameras; c++)
        if (!results_dev[c]) return CTAG_ERR_ARG;
    ctag_camera_fit_opts opts;
    if (cfit_opts(opts_in, opts) != CTAG_OK) return CTAG_ERR_ARG;
    if (model_c->model_size != ctag::handle_dict_cols(h) || model_c->model_size > CTAG_MAX_CODE_POS) return CTAG_ERR_ARG;
    if (rigs->n_models != model_c->n_models) return CTAG_ERR_ARG;
    for (int c = 0; c < n_cameras; c++)
        if (!ctag::camera_ok(&cameras[c])) return CTAG_ERR_UNSUPPORTED;
    const int ng = rigs->n_rigs, nc = n_cameras;
    if ((long long)n_frames * CTAG_MAX_MARKERS > (1ll << 30) || (long long)n_frames * ng > (1ll << 28)) return CTAG_ERR_LIMIT;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    CfitWork w;
    int rc = w.c.prepare(h, ctag::kCamFitState, nullptr, n_frames, &cameras[0]);
    if (rc != CTAG_OK) return rc;
    std::memset(stat, 0, sizeof(*stat));
    stat->status = CTAG_POSE_NOT_SEEN;
    stat->anchor = -1;
    stat->n_unplaced = nc;
    stat->lambda = opts.lambda0;
    for (int c = 0; c < nc; c++) {
        std::memset(&cam_stats[c], 0, sizeof(cam_stats[c]));
        cam_stats[c].status = CTAG_POSE_NOT_SEEN;
        cam_stats[c].parent = -1;
    }
    const size_t n_items = (size_t)n_frames * ng;

    // ---- rule 1: every camera's own rig poses
    std::vector<std::vector<ctag_rig_pose_rec>> rp(nc);
    {
        ctag::DevBuf<ctag_rig_pose_rec> d_rp;
        FIT_HIP(d_rp.grow(n_items));
        for (int c = 0; c < nc; c++) {
            rc = w.c.pose_pass(0, [&]() { return ctag_rig_pose_batch_device(h, results_dev[c], n_frames, model, rigs, &cameras[c], d_rp.p); }, d_rp.p, n_items, rp[c]);
            if (rc != CTAG_OK) return rc;
        }
    }
    auto counted = [&](int c, size_t i) { return rp[c][i].status == CTAG_POSE_OK && rp[c][i].n_points >= opts.min_points; };

    // ---- rule 2: the initial assembly
    std::vector<int> cnt((size_t)nc * nc, 0);
    for (size_t i = 0; i < n_items; i++)
        for (int a = 0; a < nc; a++) {
            if (!counted(a, i)) continue;
            for (int b = a + 1; b < nc; b++)
                if (counted(b, i)) {
                    cnt[(size_t)a * nc + b]++;
                    cnt[(size_t)b * nc + a]++;
                }
        }
    int anchor = -1;
    for (int a = 0; a < nc && anchor < 0; a++)
        for (int b = 0; b < nc; b++)
            if (cnt[(size_t)a * nc + b] >= opts.min_items) {
                anchor = a;
                break;
            }
    if (anchor < 0) return CTAG_OK;
    std::vector<ctag_camera_pose> pose(nc);  // the accepted state: X_c = R(rvec) X_anchor + tvec
    for (auto& p : pose) std::memset(&p, 0, sizeof(p));
    std::vector<uint8_t> in_tree(nc, 0);
    in_tree[anchor] = 1;
    int n_placed = 1;
    for (;;) {
        int best = opts.min_items - 1, ba = -1, bb = -1;
        for (int b = 0; b < nc; b++) {  // ascending b, then ascending a: the first of equal counts stays
            if (in_tree[b]) continue;
            for (int a = 0; a < nc; a++)
                if (in_tree[a] && cnt[(size_t)a * nc + b] > best) {
                    best = cnt[(size_t)a * nc + b];
                    ba = a;
                    bb = b;
                }
        }
        if (bb < 0) break;
        double sumR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < n_items; i++) {
            if (!counted(ba, i) || !counted(bb, i)) continue;
            double Ra[9], Rb[9], RaT[9], Q[9];
            ctl::angle_axis_rot(rp[ba][i].rvec, Ra, nullptr);
            ctl::angle_axis_rot(rp[bb][i].rvec, Rb, nullptr);
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) RaT[r * 3 + k] = Ra[k * 3 + r];
            mat_mul(Rb, RaT, Q);
            for (int k = 0; k < 9; k++) sumR[k] += Q[k];
        }
        double ER[9], Et[3], sv[3], sumt[3] = {0, 0, 0};
        fit::nearest_rotation(sumR, ER, sv);
        for (size_t i = 0; i < n_items; i++) {
            if (!counted(ba, i) || !counted(bb, i)) continue;
            double e[3];
            mat_vec(ER, rp[ba][i].tvec, e);
            for (int k = 0; k < 3; k++) sumt[k] += rp[bb][i].tvec[k] - e[k];
        }
        for (int k = 0; k < 3; k++) Et[k] = sumt[k] / (double)best;
        // T_b = E o T_a
        double Ra[9], Rb[9], e[3];
        ctl::angle_axis_rot(pose[ba].rvec, Ra, nullptr);
        mat_mul(ER, Ra, Rb);
        ctl::rodrigues_from_matrix(Rb, pose[bb].rvec);
        mat_vec(ER, pose[ba].tvec, e);
        for (int k = 0; k < 3; k++) pose[bb].tvec[k] = e[k] + Et[k];
        in_tree[bb] = 1;
        n_placed++;
        cam_stats[bb].parent = ba;
        cam_stats[bb].n_items_with_parent = best;
    }
    std::vector<int> placed;  // slot -> camera
    for (int c = 0; c < nc; c++)
        if (in_tree[c]) {
            if (c == anchor) w.drop = (int32_t)placed.size();
            placed.push_back(c);
            cam_stats[c].status = CTAG_POSE_OK;
        }
    const int np = n_placed;
    w.n_slots = np;
    stat->status = CTAG_POSE_OK;
    stat->anchor = anchor;
    stat->n_placed = np;
    stat->n_unplaced = nc - np;
    const ctag_frame_result* ptrs[CTAG_MV_MAX_CAMERAS];
    ctag_camera cams_placed[CTAG_MV_MAX_CAMERAS];
    for (int k = 0; k < CTAG_MV_MAX_CAMERAS; k++) {
        ptrs[k] = k < np ? results_dev[placed[k]] : nullptr;
        w.res.p[k] = ptrs[k];
        if (k < np) cams_placed[k] = cameras[placed[k]];
    }
    auto make_set = [&](const std::vector<ctag_camera_pose>& state, ctag_camera_set** s) {
        ctag_camera_pose pp[CTAG_MV_MAX_CAMERAS];
        for (int k = 0; k < np; k++) pp[k] = state[placed[k]];
        return ctag_camera_set_create(cams_placed, pp, np, s);
    };
    auto report = [&](const std::vector<ctag_camera_pose>& state) {
        for (int k = 0; k < np; k++) cam_stats[placed[k]].pose = state[placed[k]];
    };
    report(pose);

    // ---- rule 3: the observation set under the initial set
    SetGuard cur, tri;
    rc = make_set(pose, &cur.s);
    if (rc != CTAG_OK) return rc;
    ctag::DevBuf<ctag_mv_pose_rec> d_recs;
    FIT_HIP(d_recs.grow(n_items));
    std::vector<ctag_mv_pose_rec> acc, trial;
    auto mv_pass = [&](const ctag_camera_set* s, std::vector<ctag_mv_pose_rec>& host) {
        return w.c.pose_pass(1, [&]() { return ctag_mv_rig_pose_batch_device(h, ptrs, n_frames, model, rigs, s, d_recs.p); }, d_recs.p, n_items, host);
    };
    rc = mv_pass(cur.s, acc);
    if (rc != CTAG_OK) return rc;
    for (size_t i = 0; i < n_items; i++)
        if (acc[i].status == CTAG_POSE_OK && acc[i].n_cameras >= 2) {
            w.obs.push_back((int32_t)i);
            w.rec_group.push_back(0);
        }
    rc = w.setup(0);
    if (rc != CTAG_OK) return rc;
    const int R = w.R;
    fit::Lm lm;
    lm.start(1, opts.lambda0);
    std::vector<uint8_t> ok_cur;
    w.costs_of(acc, nullptr, lm.cost, ok_cur);
    for (int r = 0; r < R; r++) {
        const ctag_mv_pose_rec& p = acc[w.obs[r]];
        stat->n_records++;
        stat->n_points += p.n_points;
        for (int k = 0; k < np; k++)
            if (p.points_of_camera[k] > 0) {
                cam_stats[placed[k]].n_records++;
                cam_stats[placed[k]].n_points += p.points_of_camera[k];
            }
    }
    stat->cost_init = stat->cost = lm.cost[0];
    if (R > 0 && np > 1 && opts.max_rounds > 0) lm.active[0] = 1;

    // ---- rule 4: the rounds.  pose / cur / acc are the accepted state, tri / trial the trial of a round
    std::vector<ctag_camera_pose> pose_t(nc);
    bool need_system = true;
    std::vector<double> delta, cost_trial(1, 0.0);
    std::vector<uint8_t> ok_trial(1, 0);
    std::vector<int32_t> bad;
    while (lm.any_active()) {
        if (need_system) {
            FIT_HIP(hipMemcpyAsync(d_recs.p, acc.data(), sizeof(ctag_mv_pose_rec) * n_items, hipMemcpyHostToDevice, w.c.s));
            rc = w.build_system(model, cur.s, d_recs.p);
            if (rc != CTAG_OK) return rc;
            need_system = false;
        }
        // every observation record was solved by k_mv_solve on this state, so one that is flagged at all makes the system bad
        rc = w.solve(lm.lambda, lm.active, ~0, delta, bad);
        if (rc != CTAG_OK) return rc;
        bool usable = !bad[0];
        pose_t = pose;
        for (int k = 0; k < np && usable; k++) {  // Rc <- Exp(w) Rc, tc <- Exp(w) tc + v for the cameras that move
            const int c = placed[k];
            if (c == anchor) continue;
            const double* d = &delta[6 * k];
            for (int i = 0; i < 6; i++) usable = usable && std::isfinite(d[i]);
            if (!usable) break;
            double E[9], Rc[9], Rn[9], e[3];
            ctl::angle_axis_rot(d, E, nullptr);
            ctl::angle_axis_rot(pose[c].rvec, Rc, nullptr);
            mat_mul(E, Rc, Rn);
            ctl::rodrigues_from_matrix(Rn, pose_t[c].rvec);
            mat_vec(E, pose[c].tvec, e);
            for (int i = 0; i < 3; i++) pose_t[c].tvec[i] = e[i] + d[3 + i];
            for (int i = 0; i < 3; i++) usable = usable && std::isfinite(pose_t[c].rvec[i]) && std::isfinite(pose_t[c].tvec[i]);
        }
        if (usable) {
            tri.reset(nullptr);
            rc = make_set(pose_t, &tri.s);
            if (rc != CTAG_OK) return rc;
            rc = mv_pass(tri.s, trial);
            if (rc != CTAG_OK) return rc;
            w.costs_of(trial, nullptr, cost_trial, ok_trial);
            usable = ok_trial[0] != 0;
        }
        if (!lm.decide(0, usable, cost_trial[0], opts)) continue;
        pose = pose_t;
        std::swap(cur.s, tri.s);
        w.take_records(0, trial, acc);
        need_system = true;
    }
    report(pose);
    stat->rounds = lm.rounds[0];
    stat->cost = lm.cost[0];
    stat->lambda = lm.lambda[0];
    stat->rms_px = stat->n_points > 0 ? std::sqrt(2.0 * lm.cost[0] / (double)stat->n_points) : 0.0;
    if (np == nc) {
        *out = cur.s;
        cur.s = nullptr;
    }
    return CTAG_OK;
}

int ctag_camera_fit(ctag_handle* h, const ctag_frame_result* results, int n_cameras, int n_frames, const ctag_model* model, const ctag_rigs* rigs,
                    const ctag_camera* cameras, const ctag_camera_fit_opts* opts, ctag_camera_set** out, ctag_camera_fit_stat* stat,
                    ctag_camera_fit_cam_stat* cam_stats) {
    if (out) *out = nullptr;
    if (!h || !results || n_frames < 1 || !model || !rigs || !cameras || !out || !stat || !cam_stats) return CTAG_ERR_ARG;
    if (n_cameras < 2 || n_cameras > CTAG_MV_MAX_CAMERAS) return CTAG_ERR_ARG;
    if ((long long)n_frames * n_cameras > (1ll << 24)) return CTAG_ERR_LIMIT;
    return fit::with_results_on_device(h, results, n_frames * n_cameras, [&](const ctag_frame_result* results_dev) {
        const ctag_frame_result* ptrs[CTAG_MV_MAX_CAMERAS];
        for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) ptrs[c] = c < n_cameras ? results_dev + (size_t)c * n_frames : nullptr;
        return ctag_camera_fit_device(h, ptrs, n_cameras, n_frames, model, rigs, cameras, opts, out, stat, cam_stats);
    });
}

}  // extern "C"
