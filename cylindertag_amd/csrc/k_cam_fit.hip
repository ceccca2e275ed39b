// k_cam_fit.hip -- the poses of the cameras of a set in the frame of one of them, from the detection records of instants that two or
// more of them see together, on the device.  The semantics are stated in include/ctag_pose.h (camera set fit, rules 1-6).
//
// Mapping.  The reprojection problem over camera poses and per-instant rig poses separates: given the camera
// poses an instant's rig pose is the solve k_mv_solve already does, so a round is
//   pose      ctag_mv_rig_pose_batch_device under the trial camera set (k_mv_pose.hip, untouched);
//   record    k_cfit_record: one wavefront per observation record, grid-stride.  The walk is k_mv_count's / k_mv_solve's order: camera,
//             then fit_member_walk (ctag_pose_dev.h) over member_mask[c]; corner_point and mv_point_residual are the pose kernels',
//             every camera's pixels undistorted with its own coefficients.  Lane l owns the points l, l + 64, ... of the record.
//             Pass 1: the 21 entries of U = sum Jp^T Jp and the 6 of sum Jp^T r over all points, pose_block6 (ctag_schur6.h).  Pass 2,
//             camera by camera: a camera's points are one contiguous run, so the 36 + 21 + 6 sums of Jp^T Jc, Jc^T Jc and Jc^T r over
//             it are wave sums in which the lanes without a point of the run add zeros; then Z = L^-1 (Jp^T Jc) and
//             g = Jc^T r - Z^T y: the slot block of ctag_schur6.h, 63 doubles per camera slot, 8 slots, plus the record's mask of
//             cameras with points;
//   assemble  k_fit_assemble<48> (ctag_fit_solve.h, the rig assembly's kernel) with CfitSlotOf: one thread per entry (i <= j) of the
//             48 x 48 S and of g; it walks the records in record order, subtracts Z_a^T Z_b and adds Jc^T Jc on the diagonal blocks.
//             The running sums live in global memory between passes of the record workspace, so the result does not depend on the
//             pass size;
//   solve     k_fit_solve<48> (ctag_fit_solve.h, the rig assembly's kernel): one block, at most 42 unknowns, the anchor's rows as
//             identity rows.
// The host decides (initial assembly, accept / reject, lambda, stop) between the launches.  FP64 VALU like the pose kernels.
// The pose block and the slot block of a record are ctag_schur6.h's, the host side of a fit (timed state, call context, the slot
// systems with their pass loop, solve and probe hand-out, the co-visibility tree of rule 2, the accept / reject rule) is
// ctag_fit_host.h's.  This file keeps its record kernel with its point evaluation and its lane-to-point assignment, the counts and
// the edge of rule 2's tree, and its round loop.
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
constexpr int kCfitN = 6 * kMvCams;       // 48: row stride of S, delta and g

struct CfitLds {
    PoseCam cam[kMvCams];            // the camera table, once per block
    double R[kMvCams][9];
    double t[kMvCams][3];
    int32_t src[kFitMaxPts];        // point i: its descriptor (point_desc, ctag_pose_dev.h)
    int16_t mdl[kFitMaxPts];        // ... and its model index
    int32_t cstart[kMvCams + 1];     // camera c owns the points cstart[c] .. cstart[c + 1] - 1
};

// Observation records r0 .. r1-1 (indices into obs, which holds multi-view record indices): workspace slot r - r0 gets the slot block
// (ctag_schur6.h) of every camera with points, cmask[r] the mask of those cameras, flags[r] the record's state (kRec*).
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
            ok = FR.status == CTAG_OK && fit_member_walk(FR, mask, model, lane, c, n, [](int, int) { return true; }, [&](int i, int32_t desc, int mi) {
                     L.src[i] = desc;
                     L.mdl[i] = (int16_t)mi;
                 });
            if (!ok) break;
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
        // ---- pass 2: the slot block of every camera with points, Jc = (dr/dQ) [-[Q]x | I]
        double* W = ws + (size_t)(r - r0) * kMvCams * kSlotDoubles;
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
            // the lane's own points (i = lane mod 64) inside the run: the same lanes as in pass 1, they decide the order of the wave sums
            for (int i = i0 + ((lane - i0) & 63); i < i1; i += 64) {
                int cc;
                double Q[3], q0, q1, j0[6], j1[6], m0[6], m1[6];
                point(i, cc, Q, q0, q1, j0, j1);
                // d residual / d Q = (a0, 0, -b0), (0, a1, -b1)
                const double iz = 1.0 / Q[2];
                const double x0[3] = {fx * iz, 0.0, -(fx * Q[0] * iz * iz)};
                const double x1[3] = {0.0, fy * iz, -(fy * Q[1] * iz * iz)};
                slot_rows(Q, x0, x1, m0, m1);
                cross6_add(j0, j1, m0, m1, Z);
                gram6_add(m0, m1, A);
                grad6_add(m0, m1, q0, q1, gm);
            }
            slot_finish(Z, A, gm, Lc, b, lane, W + (size_t)c * kSlotDoubles);
        }
    }
}

// k_fit_assemble's SlotOf: one group; a camera's slot block lies at the slot itself, when the camera has points in the record
struct CfitSlotOf {
    const int32_t* cmask;
    __device__ int group() const { return 0; }
    __device__ bool operator()(int r, int a, int b, int& ka, int& kb) const {
        const int need = (1 << a) | (1 << b);
        ka = a;
        kb = b;
        return (cmask[r] & need) == need;
    }
};

}  // namespace ctag

// =====================================================================================================
// host side: what the fits share is ctag_fit_host.h's (namespace ctag::fit)
// =====================================================================================================
namespace {

namespace fit = ctag::fit;

struct SetGuard {  // frees a camera set unless it is handed out
    ctag_camera_set* s = nullptr;
    ~SetGuard() { reset(nullptr); }
    void reset(ctag_camera_set* n) {
        if (s) ctag_camera_set_free(s);
        s = n;
    }
};

// The device side of one call: the one system (group 0: its slots are the placed cameras, the anchor's dropped), the record workspace
// and the cameras' detection records.
struct CfitWork : fit::SlotSystems<ctag::kCfitN> {
    ctag::MvResults res{};
    ctag::DevBuf<int32_t> d_cmask;

    int setup(int pass_records) {
        const int rc = SlotSystems::setup(pass_records, ctag::kCfitPassRecords);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_cmask.grow((size_t)std::max(R, 1)));
        return CTAG_OK;
    }

    // S and g at (cams, recs_dev).  Waits.
    int build_system(const ctag_model* model, const ctag_camera_set* cams, const ctag_mv_pose_rec* recs_dev) {
        const ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
        return build_timed(c, [&](int r0, int r1) {
            hipLaunchKernelGGL(ctag::k_cfit_record, dim3(std::min(r1 - r0, ctag::kCfitGrid)), dim3(64), 0, c.s, res, c.n_frames, recs_dev, d_obs.p, r0, r1, md,
                               cams->dev, d_ws.p, d_cmask.p, d_flags.p);
            assemble(ctag::CfitSlotOf{d_cmask.p}, r0, r1);
        });
    }
};

int cfit_opts(const ctag_camera_fit_opts* o, ctag_camera_fit_opts& r) {
    ctag_camera_fit_opts_default(&r);
    if (o) r = *o;
    return r.max_rounds >= 0 && r.min_items >= 1 && r.min_points >= 1 && fit::lm_opts_ok(r) ? CTAG_OK : CTAG_ERR_ARG;
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
    w.n_slots.assign(1, nc);
    w.drop.assign(1, anchor);
    rc = w.setup(pass_records);
    if (rc != CTAG_OK) return rc;
    rc = w.build_system(model, cams, d_recs.p);
    if (rc != CTAG_OK) return rc;
    return w.probe(0, lambda, S, g, delta, n_unknowns, bad_pivot);
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
    std::vector<ctag_camera_pose> pose(nc);  // the accepted state: X_c = R(rvec) X_anchor + tvec
    for (auto& p : pose) std::memset(&p, 0, sizeof(p));
    std::vector<uint8_t> in_tree;
    const int anchor = fit::covisibility_tree(nc, cnt, opts.min_items, in_tree, [&](int ba, int bb, int best) {
        double sumR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < n_items; i++) {
            if (!counted(ba, i) || !counted(bb, i)) continue;
            double Ra[9], Rb[9], RaT[9], Q[9];
            ctl::angle_axis_rot(rp[ba][i].rvec, Ra, nullptr);
            ctl::angle_axis_rot(rp[bb][i].rvec, Rb, nullptr);
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) RaT[r * 3 + k] = Ra[k * 3 + r];
            fit::mat_mul(Rb, RaT, Q);
            for (int k = 0; k < 9; k++) sumR[k] += Q[k];
        }
        double ER[9], Et[3], sv[3], sumt[3] = {0, 0, 0};
        fit::nearest_rotation(sumR, ER, sv);
        for (size_t i = 0; i < n_items; i++) {
            if (!counted(ba, i) || !counted(bb, i)) continue;
            double e[3];
            fit::mat_vec(ER, rp[ba][i].tvec, e);
            for (int k = 0; k < 3; k++) sumt[k] += rp[bb][i].tvec[k] - e[k];
        }
        for (int k = 0; k < 3; k++) Et[k] = sumt[k] / (double)best;
        // T_b = E o T_a
        double Ra[9], Rb[9], e[3];
        ctl::angle_axis_rot(pose[ba].rvec, Ra, nullptr);
        fit::mat_mul(ER, Ra, Rb);
        ctl::rodrigues_from_matrix(Rb, pose[bb].rvec);
        fit::mat_vec(ER, pose[ba].tvec, e);
        for (int k = 0; k < 3; k++) pose[bb].tvec[k] = e[k] + Et[k];
        cam_stats[bb].parent = ba;
        cam_stats[bb].n_items_with_parent = best;
    });
    if (anchor < 0) return CTAG_OK;
    w.n_slots.assign(1, 0);
    w.drop.assign(1, 0);
    std::vector<int> placed;  // slot -> camera
    for (int c = 0; c < nc; c++)
        if (in_tree[c]) {
            if (c == anchor) w.drop[0] = (int32_t)placed.size();
            placed.push_back(c);
            cam_stats[c].status = CTAG_POSE_OK;
        }
    const int np = w.n_slots[0] = (int)placed.size();
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
            fit::mat_mul(E, Rc, Rn);
            ctl::rodrigues_from_matrix(Rn, pose_t[c].rvec);
            fit::mat_vec(E, pose[c].tvec, e);
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
