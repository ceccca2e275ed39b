// k_rig_fit.hip -- assembly of the models of a rig into one common frame from the detection records of frames that show two or
// more of its markers together, on the device.  The semantics are stated in include/ctag_pose.h (rig assembly, rules 1-7).
//
// Mapping.  The reprojection problem over member transforms and per-frame rig poses separates: given the
// transforms a frame's rig pose is the solve k_rig_pose already does, so a round is
//   pose      ctag_rig_pose_batch_device on the call's working copy of the model (k_rig_pose.hip, untouched);
//   record    k_rfit_record: one wavefront per observation record, grid-stride.  The member walk is fit_member_walk (ctag_pose_dev.h:
//             marker_points over the record's member_mask), corner_point and point_residual are the pose
//             kernels'.  A member's points are one contiguous run of the record, lane l takes the points l, l + 64, ... of the run.
//             Pass 1: the 21 entries of U = sum Jp^T Jp and the 6 of sum Jp^T r over all points through wave_sum_f64, every lane
//             factors U = L L^T.  Pass 2, member by member: the slot block (ctag_schur6.h) -- the 36 + 21 + 6 sums of Jp^T Jm, Jm^T Jm
//             and Jm^T r over the member's run through wave_sum_f64 (lanes without a point of the run add zeros: masked wave sums),
//             then Z = L^-1 (Jp^T Jm) and g = Jm^T r - Z^T y: 63 doubles per member slot -- plus the record's model-slot -> member
//             table (int8, -1 where absent);
//   assemble  k_fit_assemble<96> (ctag_fit_solve.h) with RfitSlotOf: for rig g one thread per entry (i <= j) of its 96 x 96 S; it walks
//             the records in record order (other rigs' records skipped by a block-uniform branch), subtracts Z_a^T Z_b and adds
//             Jm^T Jm on the diagonal blocks; g the same way.  The running sums live in global memory between passes of the record
//             workspace, so the result does not depend on the pass size;
//   solve     k_fit_solve<96> (ctag_fit_solve.h): one block per rig, the damped system (S + lambda diag S) as a packed lower triangle in LDS (at most
//             96 x 97 / 2 doubles, 37 KB), right-looking Cholesky, the dropped rows (the anchor's) as identity rows with a zero
//             right-hand side, the two triangular solves, delta and a flag for a pivot that is not positive.
// The host decides (initial assembly, accept / reject, lambda, stop) per rig between the launches.  FP64 VALU like the pose kernels;
// the largest system is 90 x 90, nothing here is MFMA-shaped.
//
// What the assembly shares with the other fits is not here: the pose block of a record (pass 1, a column through L^-1, the point
// Jacobian) and the slot block are ctag_schur6.h's, the member walk, the point descriptor and load_state6 are ctag_pose_dev.h's, the
// assemble and the solve kernel are ctag_fit_solve.h's, and the host side of a fit -- timed state, call context, working model, the
// slot systems with their pass loop, solve and probe hand-out, the co-visibility tree of rule 2, the accept / reject rule -- is
// ctag_fit_host.h's.  This file keeps its record kernel with its tables and its lane-to-point assignment, the counts and the edge
// of rule 2's tree, apply_rigid, report_transforms, and its round loop.
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
constexpr int kRfitN = 6 * kRfitSlots;    // 96: row stride of S, delta and g
// flags of a record: kRecLeftOut (it does not describe its detection record: never for records k_rig_solve wrote) and kRecSingular

struct RfitLds {
    int32_t src[kFitMaxPts];         // point i: its descriptor (point_desc, ctag_pose_dev.h; camera 0)
    int32_t mstart[kRfitSlots + 1];  // member k owns the points mstart[k] .. mstart[k + 1] - 1
    int32_t mmodel[kRfitSlots];      // its model index
    int8_t table[kRfitSlots];        // model slot of the rig -> member, -1 where absent
};

// Observation records r0 .. r1-1 (indices into obs, which holds rig-pose record indices): workspace slot r - r0 gets the slot block
// (ctag_schur6.h) of every member, table row r the model-slot -> member map, flags[r] the record's state.
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
        bool ok = P.status == CTAG_POSE_OK && P.frame >= 0 && P.frame < n_frames && res[P.frame].status == CTAG_OK;
        ok = ok && fit_member_walk(res[P.frame], P.member_mask, model, lane, 0, n,
                                   // a member: its model has a slot in a system, and the record has room for it.  It is entered here, before
                                   // its points are walked; should they turn the record down, the record is left out and the entry is never read
                                   [&](int mi, int base) {
                                       if (slot_of_model[mi] < 0 || nmem >= kRfitSlots) return false;
                                       if (lane == 0) {
                                           L.mstart[nmem] = base;
                                           L.mmodel[nmem] = mi;
                                           L.table[slot_of_model[mi]] = (int8_t)nmem;
                                       }
                                       nmem++;
                                       return true;
                                   },
                                   [&](int i, int32_t desc, int) { L.src[i] = desc; });
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
        // point i of member k's run: its residual, the rows of Jp, and Y, the model point
        auto point = [&](int k, int i, double* Y, double& q0, double& q1, double* j0, double* j1) {
            const int s = L.src[i];
            double xn, yn, ob[2];
            corner_point(cam, model.corners + (size_t)L.mmodel[k] * model.model_size * 24, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, Y);
            point_residual(R, dR, x, cam.fx, cam.fy, cam.cx, cam.cy, Y, ob, q0, q1, j0, j1, true);
        };
        // ---- pass 1: U and sum Jp^T r over the record's points, member by member, lane l owning points l, l + 64, ... of a member's run
        double H[21], b[6];
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) b[a] = 0.0;
        for (int k = 0; k < nmem; k++) {
            const int i1 = L.mstart[k + 1];
            for (int i = L.mstart[k] + lane; i < i1; i += 64) {
                double Y[3], q0, q1, j0[6], j1[6];
                point(k, i, Y, q0, q1, j0, j1);
                gram6_add(j0, j1, H);
                grad6_add(j0, j1, q0, q1, b);
            }
        }
        double Lc[36];
        const bool pd = pose_block6(H, b, Lc);  // the same in every lane; b is y from here on
        if (lane == 0) flags[r] = pd ? 0 : kRecSingular;
        if (!pd) continue;
        // ---- pass 2: the slot block of every member, Jm = (dr/dY) [-[Y]x | I]
        double* W = ws + (size_t)(r - r0) * kRfitSlots * kSlotDoubles;
        for (int k = 0; k < nmem; k++) {
            const int i1 = L.mstart[k + 1];
            double Z[36], A[21], gm[6];
#pragma unroll
            for (int e = 0; e < 36; e++) Z[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 21; e++) A[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) gm[e] = 0.0;
            for (int i = L.mstart[k] + lane; i < i1; i += 64) {  // the same lanes as in pass 1: they decide the order of the wave sums
                double Y[3], q0, q1, j0[6], j1[6], x0[3], x1[3], m0[6], m1[6];
                point(k, i, Y, q0, q1, j0, j1);
                point_dX(R, j0, j1, x0, x1);  // d residual / d Y
                slot_rows(Y, x0, x1, m0, m1);
                cross6_add(j0, j1, m0, m1, Z);
                gram6_add(m0, m1, A);
                grad6_add(m0, m1, q0, q1, gm);
            }
            slot_finish(Z, A, gm, Lc, b, lane, W + (size_t)k * kSlotDoubles);
        }
    }
}

// k_fit_assemble's SlotOf: a row of blocks per rig; the record's table row says which member holds a model slot of the rig, another
// rig's record holds none (a block-uniform branch)
struct RfitSlotOf {
    const int8_t* table;
    const int32_t* rec_rig;
    __device__ int group() const { return blockIdx.y; }
    __device__ bool operator()(int r, int a, int b, int& ka, int& kb) const {
        if (rec_rig[r] != group()) return false;
        ka = table[(size_t)r * kRfitSlots + a];
        kb = table[(size_t)r * kRfitSlots + b];
        return ka >= 0 && kb >= 0;
    }
};

}  // namespace ctag

// =====================================================================================================
// host side: the parts the assembly shares with the model reconstruction are ctag_fit_host.h's (namespace ctag::fit)
// =====================================================================================================
namespace {

namespace fit = ctag::fit;

struct Rigid {  // X_rig = R X_in + t
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
};

// The device side of one call: the rigs' systems (a group is a rig), the record workspace, and the slots of the models in them.
struct RfitWork : fit::SlotSystems<ctag::kRfitN> {
    std::vector<int32_t> slot_of_model;  // [n_models]: the model's slot in its rig's system, -1 outside every system
    ctag::DevBuf<int32_t> d_slot;
    ctag::DevBuf<int8_t> d_table;

    int setup(int pass_records) {
        const int n_models = (int)slot_of_model.size();
        const int rc = SlotSystems::setup(pass_records, ctag::kRfitPassRecords);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_table.grow((size_t)std::max(R, 1) * ctag::kRfitSlots));
        FIT_HIP(d_slot.grow(std::max(n_models, 1)));
        if (n_models > 0) FIT_HIP(hipMemcpyAsync(d_slot.p, slot_of_model.data(), sizeof(int32_t) * n_models, hipMemcpyHostToDevice, c.s));
        return CTAG_OK;
    }

    // S and g of every rig at (model, recs_dev).  Waits.
    int build_system(const ctag_model* model, const ctag_rig_pose_rec* recs_dev) {
        const ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
        return build_timed(c, [&](int r0, int r1) {
            hipLaunchKernelGGL(ctag::k_rfit_record, dim3(std::min(r1 - r0, ctag::kRfitGrid)), dim3(64), 0, c.s, c.res, c.n_frames, recs_dev, d_obs.p, r0, r1, md,
                               d_slot.p, c.cam, d_ws.p, d_table.p, d_flags.p);
            assemble(ctag::RfitSlotOf{d_table.p, d_rec_group.p}, r0, r1);
        });
    }
};

int rfit_opts(const ctag_rig_fit_opts* o, ctag_rig_fit_opts& r) {
    ctag_rig_fit_opts_default(&r);
    if (o) r = *o;
    return r.max_rounds >= 0 && r.min_frames >= 1 && fit::lm_opts_ok(r) ? CTAG_OK : CTAG_ERR_ARG;
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
        fit::mat_vec(T.R, X, Y);
        for (int k = 0; k < 3; k++) W->corners[((size_t)m * pm + c) * 3 + k] = (float)(Y[k] + T.t[k]);
    }
    const double B[3] = {(double)in->base[3 * m], (double)in->base[3 * m + 1], (double)in->base[3 * m + 2]};
    const double Ax[3] = {(double)in->axis[3 * m], (double)in->axis[3 * m + 1], (double)in->axis[3 * m + 2]};
    double Y[3];
    fit::mat_vec(T.R, B, Y);
    for (int k = 0; k < 3; k++) W->base[3 * m + k] = (float)(Y[k] + T.t[k]);
    fit::mat_vec(T.R, Ax, Y);
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
    return w.probe(rig, lambda, S, g, delta, n_unknowns, bad_pivot);
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
        std::vector<uint8_t> in_tree;
        const int anchor = fit::covisibility_tree(k, cnt, opts.min_frames, in_tree, [&](int ba, int bb, int best) {
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
                fit::mat_mul(RaT, Rb, Q);
                for (int i = 0; i < 9; i++) sumR[i] += Q[i];
                for (int i = 0; i < 3; i++) d[i] = poses[ib].tvec[i] - poses[ia].tvec[i];
                fit::mat_vec(RaT, d, e);
                for (int i = 0; i < 3; i++) sumt[i] += e[i];
            }
            Rigid E;
            double sv[3];
            fit::nearest_rotation(sumR, E.R, sv);
            for (int i = 0; i < 3; i++) E.t[i] = sumt[i] / (double)best;
            Rigid& Tb = T[mb];
            const Rigid& Ta = T[ma];
            fit::mat_mul(Ta.R, E.R, Tb.R);
            double e[3];
            fit::mat_vec(Ta.R, E.t, e);
            for (int i = 0; i < 3; i++) Tb.t[i] = e[i] + Ta.t[i];
            model_stats[mb].parent = ma;
            model_stats[mb].n_frames_with_parent = best;
        });
        if (anchor < 0) continue;
        for (int a = 0; a < k; a++)
            if (in_tree[a]) {
                if (a == anchor) w.drop[g] = w.n_slots[g];
                w.slot_of_model[M[a]] = w.n_slots[g]++;
                placed[M[a]] = 1;
                model_stats[M[a]].status = CTAG_POSE_OK;
            }
        rig_stats[g].status = CTAG_POSE_OK;
        rig_stats[g].anchor = M[anchor];
        rig_stats[g].n_placed = w.n_slots[g];
        rig_stats[g].n_unplaced = k - w.n_slots[g];
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
            fit::mat_mul(E, T[m].R, Tt[m].R);
            fit::mat_vec(E, T[m].t, e);
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
