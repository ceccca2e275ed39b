// k_rig_pose.hip -- one pose per rig (a rigid object carrying several markers whose models share one frame) for every frame
// of a batch, on the device, straight from the detection records.  The pose of a rig is the arithmetic of k_pose.hip (the
// reference's PnPSolver: solvePnP EPNP, then PoseBA) applied to the union of its members' correspondences; the semantics
// are stated in include/ctag_pose.h.
//
// Mapping:
//   k_rig_count        one thread per (frame, rig) item: membership, exclusions and the point count n, by the per-marker
//                      correspondence rule of ctag_pose_dev.h run without writing.  It writes every record's header and
//                      zero pose fields, and appends the items that need a solve to one of two work lists: n <= 160 and n > 160.
//   k_rig_solve<160,64>  the small list: one wave per item on k_pose's LDS image and occupancy.
//   k_rig_solve<800,256> the large list: a 256-thread workgroup per item on an 800-point LDS image (~130 KB, one workgroup
//                      per CU); per-point loops stride over the four waves, every sum over the points stays with its owner lane.
// Both solves are grid-stride over their list and share the EPnP + PoseBA body with k_pose (ctag_pose_dev.h), so a rig
// record equals the sequential evaluation over the concatenated points bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"

static_assert(sizeof(ctag_rig_pose_rec) == 160, "ctag_rig_pose_rec layout");
static_assert(CTAG_RIG_MAX_POINTS == CTAG_MAX_FEATURES * 8, "every valid detection record fits one rig problem");

// struct ctag_rigs: ctag_internal.h (the multi-view poses of k_mv_pose.hip read it too)

namespace ctag {

constexpr int kRigSmallPts = kPoseMaxPts;       // 160: one wave, k_pose's LDS image
constexpr int kRigMaxPts = CTAG_RIG_MAX_POINTS;  // 800
constexpr int kRigLargeThreads = 256;

__global__ __launch_bounds__(256) void k_rig_count(const ctag_frame_result* __restrict__ res, int n_frames, PoseModelDev model,
                                                   const int32_t* __restrict__ rig_of_model, int n_rigs, ctag_rig_pose_rec* __restrict__ out,
                                                   int32_t* __restrict__ lists, int32_t* __restrict__ counts) {
    const int n_items = n_frames * n_rigs;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < n_items; item += gridDim.x * blockDim.x) {
        const int f = item / n_rigs, g = item - f * n_rigs;
        const ctag_frame_result& FR = res[f];
        int status = CTAG_POSE_NOT_SEEN, n_members = 0, n_excluded = 0, n = 0;
        uint32_t mask[4] = {0u, 0u, 0u, 0u};
        if (FR.status == CTAG_OK) {
            const int nm = min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
            for (int k = 0; k < nm; k++) {
                const ctag_marker_rec& M = FR.markers[k];
                const int mi = model_lookup(model, M.marker_id);
                if (mi < 0 || rig_of_model[mi] != g) continue;
                bool dup = false;  // equal marker ids <=> equal model index: the first marker with it claims it
                for (int k2 = 0; k2 < k && !dup; k2++) dup = FR.markers[k2].marker_id == M.marker_id;
                int nl = 0;
                if (dup || marker_points(FR, M, model.model_size, kPoseMaxPts, nl, [](const ctag_feature_rec&, int, int, int) {}) != CTAG_POSE_OK ||
                    n + nl > kRigMaxPts) {
                    n_excluded++;
                    continue;
                }
                mask[k >> 5] |= 1u << (k & 31);
                n_members++;
                n += nl;
            }
            status = n_members == 0 ? CTAG_POSE_NOT_SEEN : (n < 4 ? CTAG_POSE_TOO_FEW : CTAG_POSE_OK);
        }
        ctag_rig_pose_rec* P = out + item;
        P->status = status;
        P->rig = g;
        P->frame = f;
        P->n_members = n_members;
        P->n_excluded = n_excluded;
        P->n_points = n;
        P->iterations = 0;
        P->reserved = 0;
        for (int i = 0; i < 4; i++) P->member_mask[i] = mask[i];
        for (int i = 0; i < 3; i++) P->rvec[i] = P->tvec[i] = P->rvec0[i] = P->tvec0[i] = 0.0;
        P->cost0 = P->cost = 0.0;
        if (status == CTAG_POSE_OK) {
            const int large = n > kRigSmallPts ? 1 : 0;
            lists[large * n_items + atomicAdd(&counts[large], 1)] = item;
        }
    }
}

// Items of one work list: the members' correspondences (member_mask of the record k_rig_count wrote) into LDS, then EPnP +
// PoseBA.  `list` holds *count items, each with n <= PTS points.
template <int PTS, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_rig_solve(const ctag_frame_result* __restrict__ res, int n_rigs,
                                                                                            const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                                                            PoseModelDev model, PoseCam cam, ctag_rig_pose_rec* __restrict__ out) {
    __shared__ PoseLds<PTS> S;
    const int lane = threadIdx.x;
    const int total = *count;
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int item = list[w];
        const ctag_frame_result& FR = res[item / n_rigs];
        ctag_rig_pose_rec* P = out + item;
        uint32_t mask[4];
        for (int i = 0; i < 4; i++) mask[i] = P->member_mask[i];
        const int nm = min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
        wave_sync();  // previous item's LDS reads are done
        int n = 0;
        for (int k = 0; k < nm; k++) {
            if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
            const ctag_marker_rec& M = FR.markers[k];
            const int mi = model_lookup(model, M.marker_id);
            const float* __restrict__ corners = model.corners + (size_t)mi * model.model_size * 24;
            const int base = n;
            int nl = 0;
            (void)marker_points(FR, M, model.model_size, kPoseMaxPts, nl, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
                if (lane < cnt && base + i0 + cnt <= PTS) load_point(S, cam, corners, F, pos, lane, base + i0 + lane);
            });
            n += nl;
        }
        wave_sync();
        pose_solve<PTS, NT>(S, lane, n, cam, P);
    }
}

}  // namespace ctag

namespace {

struct RigState {
    ctag::DevBuf<int32_t> d_lists;   // 2 x n_items work items
    ctag::DevBuf<int32_t> d_counts;  // the two lists' lengths
    ctag::DevBuf<ctag_frame_result> d_result;  // scratch of ctag_estimate_rig_pose
    ctag::DevBuf<ctag_rig_pose_rec> d_out;
};

void rig_state_free(void* p) { delete static_cast<RigState*>(p); }

RigState* rig_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kRigState, rig_state_free);
    if (!*slot) {
        RigState* s = new (std::nothrow) RigState();
        if (!s) return nullptr;
        if (s->d_counts.grow(2) != hipSuccess) {
            rig_state_free(s);
            return nullptr;
        }
        *slot = s;
    }
    return static_cast<RigState*>(*slot);
}

}  // namespace

namespace ctag {

int rigs_to_device(ctag_rigs* r, int device) {
    if (r->device == device && r->d_rig.p) return CTAG_OK;
    r->d_rig.release();  // (it may lie on another device)
    if (r->d_rig.grow(std::max<size_t>(1, r->rig_of_model.size())) != hipSuccess) return CTAG_ERR_HIP;
    if (!r->rig_of_model.empty() &&
        hipMemcpy(r->d_rig.p, r->rig_of_model.data(), sizeof(int32_t) * r->rig_of_model.size(), hipMemcpyHostToDevice) != hipSuccess)
        return CTAG_ERR_HIP;
    r->device = device;
    return CTAG_OK;
}

}  // namespace ctag

using ctag::rigs_to_device;

extern "C" {

int ctag_rigs_create(const ctag_model* model, const int32_t* rig_of_model, int n_rigs, ctag_rigs** out) {
    if (!model || !out || n_rigs < 1 || (model->n_models > 0 && !rig_of_model)) return CTAG_ERR_ARG;
    for (int i = 0; i < model->n_models; i++)
        if (rig_of_model[i] < -1 || rig_of_model[i] >= n_rigs) return CTAG_ERR_ARG;
    ctag_rigs* r = new (std::nothrow) ctag_rigs();
    if (!r) return CTAG_ERR_ARG;
    r->n_models = model->n_models;
    r->n_rigs = n_rigs;
    r->rig_of_model.assign(rig_of_model, rig_of_model + model->n_models);
    *out = r;
    return CTAG_OK;
}

void ctag_rigs_free(ctag_rigs* r) {
    delete r;
}

int ctag_rig_pose_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model_c,
                               const ctag_rigs* rigs_c, const ctag_camera* camera, ctag_rig_pose_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model_c || !rigs_c || !out_dev) return CTAG_ERR_ARG;
    if (rigs_c->n_models != model_c->n_models) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    const long long n_items = (long long)n_frames * rigs_c->n_rigs;
    if (n_items > INT_MAX / 2) return CTAG_ERR_LIMIT;  // item indices and the two lists stay in int32
    if (n_items == 0) return CTAG_OK;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    ctag_rigs* rigs = const_cast<ctag_rigs*>(rigs_c);
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    if (ctag::model_to_device(model, dev) != CTAG_OK || rigs_to_device(rigs, dev) != CTAG_OK) return CTAG_ERR_HIP;
    RigState* st = rig_state(h);
    if (!st) return CTAG_ERR_HIP;
    {   // records of frames that wait for the any-frame pass (CTAG_PENDING) are completed before they are read
        const int fr = ctag::handle_finish_pending(h);
        if (fr != CTAG_OK) return fr;
    }
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    if (st->d_lists.cap < 2 * (size_t)n_items) {
        if (st->d_lists.p && hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;  // an earlier call's kernels may still read the old lists
        if (st->d_lists.grow(2 * (size_t)n_items) != hipSuccess) return CTAG_ERR_HIP;
    }
    const int ni = (int)n_items;
    const ctag::PoseCam cam = ctag::make_pose_cam(camera);
    const ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
    if (hipMemsetAsync(st->d_counts.p, 0, 2 * sizeof(int32_t), s) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_rig_count, dim3(std::min((ni + 255) / 256, 1024)), dim3(256), 0, s, results_dev, n_frames, md, rigs->d_rig.p,
                       rigs->n_rigs, out_dev, st->d_lists.p, st->d_counts.p);
    // grids for the worst case (every item in one list); a workgroup past its list's length exits at once
    hipLaunchKernelGGL((ctag::k_rig_solve<ctag::kRigSmallPts, 64>), dim3(std::min(ni, 256 * 16)), dim3(64), 0, s, results_dev, rigs->n_rigs,
                       st->d_lists.p, st->d_counts.p, md, cam, out_dev);
    hipLaunchKernelGGL((ctag::k_rig_solve<ctag::kRigMaxPts, ctag::kRigLargeThreads>), dim3(std::min(ni, 256)), dim3(ctag::kRigLargeThreads), 0, s,
                       results_dev, rigs->n_rigs, st->d_lists.p + ni, st->d_counts.p + 1, md, cam, out_dev);
    if (hipGetLastError() != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

int ctag_estimate_rig_pose(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_rigs* rigs,
                           const ctag_camera* camera, ctag_rig_pose_rec* out) {
    if (!h || !result || !model || !rigs || !camera || !out) return CTAG_ERR_ARG;
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    RigState* st = rig_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    if (st->d_result.grow(1) != hipSuccess) return CTAG_ERR_HIP;
    if (st->d_out.cap < (size_t)rigs->n_rigs) {
        if (st->d_out.p && hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
        if (st->d_out.grow((size_t)rigs->n_rigs) != hipSuccess) return CTAG_ERR_HIP;
    }
    if (hipMemcpyAsync(st->d_result.p, result, sizeof(ctag_frame_result), hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    const int rc = ctag_rig_pose_batch_device(h, st->d_result.p, 1, model, rigs, camera, st->d_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_rig_pose_rec) * (size_t)rigs->n_rigs, hipMemcpyDeviceToHost, s) != hipSuccess)
        return CTAG_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

}  // extern "C"
