// k_mv_pose.hip -- one pose per rig and frame from several calibrated cameras that see the same instant, on the device, straight
// from one detection record array per camera.  The semantics are stated in include/ctag_pose.h (multi-view rig pose).
//
// Mapping:
//   k_mv_count         one thread per (frame, rig) item: membership over all cameras by the rule of k_rig_count, the start camera,
//                      the record's header and zero pose fields; items that need a solve go to one of two work lists by their
//                      total point count: n <= 160 and n > 160.
//   k_mv_solve<160,64>   the small list, one wave per item; k_mv_solve<800,256> the large list, a 256-thread workgroup per item.
// A solve loads the start camera's points and runs EPnP + PoseBA on them (stage 1: pose_epnp and pose_ba of ctag_pose_dev.h with
// the one-camera residual, the bytes of k_rig_solve), moves that pose into the reference frame, then lays out the points of all
// cameras with a per-point camera index and runs pose_ba once more with the residual that carries a camera per point (stage 2).
// The cameras (intrinsics, Rc, tc) sit in LDS beside the problem's image.  The camera set (MvCams, ctag_camera_set) and the
// per-camera residual are stated in ctag_pose_dev.h: the covariance of k_pose_cov.hip reads them too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <new>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"

static_assert(sizeof(ctag_mv_pose_rec) == 432, "ctag_mv_pose_rec layout");
static_assert(CTAG_MV_MAX_CAMERAS <= 255, "the per-point camera index is one byte");

namespace ctag {

constexpr int kMvSmallPts = kPoseMaxPts;         // 160: one wave
constexpr int kMvMaxPts = CTAG_RIG_MAX_POINTS;   // 800
constexpr int kMvLargeThreads = 256;

__global__ __launch_bounds__(256) void k_mv_count(MvResults res, int n_cameras, int n_frames, PoseModelDev model, const int32_t* __restrict__ rig_of_model,
                                                  int n_rigs, ctag_mv_pose_rec* __restrict__ out, int32_t* __restrict__ lists, int32_t* __restrict__ counts) {
    const int n_items = n_frames * n_rigs;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < n_items; item += gridDim.x * blockDim.x) {
        const int f = item / n_rigs, g = item - f * n_rigs;
        ctag_mv_pose_rec* P = out + item;
        int n_members = 0, n_excluded = 0, n = 0, n_seen = 0, start = 0, start_points = 0;
        for (int c = 0; c < kMvCams; c++) {
            uint32_t mask[4] = {0u, 0u, 0u, 0u};
            int nc = 0, members = 0;
            if (c < n_cameras && res.p[c][f].status == CTAG_OK) {
                const ctag_frame_result& FR = res.p[c][f];
                const int nm = min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
                for (int k = 0; k < nm; k++) {
                    const ctag_marker_rec& M = FR.markers[k];
                    const int mi = model_lookup(model, M.marker_id);
                    if (mi < 0 || rig_of_model[mi] != g) continue;
                    bool dup = false;  // per camera: the first marker with a model index claims it
                    for (int k2 = 0; k2 < k && !dup; k2++) dup = FR.markers[k2].marker_id == M.marker_id;
                    int nl = 0;
                    if (dup || marker_points(FR, M, model.model_size, kPoseMaxPts, nl, [](const ctag_feature_rec&, int, int, int) {}) != CTAG_POSE_OK ||
                        n + nl > kMvMaxPts) {
                        n_excluded++;
                        continue;
                    }
                    mask[k >> 5] |= 1u << (k & 31);
                    members++;
                    nc += nl;
                    n += nl;
                }
            }
            n_members += members;
            if (members) n_seen++;
            if (nc > start_points) {  // the most points, the lowest index on a tie
                start = c;
                start_points = nc;
            }
            P->points_of_camera[c] = nc;
            for (int i = 0; i < 4; i++) P->member_mask[c][i] = mask[i];
        }
        const int status = n_members == 0 ? CTAG_POSE_NOT_SEEN : (start_points < 4 ? CTAG_POSE_TOO_FEW : CTAG_POSE_OK);
        P->status = status;
        P->rig = g;
        P->frame = f;
        P->n_cameras = n_seen;
        P->start_camera = start;
        P->n_members = n_members;
        P->n_excluded = n_excluded;
        P->n_points = n;
        P->iterations = P->iterations_cam = 0;
        P->reserved[0] = P->reserved[1] = 0;
        for (int i = 0; i < 3; i++) {
            P->rvec_epnp[i] = P->tvec_epnp[i] = P->rvec_cam[i] = P->tvec_cam[i] = 0.0;
            P->rvec_start[i] = P->tvec_start[i] = P->rvec[i] = P->tvec[i] = 0.0;
        }
        P->cost_cam0 = P->cost_cam = P->cost0 = P->cost = 0.0;
        if (status == CTAG_POSE_OK) {
            const int large = n > kMvSmallPts ? 1 : 0;
            lists[large * n_items + atomicAdd(&counts[large], 1)] = item;
        }
    }
}

// the cameras and the per-point camera index of one block
template <int PTS>
struct MvLds {
    PoseCam cam[kMvCams];
    double R[kMvCams][9];
    double t[kMvCams][3];
    unsigned char cam_of[PTS];
};

// the points of camera c's members of frame record FR (member_mask[c] of the record k_mv_count wrote) into S from index n on
template <int PTS>
__device__ __forceinline__ int mv_load_camera(PoseLds<PTS>& S, MvLds<PTS>& T, const int lane, const ctag_frame_result& FR, const uint32_t* mask,
                                              const PoseModelDev& model, const int c, int n) {
    const int nm = min(max(FR.n_markers, 0), CTAG_MAX_MARKERS);
    for (int k = 0; k < nm; k++) {
        if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
        const ctag_marker_rec& M = FR.markers[k];
        const int mi = model_lookup(model, M.marker_id);
        const float* __restrict__ corners = model.corners + (size_t)mi * model.model_size * 24;
        const int base = n;
        int nl = 0;
        (void)marker_points(FR, M, model.model_size, kPoseMaxPts, nl, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
            if (lane < cnt && base + i0 + cnt <= PTS) {
                load_point(S, T.cam[c], corners, F, pos, lane, base + i0 + lane);
                T.cam_of[base + i0 + lane] = (unsigned char)c;
            }
        });
        n += nl;
    }
    return n;
}

// Items of one work list.  `list` holds *count items, each with n_points <= PTS.
template <int PTS, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_mv_solve(MvResults res, int n_rigs, const int32_t* __restrict__ list,
                                                                                           const int32_t* __restrict__ count, PoseModelDev model, MvCams cams,
                                                                                           ctag_mv_pose_rec* __restrict__ out) {
    __shared__ PoseLds<PTS> S;
    __shared__ MvLds<PTS> T;
    const int lane = threadIdx.x;
    const int total = *count;
    if ((int)blockIdx.x >= total) return;
    for (int c = lane; c < kMvCams; c += NT) {
        T.cam[c] = cams.cam[c];
        for (int i = 0; i < 9; i++) T.R[c][i] = cams.R[c][i];
        for (int i = 0; i < 3; i++) T.t[c][i] = cams.t[c][i];
    }
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int item = list[w];
        const int f = item / n_rigs;
        ctag_mv_pose_rec* P = out + item;
        const int sc = min(max(P->start_camera, 0), cams.n - 1);
        const int n_total = P->n_points;
        uint32_t mask[4];
        for (int i = 0; i < 4; i++) mask[i] = P->member_mask[sc][i];
        wave_sync();  // previous item's LDS reads are done (and the cameras are in LDS)
        // ---- stage 1: the start camera alone
        const int ns = mv_load_camera(S, T, lane, res.p[sc][f], mask, model, sc, 0);
        wave_sync();
        if (!pose_epnp<PTS, NT>(S, lane, ns, T.cam[sc])) {
            if (lane == 0) P->status = CTAG_POSE_DEGENERATE;
            continue;  // block-uniform
        }
        double x[6];
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = S.x[i];
        if (lane == 0)
            for (int i = 0; i < 3; i++) {
                P->rvec_epnp[i] = x[i];
                P->tvec_epnp[i] = x[3 + i];
            }
        int iter_cam;
        double cost_cam0, cost_cam;
        pose_ba<PTS, NT>(S, lane, ns, x, camera_residual(S, T.cam[sc]), iter_cam, cost_cam0, cost_cam);
        // ---- into the reference frame: R_start = Rc^T R(rvec_cam), t_start = Rc^T (tvec_cam - tc)
        wave_sync();
        if (lane == 0) {
            if (!cams.at_reference[sc]) {
                const double* Rc = T.R[sc];
                const double* tc = T.t[sc];
                double R1[9], Rs[9], rv[3];
                ctl::angle_axis_rot(x, R1, nullptr);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) Rs[3 * i + j] = Rc[i] * R1[j] + Rc[3 + i] * R1[3 + j] + Rc[6 + i] * R1[6 + j];
                ctl::rodrigues_from_matrix(Rs, rv);
                const double d[3] = {x[3] - tc[0], x[4] - tc[1], x[5] - tc[2]};
                for (int i = 0; i < 3; i++) {
                    S.x[i] = rv[i];
                    S.x[3 + i] = Rc[i] * d[0] + Rc[3 + i] * d[1] + Rc[6 + i] * d[2];
                }
            } else {
                for (int i = 0; i < 6; i++) S.x[i] = x[i];
            }
            for (int i = 0; i < 3; i++) {
                P->rvec_cam[i] = x[i];
                P->tvec_cam[i] = x[3 + i];
                P->rvec_start[i] = S.x[i];
                P->tvec_start[i] = S.x[3 + i];
            }
            P->iterations_cam = iter_cam;
            P->cost_cam0 = cost_cam0;
            P->cost_cam = cost_cam;
        }
        wave_sync();
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = S.x[i];
        // ---- stage 2: all cameras' points
        int iter = 0;
        double cost0 = cost_cam, cost = cost_cam;
        if (ns != n_total) {  // block-uniform
            int n = 0;
            for (int c = 0; c < cams.n; c++) {
                for (int i = 0; i < 4; i++) mask[i] = P->member_mask[c][i];
                if ((mask[0] | mask[1] | mask[2] | mask[3]) == 0u) continue;
                n = mv_load_camera(S, T, lane, res.p[c][f], mask, model, c, n);
            }
            wave_sync();
            auto residual = [](int i, const double* R, const double* dR, const double* y, double& r0, double& r1, double* j0, double* j1) {
                const int c = T.cam_of[i];
                mv_point_residual(R, dR, y, T.cam[c], T.R[c], T.t[c], S.X + 3 * i, S.OBS + 2 * i, r0, r1, j0, j1);
            };
            pose_ba<PTS, NT>(S, lane, n, x, residual, iter, cost0, cost);
        }
        if (lane == 0) {
            for (int i = 0; i < 3; i++) {
                P->rvec[i] = x[i];
                P->tvec[i] = x[3 + i];
            }
            P->iterations = iter;
            P->cost0 = cost0;
            P->cost = cost;
        }
    }
}

}  // namespace ctag

namespace {

struct MvState {
    ctag::DevBuf<int32_t> d_lists;   // 2 x n_items work items
    ctag::DevBuf<int32_t> d_counts;  // the two lists' lengths
    ctag::DevBuf<ctag_frame_result> d_result;  // scratch of ctag_estimate_mv_rig_pose: one record per camera
    ctag::DevBuf<ctag_mv_pose_rec> d_out;
};

void mv_state_free(void* p) { delete static_cast<MvState*>(p); }

MvState* mv_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kMvState, mv_state_free);
    if (!*slot) {
        MvState* s = new (std::nothrow) MvState();
        if (!s) return nullptr;
        if (s->d_counts.grow(2) != hipSuccess) {
            mv_state_free(s);
            return nullptr;
        }
        *slot = s;
    }
    return static_cast<MvState*>(*slot);
}

}  // namespace

extern "C" {

int ctag_camera_set_create(const ctag_camera* cameras, const ctag_camera_pose* poses, int n_cameras, ctag_camera_set** out) {
    if (!cameras || !poses || !out || n_cameras < 1 || n_cameras > CTAG_MV_MAX_CAMERAS) return CTAG_ERR_ARG;
    for (int c = 0; c < n_cameras; c++)
        for (int i = 0; i < 3; i++)
            if (!ctl::finite64(poses[c].rvec[i]) || !ctl::finite64(poses[c].tvec[i])) return CTAG_ERR_ARG;
    for (int c = 0; c < n_cameras; c++)
        if (!ctag::camera_ok(&cameras[c])) return CTAG_ERR_UNSUPPORTED;
    ctag_camera_set* s = new (std::nothrow) ctag_camera_set();
    if (!s) return CTAG_ERR_ARG;
    ctag::MvCams& d = s->dev;
    d.n = n_cameras;
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) {  // the slots past n are copies of camera 0: never read, never uninitialised
        const int src = c < n_cameras ? c : 0;
        d.cam[c] = ctag::make_pose_cam(&cameras[src]);
        ctl::angle_axis_rot(poses[src].rvec, d.R[c], nullptr);
        bool zero = true;
        for (int i = 0; i < 3; i++) {
            d.t[c][i] = poses[src].tvec[i];
            zero = zero && poses[src].rvec[i] == 0.0 && poses[src].tvec[i] == 0.0;
        }
        d.at_reference[c] = zero ? 1 : 0;
        s->cameras[c] = cameras[src];
        s->poses[c] = poses[src];
    }
    *out = s;
    return CTAG_OK;
}

int ctag_camera_set_get(const ctag_camera_set* s, int* n_cameras, ctag_camera* cameras, ctag_camera_pose* poses) {
    if (!s || !n_cameras) return CTAG_ERR_ARG;
    *n_cameras = s->dev.n;
    for (int c = 0; c < s->dev.n; c++) {
        if (cameras) cameras[c] = s->cameras[c];
        if (poses) poses[c] = s->poses[c];
    }
    return CTAG_OK;
}

void ctag_camera_set_free(ctag_camera_set* s) {
    delete s;
}

int ctag_mv_rig_pose_batch_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_frames, const ctag_model* model_c,
                                  const ctag_rigs* rigs_c, const ctag_camera_set* cams, ctag_mv_pose_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model_c || !rigs_c || !cams || !out_dev) return CTAG_ERR_ARG;
    if (rigs_c->n_models != model_c->n_models) return CTAG_ERR_ARG;
    ctag::MvResults res;
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) {
        res.p[c] = c < cams->dev.n ? results_dev[c] : nullptr;
        if (c < cams->dev.n && !res.p[c]) return CTAG_ERR_ARG;
    }
    const long long n_items = (long long)n_frames * rigs_c->n_rigs;
    if (n_items > INT_MAX / 2) return CTAG_ERR_LIMIT;  // item indices and the two lists stay in int32
    if (n_items == 0) return CTAG_OK;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    ctag_rigs* rigs = const_cast<ctag_rigs*>(rigs_c);
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    if (ctag::model_to_device(model, dev) != CTAG_OK || ctag::rigs_to_device(rigs, dev) != CTAG_OK) return CTAG_ERR_HIP;
    MvState* st = mv_state(h);
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
    const ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
    if (hipMemsetAsync(st->d_counts.p, 0, 2 * sizeof(int32_t), s) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_mv_count, dim3(std::min((ni + 255) / 256, 1024)), dim3(256), 0, s, res, cams->dev.n, n_frames, md, rigs->d_rig.p,
                       rigs->n_rigs, out_dev, st->d_lists.p, st->d_counts.p);
    // grids for the worst case (every item in one list); a workgroup past its list's length exits at once
    hipLaunchKernelGGL((ctag::k_mv_solve<ctag::kMvSmallPts, 64>), dim3(std::min(ni, 256 * 16)), dim3(64), 0, s, res, rigs->n_rigs, st->d_lists.p,
                       st->d_counts.p, md, cams->dev, out_dev);
    hipLaunchKernelGGL((ctag::k_mv_solve<ctag::kMvMaxPts, ctag::kMvLargeThreads>), dim3(std::min(ni, 256)), dim3(ctag::kMvLargeThreads), 0, s, res,
                       rigs->n_rigs, st->d_lists.p + ni, st->d_counts.p + 1, md, cams->dev, out_dev);
    if (hipGetLastError() != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

int ctag_estimate_mv_rig_pose(ctag_handle* h, const ctag_frame_result* results, const ctag_model* model, const ctag_rigs* rigs,
                              const ctag_camera_set* cams, ctag_mv_pose_rec* out) {
    if (!h || !results || !model || !rigs || !cams || !out) return CTAG_ERR_ARG;
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    MvState* st = mv_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    if (st->d_result.grow(CTAG_MV_MAX_CAMERAS) != hipSuccess) return CTAG_ERR_HIP;
    if (st->d_out.cap < (size_t)rigs->n_rigs) {
        if (st->d_out.p && hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
        if (st->d_out.grow((size_t)rigs->n_rigs) != hipSuccess) return CTAG_ERR_HIP;
    }
    const int n = cams->dev.n;
    if (hipMemcpyAsync(st->d_result.p, results, sizeof(ctag_frame_result) * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    const ctag_frame_result* ptrs[CTAG_MV_MAX_CAMERAS];
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) ptrs[c] = c < n ? st->d_result.p + c : nullptr;
    const int rc = ctag_mv_rig_pose_batch_device(h, ptrs, 1, model, rigs, cams, st->d_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_mv_pose_rec) * (size_t)rigs->n_rigs, hipMemcpyDeviceToHost, s) != hipSuccess)
        return CTAG_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

}  // extern "C"
