// k_pose.hip -- pose of every decoded marker of a batch, on the device, straight from the detection records.
// Replaces, for the GPU path,
//   CylinderTag::estimatePose        /root/reference/CylinderTag.cpp:198-209
//   PoseEstimator::PnPSolver         /root/reference/pose_estimation.cpp:50-98   correspondences + cv::solvePnP(SOLVEPNP_EPNP)
//   PoseEstimator::PoseBA            /root/reference/pose_estimation.cpp:100-143 cv::undistortPoints + Ceres LM on the
//                                                                                reprojection residual of :5-48
// Third-party arithmetic restated from the published algorithms (OpenCV 4.5.3 calib3d epnp.cpp / undistort, Ceres 2.0
// trust_region_minimizer.cc + levenberg_marquardt_strategy.cc); none of it is GEMM-shaped at these sizes (<= 160 points,
// 6 unknowns), so no MFMA: FP64 VALU, one wavefront per marker.
//
// Mapping: block = one wave = one marker.  Lanes are points wherever the work is per point (undistortion, barycentric
// coordinates, camera-frame points, residuals and Jacobian rows); every SUM the CPU path accumulates sequentially over
// the points is accumulated by ONE lane in the same order (lane = matrix entry: 144 entries of M^T M, 21+6+1 entries of
// the normal equations), so the result does not depend on the wave width and equals the sequential evaluation bit for
// bit.  The 12x12 symmetric eigenproblem runs as cyclic Jacobi in round-robin order, six disjoint rotations at a time.
// The correspondence rule and the EPnP + PoseBA body live in ctag_pose_dev.h, shared with the rig poses of k_rig_pose.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <string>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_linalg.h"
#include "ctag_pose_dev.h"

namespace ctag {

__global__ __launch_bounds__(256) void k_pose_offsets(const ctag_frame_result* __restrict__ res, int n_frames, int32_t* __restrict__ offsets) {
    // exclusive scan of the per-frame marker counts, one block
    __shared__ int32_t part[256];
    const int tid = threadIdx.x;
    const int per = (n_frames + 255) / 256;
    const int f0 = tid * per, f1 = min(f0 + per, n_frames);
    int32_t s = 0;
    // a corrupted record cannot make the work list (or a reader of FR.markers[]) run past the record's arrays
    auto count = [&](int f) -> int32_t { return res[f].status == CTAG_OK ? min(max(res[f].n_markers, 0), CTAG_MAX_MARKERS) : 0; };
    for (int f = f0; f < f1; f++) s += count(f);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int32_t run = 0;
        for (int i = 0; i < 256; i++) {
            const int32_t v = part[i];
            part[i] = run;
            run += v;
        }
        offsets[n_frames] = run;
    }
    __syncthreads();
    int32_t run = part[tid];
    for (int f = f0; f < f1; f++) {
        offsets[f] = run;
        run += count(f);
    }
}


template <int PTS, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_pose(const ctag_frame_result* __restrict__ res, int n_frames, const int32_t* __restrict__ offsets,
                                             PoseModelDev model, PoseCam cam, ctag_pose_rec* __restrict__ out, int capacity) {
    __shared__ PoseLds<PTS> S;
    const int lane = threadIdx.x;
    const int total = min(offsets[n_frames], capacity);
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        // work item -> (frame, marker): last frame with offsets[f] <= w
        int lo = 0, hi = n_frames - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offsets[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const int frame = lo, mk = w - offsets[lo];
        const ctag_frame_result& FR = res[frame];
        const ctag_marker_rec M = FR.markers[mk];
#ifdef CTAG_POSE_PROF
        unsigned long long prof_t = __builtin_readcyclecounter();
#endif
        ctag_pose_rec* P = out + w;
        wave_sync();  // previous item's LDS reads are done

        // ---- model lookup (pose_estimation.cpp:57-70) and correspondences (:72-95)
        const int mi = model_lookup(model, M.marker_id);
        int status = mi < 0 ? CTAG_POSE_NO_MODEL : CTAG_POSE_OK;
        int n = 0;
        if (status == CTAG_POSE_OK) {
            const float* __restrict__ corners = model.corners + (size_t)mi * model.model_size * 24;
            status = marker_points(FR, M, model.model_size, PTS, n, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
                if (lane < cnt) load_point(S, cam, corners, F, pos, lane, i0 + lane);
            });
        }
        if (status == CTAG_POSE_OK && n < 4) status = CTAG_POSE_TOO_FEW;
        if (lane == 0) {
            P->status = status;
            P->model_index = mi;
            P->frame = frame;
            P->marker = mk;
            P->n_points = status == CTAG_POSE_BAD_POS ? 0 : n;
            P->iterations = 0;
            for (int i = 0; i < 3; i++) P->rvec[i] = P->tvec[i] = P->rvec0[i] = P->tvec0[i] = 0.0;
            P->cost0 = P->cost = 0.0;
        }
        if (status != CTAG_POSE_OK) continue;  // wave-uniform
        wave_sync();
        PROF_MARK(0);
        pose_solve<PTS, 64>(S, lane, n, cam, P);
    }
}

}  // namespace ctag

// =====================================================================================================
// host side: model / camera objects, loaders, launch
// =====================================================================================================
// struct ctag_model: ctag_internal.h (the overlay of k_draw.hip reads it too)

namespace {

struct PoseState {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending = false;
    float last_ms = 0.f;
    ctag::DevBuf<int32_t> d_offsets;  // scratch of ctag_estimate_pose
    ctag::DevBuf<ctag_pose_rec> d_poses;
    ctag::DevBuf<ctag_frame_result> d_result;
};

void pose_state_free(void* p) {
    PoseState* s = static_cast<PoseState*>(p);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

PoseState* pose_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kPoseState, pose_state_free);
    if (!*slot) {
        PoseState* s = new (std::nothrow) PoseState();
        if (!s) return nullptr;
        if (hipEventCreate(&s->ev[0]) != hipSuccess || hipEventCreate(&s->ev[1]) != hipSuccess) {
            pose_state_free(s);
            return nullptr;
        }
        *slot = s;
    }
    return static_cast<PoseState*>(*slot);
}


}  // namespace

namespace ctag {

int model_to_device(ctag_model* m, int device) {
    if (m->device == device && m->d_ids.p) return CTAG_OK;
    m->d_ids.release();  // (they may lie on another device)
    m->d_corners.release();
    m->d_base_axis.release();
    m->d_base = m->d_axis = nullptr;
    if (m->d_ids.grow(std::max<size_t>(1, m->ids.size())) != hipSuccess) return CTAG_ERR_HIP;
    if (m->d_corners.grow(std::max<size_t>(1, m->corners.size())) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpy(m->d_ids.p, m->ids.data(), sizeof(int32_t) * m->ids.size(), hipMemcpyHostToDevice) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpy(m->d_corners.p, m->corners.data(), sizeof(float) * m->corners.size(), hipMemcpyHostToDevice) != hipSuccess)
        return CTAG_ERR_HIP;
    const size_t nb = m->base.size();
    if (m->d_base_axis.grow(std::max<size_t>(1, 2 * nb)) != hipSuccess) return CTAG_ERR_HIP;
    m->d_base = m->d_base_axis.p;
    m->d_axis = m->d_base_axis.p + nb;
    if (nb && (hipMemcpy(m->d_base, m->base.data(), sizeof(float) * nb, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(m->d_axis, m->axis.data(), sizeof(float) * nb, hipMemcpyHostToDevice) != hipSuccess))
        return CTAG_ERR_HIP;
    m->device = device;
    return CTAG_OK;
}

bool camera_ok(const ctag_camera* c) {
    if (!c) return false;
    if (!(c->n_dist == 0 || c->n_dist == 4 || c->n_dist == 5 || c->n_dist == 8 || c->n_dist == 12 || c->n_dist == 14)) return false;
    if (c->n_dist == 14 && (c->dist[12] != 0.f || c->dist[13] != 0.f)) return false;  // tilted sensor model not supported
    return c->K[0] != 0.f && c->K[4] != 0.f;
}

}  // namespace ctag

using ctag::camera_ok;
using ctag::model_to_device;

extern "C" {

int ctag_model_create(const ctag_model_view* v, ctag_model** out) {
    if (!v || !out || v->n_models < 0 || v->model_size < 1 || v->model_size > (1 << 16) || (v->n_models > 0 && (!v->marker_id || !v->corners)))
        return CTAG_ERR_ARG;
    ctag_model* m = new (std::nothrow) ctag_model();
    if (!m) return CTAG_ERR_ARG;
    m->n_models = v->n_models;
    m->model_size = v->model_size;
    const size_t n = (size_t)v->n_models;
    m->ids.assign(v->marker_id, v->marker_id + n);
    m->base.assign(n * 3, 0.f);
    m->axis.assign(n * 3, 0.f);
    if (v->base) m->base.assign(v->base, v->base + n * 3);
    if (v->axis) m->axis.assign(v->axis, v->axis + n * 3);
    m->corners.assign(v->corners, v->corners + n * v->model_size * 24);
    *out = m;
    return CTAG_OK;
}

// CylinderTag::loadModel (CylinderTag.cpp:161-190): "model_num model_size", then per model: id, base xyz, axis xyz and
// model_size*8 lines "corner_id x y z" (values parsed as float, stored at corner_id).
int ctag_model_load(const char* path, ctag_model** out) {
    if (!path || !out) return CTAG_ERR_ARG;
    std::ifstream in(path);
    if (!in.is_open()) return CTAG_ERR_ARG;
    int n = 0, size = 0;
    in >> n >> size;
    if (!in || n < 0 || n > (1 << 20) || size < 1 || size > (1 << 16)) return CTAG_ERR_ARG;
    ctag_model* m = new (std::nothrow) ctag_model();
    if (!m) return CTAG_ERR_ARG;
    m->n_models = n;
    m->model_size = size;
    m->ids.assign(n, 0);
    m->base.assign((size_t)n * 3, 0.f);
    m->axis.assign((size_t)n * 3, 0.f);
    m->corners.assign((size_t)n * size * 24, 0.f);
    for (int i = 0; i < n; i++) {
        in >> m->ids[i];
        for (int k = 0; k < 3; k++) in >> m->base[3 * i + k];
        for (int k = 0; k < 3; k++) in >> m->axis[3 * i + k];
        for (int j = 0; j < 8 * size; j++) {
            int cid = -1;
            float x = 0, y = 0, z = 0;
            in >> cid >> x >> y >> z;
            if (!in || cid < 0 || cid >= 8 * size) {  // the reference would write out of bounds
                delete m;
                return CTAG_ERR_ARG;
            }
            float* c = &m->corners[((size_t)i * size * 8 + cid) * 3];
            c[0] = x;
            c[1] = y;
            c[2] = z;
        }
    }
    *out = m;
    return CTAG_OK;
}

void ctag_model_free(ctag_model* m) {
    delete m;
}

int ctag_model_get_view(const ctag_model* m, ctag_model_view* v) {
    if (!m || !v) return CTAG_ERR_ARG;
    v->n_models = m->n_models;
    v->model_size = m->model_size;
    v->marker_id = m->ids.data();
    v->base = m->base.data();
    v->axis = m->axis.data();
    v->corners = m->corners.data();
    return CTAG_OK;
}

// The two nodes cv::FileStorage reads at CylinderTag.cpp:192-196, from an OpenCV "%YAML:1.0" file:
//   name: !!opencv-matrix \n rows: R \n cols: C \n dt: f|d \n data: [ v, v, ... ]
int ctag_camera_load(const char* path, ctag_camera* out) {
    if (!path || !out) return CTAG_ERR_ARG;
    std::ifstream in(path);
    if (!in.is_open()) return CTAG_ERR_ARG;
    std::string txt((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    auto read_node = [&](const char* name, int& rows, int& cols, std::vector<double>& data) -> bool {
        size_t p = 0;
        const std::string key = std::string(name) + ":";
        for (;;) {  // a key at the start of a line
            p = txt.find(key, p);
            if (p == std::string::npos) return false;
            if (p == 0 || txt[p - 1] == '\n') break;
            p += key.size();
        }
        auto field = [&](const char* f, size_t from) -> size_t {
            const size_t q = txt.find(f, from);
            return q == std::string::npos ? q : q + std::strlen(f);
        };
        size_t q = field("rows:", p);
        if (q == std::string::npos) return false;
        rows = std::atoi(txt.c_str() + q);
        q = field("cols:", q);
        if (q == std::string::npos) return false;
        cols = std::atoi(txt.c_str() + q);
        q = field("data:", q);
        if (q == std::string::npos) return false;
        q = txt.find('[', q);
        const size_t e = txt.find(']', q);
        if (q == std::string::npos || e == std::string::npos) return false;
        data.clear();
        const char* s = txt.c_str() + q + 1;
        const char* end = txt.c_str() + e;
        while (s < end) {
            char* nx = nullptr;
            const double v = std::strtod(s, &nx);
            if (nx == s) {
                s++;
                continue;
            }
            data.push_back(v);
            s = nx;
        }
        return rows > 0 && cols > 0 && (size_t)rows * cols == data.size();
    };
    int r = 0, c = 0;
    std::vector<double> d;
    std::memset(out, 0, sizeof(*out));
    if (!read_node("cameraMatrix", r, c, d) || r != 3 || c != 3) return CTAG_ERR_ARG;
    for (int i = 0; i < 9; i++) out->K[i] = (float)d[i];
    if (!read_node("distCoeffs", r, c, d) || d.size() > 14) return CTAG_ERR_ARG;
    for (size_t i = 0; i < d.size(); i++) out->dist[i] = (float)d[i];
    out->n_dist = (int)d.size();
    return camera_ok(out) ? CTAG_OK : CTAG_ERR_UNSUPPORTED;
}

int ctag_pose_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model_c,
                           const ctag_camera* camera, int32_t* offsets_dev, ctag_pose_rec* poses_dev, int capacity) {
    if (!h || !results_dev || n_frames < 0 || !model_c || !offsets_dev || !poses_dev || capacity < 0) return CTAG_ERR_ARG;
    if (!camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag_model* model = const_cast<ctag_model*>(model_c);
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    if (model_to_device(model, dev) != CTAG_OK) return CTAG_ERR_HIP;
    PoseState* st = pose_state(h);
    if (!st) return CTAG_ERR_HIP;
    {   // records of frames that wait for the any-frame pass (CTAG_PENDING) are completed before they are read
        const int fr = ctag::handle_finish_pending(h);
        if (fr != CTAG_OK) return fr;
    }
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const ctag::PoseCam cam = ctag::make_pose_cam(camera);
    ctag::PoseModelDev md{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
    const bool timing = ctag::handle_timing(h);
    if (timing && hipEventRecord(st->ev[0], s) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_pose_offsets, dim3(1), dim3(256), 0, s, results_dev, n_frames, offsets_dev);
    if (n_frames > 0 && capacity > 0) {
        const int grid = std::min(capacity, 256 * 16);
        if (model->model_size * 8 <= ctag::kPoseSmallPts)
            hipLaunchKernelGGL((ctag::k_pose<ctag::kPoseSmallPts, 2>), dim3(grid), dim3(64), 0, s, results_dev, n_frames, offsets_dev, md, cam,
                               poses_dev, capacity);
        else
            hipLaunchKernelGGL((ctag::k_pose<ctag::kPoseMaxPts, 1>), dim3(grid), dim3(64), 0, s, results_dev, n_frames, offsets_dev, md, cam,
                               poses_dev, capacity);
    }
    if (hipGetLastError() != hipSuccess) return CTAG_ERR_HIP;
    if (timing) {
        if (hipEventRecord(st->ev[1], s) != hipSuccess) return CTAG_ERR_HIP;
        st->pending = true;
    }
    return CTAG_OK;
}

#ifdef CTAG_POSE_PROF
int ctag_pose_debug_prof(unsigned long long* out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(ctag::g_pose_prof), 16 * sizeof(unsigned long long)) != hipSuccess) return CTAG_ERR_HIP;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(ctag::g_pose_prof), z, sizeof(z)) != hipSuccess) return CTAG_ERR_HIP;
    }
    return CTAG_OK;
}
#endif

float ctag_pose_last_ms(ctag_handle* h) {
    if (!h) return 0.f;
    PoseState* st = pose_state(h);
    if (!st) return 0.f;
    if (st->pending) {
        if (hipEventSynchronize(st->ev[1]) == hipSuccess) (void)hipEventElapsedTime(&st->last_ms, st->ev[0], st->ev[1]);
        st->pending = false;
    }
    return st->last_ms;
}

int ctag_estimate_pose(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_camera* camera,
                       ctag_pose_rec* out) {
    if (!h || !result || !model || !camera) return CTAG_ERR_ARG;
    if (result->status != CTAG_OK || result->n_markers <= 0) return CTAG_OK;
    if (!out || result->n_markers > CTAG_MAX_MARKERS) return CTAG_ERR_ARG;
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    PoseState* st = pose_state(h);
    if (!st) return CTAG_ERR_HIP;
    if (st->d_result.grow(1) != hipSuccess || st->d_offsets.grow(2) != hipSuccess || st->d_poses.grow(CTAG_MAX_MARKERS) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    if (hipMemcpyAsync(st->d_result.p, result, sizeof(ctag_frame_result), hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    const int rc = ctag_pose_batch_device(h, st->d_result.p, 1, model, camera, st->d_offsets.p, st->d_poses.p, CTAG_MAX_MARKERS);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_poses.p, sizeof(ctag_pose_rec) * result->n_markers, hipMemcpyDeviceToHost, s) != hipSuccess)
        return CTAG_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

}  // extern "C"
