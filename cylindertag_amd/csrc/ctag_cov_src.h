// ctag_cov_src.h -- rule 2 of the pose covariance (include/ctag_pose.h), which the robust refit shares: the points of a finished pose
// record of any of the three kinds, rebuilt from the detection record(s) where they lie.  Read by k_pose_cov.hip and k_pose_robust.hip.
// Both kernels walk a record once with the whole wave and leave one descriptor per point in LDS; what they do with the points afterwards
// is their own.  Lds is the kernel's LDS image: it has cam[kMvCams], R[kMvCams][9], t[kMvCams][3] (the camera set) and src[kCovMaxPts],
// model[kCovMaxPts] (where point i comes from: its descriptor, point_desc of ctag_pose_dev.h, and its model index).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"

namespace ctag {

constexpr int kCovMaxPts = CTAG_RIG_MAX_POINTS;  // 800

// Member k of frame record FR against model mi, seen by camera c: its points' descriptors from index n on.  False when the
// marker or the model lies outside its array, the builder rejects the marker or the total passes kCovMaxPts.
template <class Lds>
__device__ __forceinline__ bool cov_add_marker(Lds& L, const int lane, const ctag_frame_result& FR, const int k, const PoseModelDev& model,
                                               const int mi, const int c, int& n) {
    if (k < 0 || k >= min(max(FR.n_markers, 0), CTAG_MAX_MARKERS) || mi < 0 || mi >= model.n_models) return false;
    const ctag_marker_rec& M = FR.markers[k];
    const ctag_feature_rec* F0 = FR.features;
    const int base = n;
    int nl = 0;
    const int st = marker_points(FR, M, model.model_size, kPoseMaxPts, nl, [&](const ctag_feature_rec& F, int pos, int cnt, int i0) {
        if (lane < cnt && base + i0 + cnt <= kCovMaxPts) {
            L.src[base + i0 + lane] = point_desc((int)(&F - F0), lane, c, pos);
            L.model[base + i0 + lane] = mi;
        }
    });
    n += nl;
    return st == CTAG_POSE_OK && n <= kCovMaxPts;
}

// the members of one frame record by a member mask, in marker order, each against the first model with its id.  Not the fits'
// fit_member_walk (ctag_pose_dev.h), on purpose: a mask bit at or above the frame's marker count is rejected here and ignored there
template <class Lds>
__device__ __forceinline__ bool cov_add_members(Lds& L, const int lane, const ctag_frame_result& FR, const uint32_t* mask, const PoseModelDev& model,
                                                const int c, int& n) {
    if (FR.status != CTAG_OK) return false;
    for (int k = 0; k < 128; k++) {
        if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
        if (k >= min(max(FR.n_markers, 0), CTAG_MAX_MARKERS)) return false;
        if (!cov_add_marker(L, lane, FR, k, model, model_lookup(model, FR.markers[k].marker_id), c, n)) return false;
    }
    return true;
}

// ---- the three kinds of source record: count() records; build() leaves the descriptors of record P's points in L (false: rule
// 2's CTAG_COV_BAD_RECORD); frame(P, c) is the detection record camera c's points of P come from
struct CovMarkerSrc {
    using Rec = ctag_pose_rec;
    static constexpr bool kMultiView = false;
    const ctag_frame_result* res;
    int n_frames;
    const int32_t* offsets;
    const Rec* recs;
    int capacity;
    PoseCam cam;
    __device__ int count() const { return min(offsets[n_frames], capacity); }
    template <class Lds>
    __device__ void stage(Lds& L, int lane) const {
        if (lane == 0) L.cam[0] = cam;
    }
    __device__ const ctag_frame_result& frame(const Rec& P, int) const { return res[P.frame]; }
    template <class Lds>
    __device__ bool build(const Rec& P, const PoseModelDev& model, Lds& L, int lane, int& n) const {
        if (P.frame < 0 || P.frame >= n_frames || res[P.frame].status != CTAG_OK) return false;
        return cov_add_marker(L, lane, res[P.frame], P.marker, model, P.model_index, 0, n);
    }
};

struct CovRigSrc {
    using Rec = ctag_rig_pose_rec;
    static constexpr bool kMultiView = false;
    const ctag_frame_result* res;
    int n_frames, n_records;
    const Rec* recs;
    PoseCam cam;
    __device__ int count() const { return n_records; }
    template <class Lds>
    __device__ void stage(Lds& L, int lane) const {
        if (lane == 0) L.cam[0] = cam;
    }
    __device__ const ctag_frame_result& frame(const Rec& P, int) const { return res[P.frame]; }
    template <class Lds>
    __device__ bool build(const Rec& P, const PoseModelDev& model, Lds& L, int lane, int& n) const {
        if (P.frame < 0 || P.frame >= n_frames) return false;
        return cov_add_members(L, lane, res[P.frame], P.member_mask, model, 0, n);
    }
};

struct CovMvSrc {
    using Rec = ctag_mv_pose_rec;
    static constexpr bool kMultiView = true;
    MvResults res;
    int n_frames, n_records;
    const Rec* recs;
    MvCams cams;
    __device__ int count() const { return n_records; }
    template <class Lds>
    __device__ void stage(Lds& L, int lane) const {
        for (int c = lane; c < kMvCams; c += 64) {
            L.cam[c] = cams.cam[c];
            for (int i = 0; i < 9; i++) L.R[c][i] = cams.R[c][i];
            for (int i = 0; i < 3; i++) L.t[c][i] = cams.t[c][i];
        }
    }
    __device__ const ctag_frame_result& frame(const Rec& P, int c) const { return res.p[c][P.frame]; }
    template <class Lds>
    __device__ bool build(const Rec& P, const PoseModelDev& model, Lds& L, int lane, int& n) const {
        if (P.frame < 0 || P.frame >= n_frames) return false;
        for (int c = 0; c < kMvCams; c++) {
            const uint32_t* mask = P.member_mask[c];
            if ((mask[0] | mask[1] | mask[2] | mask[3]) == 0u) continue;
            if (c >= cams.n) return false;
            if (!cov_add_members(L, lane, res.p[c][P.frame], mask, model, c, n)) return false;
        }
        return true;
    }
};

// What every batch call of the two families does before it launches: the device, the model's device copy, the frames that wait for the
// any-frame pass (host side)
inline int cov_prepare(ctag_handle* h, const ctag_model* model_c, PoseModelDev& md, hipStream_t& s) {
    ctag_model* model = const_cast<ctag_model*>(model_c);
    const int dev = handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    if (model_to_device(model, dev) != CTAG_OK) return CTAG_ERR_HIP;
    const int fr = handle_finish_pending(h);
    if (fr != CTAG_OK) return fr;
    md = PoseModelDev{model->n_models, model->model_size, model->d_ids.p, model->d_corners.p};
    s = static_cast<hipStream_t>(ctag_stream(h));
    return CTAG_OK;
}

}  // namespace ctag
