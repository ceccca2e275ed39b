// k_pose_cov.hip -- the 6x6 covariance and the residual diagnostics of finished pose records (per marker, per rig, per rig from
// several cameras), on the device, from the pose records and the detection records where they lie.  The semantics are stated in
// include/ctag_pose.h (pose covariance, rules 1-6).
//
// Mapping: one kernel body, k_pose_cov<Src>, for the three record kinds and both parametrisations; Src
// says where a record's frames and members are.  One wavefront per source record for every size (4 .. 800 points), grid-stride
// over the records.
//   walk      the whole wave walks the record's members (ctag_cov_src.h, shared with k_pose_robust.hip) with the builder of ctag_pose_dev.h (marker_points) and leaves one
//             8-byte descriptor per point in LDS (which feature, corner, camera, model position) -- there is no LDS image of the
//             problem itself;
//   points    lane l takes points l, l+64, ... in order: corner_point (load + undistort), the residual of the pose kernels with
//             dR from angle_axis_rot (RVEC) or [e_k]x R (TANGENT), and its own 21 entries of J^T J, the sum of squares and the
//             largest residual norm with its index, all in FP64 registers;
//   combine   one fixed tree over the lanes (wave_sum_f64 / wave_max_f64 of ctag_wave.h): every lane holds the same sums;
//   factor    lane 0 scales, factors and inverts the 6x6 and stores the record.
// The camera set sits in LDS (a lane indexes it by its point's camera).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <new>

#include "../../include/ctag_pose.h"
#include "ctag_cov_src.h"
#include "ctag_internal.h"
#include "ctag_pose_dev.h"
#include "ctag_schur6.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_pose_cov_rec) == 352, "ctag_pose_cov_rec layout");
static_assert(sizeof(ctag_cov_opts) == 24, "ctag_cov_opts layout");

namespace ctag {

constexpr int kCovGrid = 256 * 16;               // wavefronts of one launch at most
constexpr double kCovMinPivot = 1e-12;

struct CovOpts {
    int param;
    double sigma_px, outlier_k;
};

struct CovLds {
    PoseCam cam[kMvCams];
    double R[kMvCams][9];
    double t[kMvCams][3];
    // where point i comes from: src = its descriptor (point_desc, ctag_pose_dev.h); model = the model index
    int32_t src[kCovMaxPts];
    int32_t model[kCovMaxPts];
    double norm[kCovMaxPts];  // residual norm of point i, written and read by its owner lane
};

// a record whose status is not CTAG_COV_OK: the status and 348 zero bytes, one 8-byte word per lane
__device__ __forceinline__ void cov_store_status(ctag_pose_cov_rec* P, int status, int lane) {
    if (lane < (int)(sizeof(ctag_pose_cov_rec) / 8)) reinterpret_cast<unsigned long long*>(P)[lane] = lane == 0 ? (unsigned long long)(unsigned)status : 0ull;
}

template <class Src>
__global__ __launch_bounds__(64) void k_pose_cov(Src src, PoseModelDev model, CovOpts opts, ctag_pose_cov_rec* __restrict__ out) {
    __shared__ CovLds L;
    const int lane = threadIdx.x;
    const int total = src.count();
    if ((int)blockIdx.x >= total) return;
    src.stage(L, lane);
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const typename Src::Rec& P = src.recs[w];
        ctag_pose_cov_rec* O = out + w;
        if (P.status != CTAG_POSE_OK) {  // wave-uniform, as every branch on the record below
            cov_store_status(O, CTAG_COV_NO_POSE, lane);
            continue;
        }
        wave_sync();  // the previous record's descriptors have been read (and the cameras are in LDS)
        int n = 0;
        double x[6];
        bool ok = src.build(P, model, L, lane, n) && n == P.n_points && n >= 4;
        ok = load_state6(P, x) && ok;
        if (!ok) {
            cov_store_status(O, CTAG_COV_BAD_RECORD, lane);
            continue;
        }
        wave_sync();
        double R[9], dR[27];
        ctl::angle_axis_rot(x, R, dR);
        if (opts.param == CTAG_COV_PARAM_TANGENT) {  // dR_k = [e_k]x R: row i of [e_k]x R is e_k x (the columns' entries)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                dR[0 + j] = 0.0;
                dR[3 + j] = -R[6 + j];
                dR[6 + j] = R[3 + j];
                dR[9 + j] = R[6 + j];
                dR[12 + j] = 0.0;
                dR[15 + j] = -R[j];
                dR[18 + j] = -R[3 + j];
                dR[21 + j] = R[j];
                dR[24 + j] = 0.0;
            }
        }
        // ---- lane l: points l, l+64, ... in order
        double H[21], ss = 0.0, worst = -1.0;
        int worst_i = INT_MAX;
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = 0.0;
        for (int i = lane; i < n; i += 64) {
            const int s = L.src[i], mi = L.model[i];
            const int c = desc_cam(s);
            const ctag_frame_result& FR = src.frame(P, c);
            double xn, yn, ob[2], X[3], r0, r1, j0[6], j1[6];
            corner_point(L.cam[c], model.corners + (size_t)mi * model.model_size * 24, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, X);
            if constexpr (Src::kMultiView)
                mv_point_residual(R, dR, x, L.cam[c], L.R[c], L.t[c], X, ob, r0, r1, j0, j1);
            else
                point_residual(R, dR, x, L.cam[c].fx, L.cam[c].fy, L.cam[c].cx, L.cam[c].cy, X, ob, r0, r1, j0, j1, true);
            gram6_add(j0, j1, H);
            const double r2 = r0 * r0 + r1 * r1;
            ss += r2;
            const double nrm = ctm::sqrt64(r2);
            L.norm[i] = nrm;
            if (nrm > worst) {  // ascending i: the first of equal norms stays
                worst = nrm;
                worst_i = i;
            }
        }
        // ---- one fixed tree over the lanes; every lane ends with the same values
#pragma unroll
        for (int e = 0; e < 21; e++) H[e] = wave_sum_f64(H[e]);
        ss = wave_sum_f64(ss);
        wave_max_f64(worst, worst_i);
        const int dof = 2 * n - 6;
        const double cost = 0.5 * ss;
        const double sigma2_hat = 2.0 * cost / (double)dof;
        const double sigma2_used = opts.sigma_px > 0.0 ? opts.sigma_px * opts.sigma_px : sigma2_hat;
        int n_out = 0;
        if (opts.outlier_k > 0.0) {
            const double bar = opts.outlier_k * ctm::sqrt64(sigma2_used);
            for (int i = lane; i < n; i += 64) n_out += L.norm[i] > bar ? 1 : 0;
            n_out = sg_sum<64>(n_out);
        }
        // ---- rule 5
        double d[6], C[36], inv[36], min_pivot = 0.0;
        bool good = ctl::finite64(cost);
        {
            int e = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double h = H[e];
                good = good && ctl::finite64(h) && h > 0.0;
                d[a] = 1.0 / ctm::sqrt64(h);
                e += 6 - a;
            }
            e = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) {
                    const double v = d[a] * H[e] * d[b];
                    C[a * 6 + b] = v;
                    C[b * 6 + a] = v;
                    e++;
                }
        }
        good = good && ctl::chol6_inverse(C, inv, kCovMinPivot, min_pivot);
        if (!good) {
            cov_store_status(O, CTAG_COV_SINGULAR, lane);
            continue;
        }
        if (lane == 0) {
            O->status = CTAG_COV_OK;
            O->n_points = n;
            O->dof = dof;
            O->worst_point = worst_i;
            O->n_outliers = n_out;
            O->param = opts.param;
            O->cost = cost;
            O->sigma2_hat = sigma2_hat;
            O->sigma2_used = sigma2_used;
            O->max_residual_px = worst;
            O->min_pivot = min_pivot;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) {
                    const double v = sigma2_used * (d[a] * inv[a * 6 + b] * d[b]);
                    O->cov[a * 6 + b] = v;
                    O->cov[b * 6 + a] = v;
                }
        }
    }
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
namespace {

struct CovState {  // scratch of the one-frame calls
    ctag::DevBuf<ctag_frame_result> d_result;  // one record per camera
    ctag::DevBuf<unsigned char> d_src;         // the source pose records
    ctag::DevBuf<int32_t> d_offsets;
    ctag::DevBuf<ctag_pose_cov_rec> d_out;
};

void cov_state_free(void* p) { delete static_cast<CovState*>(p); }

CovState* cov_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kCovState, cov_state_free);
    if (!*slot) *slot = new (std::nothrow) CovState();
    return static_cast<CovState*>(*slot);
}

// null: the defaults
int cov_opts(const ctag_cov_opts* o, ctag::CovOpts& r) {
    ctag_cov_opts d;
    ctag_cov_opts_default(&d);
    if (!o) o = &d;
    if (o->struct_size != sizeof(ctag_cov_opts)) return CTAG_ERR_ARG;
    if (o->param != CTAG_COV_PARAM_TANGENT && o->param != CTAG_COV_PARAM_RVEC) return CTAG_ERR_ARG;
    if (!ctl::finite64(o->sigma_px) || !ctl::finite64(o->outlier_k)) return CTAG_ERR_ARG;
    r.param = o->param;
    r.sigma_px = o->sigma_px;
    r.outlier_k = o->outlier_k;
    return CTAG_OK;
}

template <class Src>
int cov_launch(const Src& src, int n_records, const ctag::PoseModelDev& md, const ctag::CovOpts& opts, ctag_pose_cov_rec* out_dev, hipStream_t s) {
    hipLaunchKernelGGL(ctag::k_pose_cov<Src>, dim3(std::min(n_records, ctag::kCovGrid)), dim3(64), 0, s, src, md, opts, out_dev);
    return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

// host records to the one-frame scratch: the detection record(s), the source pose records and room for n_out results
template <class Rec>
int cov_upload(CovState* st, hipStream_t s, const ctag_frame_result* results, int n_results, const Rec* recs, int n_recs) {
    const size_t src_bytes = sizeof(Rec) * (size_t)n_recs;
    if (st->d_src.cap < src_bytes || st->d_out.cap < (size_t)n_recs) {  // an earlier call's kernel may still read the old buffers
        if ((st->d_src.p || st->d_out.p) && hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
        if (st->d_src.grow(src_bytes) != hipSuccess || st->d_out.grow((size_t)n_recs) != hipSuccess) return CTAG_ERR_HIP;
    }
    if (st->d_result.grow(CTAG_MV_MAX_CAMERAS) != hipSuccess || st->d_offsets.grow(2) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpyAsync(st->d_result.p, results, sizeof(ctag_frame_result) * (size_t)n_results, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(st->d_src.p, recs, src_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    return CTAG_OK;
}

int cov_download(CovState* st, hipStream_t s, ctag_pose_cov_rec* out, int n) {
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_pose_cov_rec) * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_cov_opts_default(ctag_cov_opts* o) {
    if (!o) return;
    o->struct_size = (uint32_t)sizeof(ctag_cov_opts);
    o->param = CTAG_COV_PARAM_TANGENT;
    o->sigma_px = 0.0;
    o->outlier_k = 3.0;
}

int ctag_pose_cov_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                               const ctag_camera* camera, const int32_t* offsets_dev, const ctag_pose_rec* poses_dev, int capacity,
                               const ctag_cov_opts* opts, ctag_pose_cov_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model || !offsets_dev || !poses_dev || capacity < 0 || !out_dev) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag::CovOpts o;
    if (cov_opts(opts, o) != CTAG_OK) return CTAG_ERR_ARG;
    if (n_frames == 0 || capacity == 0) return CTAG_OK;
    ctag::PoseModelDev md;
    hipStream_t s;
    const int rc = ctag::cov_prepare(h, model, md, s);
    if (rc != CTAG_OK) return rc;
    const ctag::CovMarkerSrc src{results_dev, n_frames, offsets_dev, poses_dev, capacity, ctag::make_pose_cam(camera)};
    return cov_launch(src, capacity, md, o, out_dev, s);
}

int ctag_rig_pose_cov_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                                   const ctag_rigs* rigs, const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses_dev,
                                   const ctag_cov_opts* opts, ctag_pose_cov_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model || !rigs || !rig_poses_dev || !out_dev) return CTAG_ERR_ARG;
    if (rigs->n_models != model->n_models) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag::CovOpts o;
    if (cov_opts(opts, o) != CTAG_OK) return CTAG_ERR_ARG;
    const long long n_items = (long long)n_frames * rigs->n_rigs;
    if (n_items > INT_MAX / 2) return CTAG_ERR_LIMIT;
    if (n_items == 0) return CTAG_OK;
    ctag::PoseModelDev md;
    hipStream_t s;
    const int rc = ctag::cov_prepare(h, model, md, s);
    if (rc != CTAG_OK) return rc;
    const ctag::CovRigSrc src{results_dev, n_frames, (int)n_items, rig_poses_dev, ctag::make_pose_cam(camera)};
    return cov_launch(src, (int)n_items, md, o, out_dev, s);
}

int ctag_mv_rig_pose_cov_batch_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_frames, const ctag_model* model,
                                      const ctag_rigs* rigs, const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses_dev,
                                      const ctag_cov_opts* opts, ctag_pose_cov_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model || !rigs || !cams || !mv_poses_dev || !out_dev) return CTAG_ERR_ARG;
    if (rigs->n_models != model->n_models) return CTAG_ERR_ARG;
    ctag::CovMvSrc src;
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) {
        src.res.p[c] = c < cams->dev.n ? results_dev[c] : nullptr;
        if (c < cams->dev.n && !src.res.p[c]) return CTAG_ERR_ARG;
    }
    ctag::CovOpts o;
    if (cov_opts(opts, o) != CTAG_OK) return CTAG_ERR_ARG;
    const long long n_items = (long long)n_frames * rigs->n_rigs;
    if (n_items > INT_MAX / 2) return CTAG_ERR_LIMIT;
    if (n_items == 0) return CTAG_OK;
    ctag::PoseModelDev md;
    hipStream_t s;
    const int rc = ctag::cov_prepare(h, model, md, s);
    if (rc != CTAG_OK) return rc;
    src.n_frames = n_frames;
    src.n_records = (int)n_items;
    src.recs = mv_poses_dev;
    src.cams = cams->dev;
    return cov_launch(src, (int)n_items, md, o, out_dev, s);
}

int ctag_estimate_pose_cov(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_camera* camera,
                           const ctag_pose_rec* poses, const ctag_cov_opts* opts, ctag_pose_cov_rec* out) {
    if (!h || !result || !model || !camera) return CTAG_ERR_ARG;
    if (result->status != CTAG_OK || result->n_markers <= 0) return CTAG_OK;
    if (!poses || !out || result->n_markers > CTAG_MAX_MARKERS) return CTAG_ERR_ARG;
    const int n = result->n_markers;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    CovState* st = cov_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    int rc = cov_upload(st, s, result, 1, poses, n);
    if (rc != CTAG_OK) return rc;
    const int32_t offsets[2] = {0, n};
    if (hipMemcpyAsync(st->d_offsets.p, offsets, sizeof(offsets), hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    rc = ctag_pose_cov_batch_device(h, st->d_result.p, 1, model, camera, st->d_offsets.p, reinterpret_cast<const ctag_pose_rec*>(st->d_src.p), n, opts,
                                    st->d_out.p);
    if (rc != CTAG_OK) return rc;
    return cov_download(st, s, out, n);
}

int ctag_estimate_rig_pose_cov(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_rigs* rigs,
                               const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses, const ctag_cov_opts* opts,
                               ctag_pose_cov_rec* out) {
    if (!h || !result || !model || !rigs || !camera || !rig_poses || !out) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    CovState* st = cov_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    int rc = cov_upload(st, s, result, 1, rig_poses, rigs->n_rigs);
    if (rc != CTAG_OK) return rc;
    rc = ctag_rig_pose_cov_batch_device(h, st->d_result.p, 1, model, rigs, camera, reinterpret_cast<const ctag_rig_pose_rec*>(st->d_src.p), opts,
                                        st->d_out.p);
    if (rc != CTAG_OK) return rc;
    return cov_download(st, s, out, rigs->n_rigs);
}

int ctag_estimate_mv_rig_pose_cov(ctag_handle* h, const ctag_frame_result* results, const ctag_model* model, const ctag_rigs* rigs,
                                  const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses, const ctag_cov_opts* opts,
                                  ctag_pose_cov_rec* out) {
    if (!h || !results || !model || !rigs || !cams || !mv_poses || !out) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    CovState* st = cov_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const int n = cams->dev.n;
    int rc = cov_upload(st, s, results, n, mv_poses, rigs->n_rigs);
    if (rc != CTAG_OK) return rc;
    const ctag_frame_result* ptrs[CTAG_MV_MAX_CAMERAS];
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) ptrs[c] = c < n ? st->d_result.p + c : nullptr;
    rc = ctag_mv_rig_pose_cov_batch_device(h, ptrs, 1, model, rigs, cams, reinterpret_cast<const ctag_mv_pose_rec*>(st->d_src.p), opts, st->d_out.p);
    if (rc != CTAG_OK) return rc;
    return cov_download(st, s, out, rigs->n_rigs);
}

}  // extern "C"
