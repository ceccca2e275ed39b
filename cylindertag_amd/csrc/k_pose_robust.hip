// k_pose_robust.hip -- finished pose records (per marker, per rig, per rig from several cameras) minimised again under Ceres' Huber or
// Cauchy loss, on the device, from the pose records and the detection records where they lie.  The semantics are stated in
// include/ctag_pose.h (robust refit, rules 1-9).
//
// Mapping: one kernel body, k_pose_robust<Src>, for the three record kinds; Src (ctag_cov_src.h, shared with
// k_pose_cov.hip) says where a record's frames and members are.  One wavefront per source record for every size (4 .. 800 points),
// grid-stride over the records.
//   walk      the whole wave walks the record's members and leaves one descriptor per point in LDS, as k_pose_cov does;
//   cache     lane l takes points l, l+64, ... in order: corner_point (load + five undistortion steps) ONCE, and leaves the model
//             point, the float-rounded observation (both are float values: 20 bytes) and the camera index in LDS.  Every evaluation
//             after that -- up to 51 of them -- reads only this;
//   scale     s_i of every point at the source pose to LDS (over the descriptors, which are done with); the lower median by rank
//             counting: a lane keeps its own s_i in registers and all lanes read every s_j once (a broadcast read), ties by index, so
//             the ranks are a permutation and exactly one lane holds the median;
//   loop      PoseBA's loop as ctag_pose_dev.h's pose_ba states it.  An evaluation forms 28 sums -- 21 of J^T W J, 6 of J^T W r, the cost
//             (the six column norms of the first evaluation are the diagonal of its J^T W J) -- each lane over its own points in FP64
//             registers, then one fixed tree over the lanes (wave_sum_f64): every lane holds the same sums, and the 6x6 solve and the
//             trust-region bookkeeping are wave-uniform;
//   report    s_i at the final pose (when a step was accepted), the mask words by lanes 0..24, the record by lane 0.
// The camera set sits in LDS (a lane indexes it by its point's camera).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <new>

#include "../../include/ctag_pose.h"
#include "ctag_cov_src.h"
#include "ctag_internal.h"
#include "ctag_loss.h"
#include "ctag_pose_dev.h"
#include "ctag_schur6.h"
#include "ctag_wave.h"

static_assert(sizeof(ctag_robust_pose_rec) == 232, "ctag_robust_pose_rec layout");
static_assert(sizeof(ctag_robust_opts) == 40, "ctag_robust_opts layout");

namespace ctag {

constexpr int kRobustGrid = 256 * 16;  // wavefronts of one launch at most
constexpr int kRobustMaxIter = 50;
constexpr int kRobustPer = (kCovMaxPts + 63) / 64;  // points of one lane at most
constexpr int kRobustMaskWords = 25;
static_assert(kRobustMaskWords * 32 >= kCovMaxPts && kRobustMaskWords <= 64, "one lane per mask word");
constexpr double kRayleighMedian = 1.1774100225154747;  // sqrt(2 ln 2)

struct RobustOpts {
    int loss, max_iterations;
    double scale_px, auto_k, min_scale_px;
};

struct RobustLds {
    PoseCam cam[kMvCams];
    double R[kMvCams][9];
    double t[kMvCams][3];
    // point i as every evaluation reads it, one array per component (lanes read neighbouring words: no bank conflict)
    float X[3][kCovMaxPts];
    float ob[2][kCovMaxPts];
    uint8_t pc[kCovMaxPts];
    union {
        struct {  // the walk: where point i comes from (point_desc, ctag_pose_dev.h) and its model index; read once, by the cache pass
            int32_t src[kCovMaxPts];
            int32_t model[kCovMaxPts];
        };
        double s2[kCovMaxPts];  // after it: s_i at the pose last reported on
    };
    double med;
};

// a record whose status is not CTAG_ROBUST_OK: the status and 228 zero bytes, one 8-byte word per lane
__device__ __forceinline__ void robust_store_status(ctag_robust_pose_rec* P, int status, int lane) {
    if (lane < (int)(sizeof(ctag_robust_pose_rec) / 8)) reinterpret_cast<unsigned long long*>(P)[lane] = lane == 0 ? (unsigned long long)(unsigned)status : 0ull;
}

template <class Src>
__global__ __launch_bounds__(64) void k_pose_robust(Src src, PoseModelDev model, RobustOpts opts, ctag_robust_pose_rec* __restrict__ out) {
    __shared__ RobustLds L;
    const int lane = threadIdx.x;
    const int total = src.count();
    if ((int)blockIdx.x >= total) return;
    src.stage(L, lane);
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const typename Src::Rec& P = src.recs[w];
        ctag_robust_pose_rec* O = out + w;
        if (P.status != CTAG_POSE_OK) {  // wave-uniform, as every branch on the record below
            robust_store_status(O, CTAG_ROBUST_NO_POSE, lane);
            continue;
        }
        wave_sync();  // the previous record's LDS image has been read (and the cameras are in LDS)
        int n = 0;
        double x[6];
        bool ok = src.build(P, model, L, lane, n) && n == P.n_points && n >= 4;
        ok = load_state6(P, x) && ok;
        if (!ok) {
            robust_store_status(O, CTAG_ROBUST_BAD_RECORD, lane);
            continue;
        }
        wave_sync();
        // ---- cache: lane l's points l, l+64, ...
        for (int i = lane; i < n; i += 64) {
            const int s = L.src[i], mi = L.model[i];
            const int c = desc_cam(s);
            const ctag_frame_result& FR = src.frame(P, c);
            double xn, yn, ob[2], X[3];
            corner_point(L.cam[c], model.corners + (size_t)mi * model.model_size * 24, FR.features[desc_feature(s)], desc_pos(s), desc_q(s), xn, yn, ob, X);
#pragma unroll
            for (int k = 0; k < 3; k++) L.X[k][i] = (float)X[k];  // float values both: nothing is rounded
            L.ob[0][i] = (float)ob[0];
            L.ob[1][i] = (float)ob[1];
            L.pc[i] = (uint8_t)c;
        }
        wave_sync();  // the descriptors have been read: s2 may take their place
        auto point = [&](int i, const double* R, const double* dR, const double* y, double& r0, double& r1, double* j0, double* j1) {
            const int c = L.pc[i];
            const double X[3] = {(double)L.X[0][i], (double)L.X[1][i], (double)L.X[2][i]};
            const double ob[2] = {(double)L.ob[0][i], (double)L.ob[1][i]};
            if constexpr (Src::kMultiView)
                mv_point_residual(R, dR, y, L.cam[c], L.R[c], L.t[c], X, ob, r0, r1, j0, j1);
            else
                point_residual(R, dR, y, L.cam[c].fx, L.cam[c].fy, L.cam[c].cx, L.cam[c].cy, X, ob, r0, r1, j0, j1, true);
        };
        // s_i at pose y to LDS; 0.5 sum s_i, the largest norm and its index (the same in every lane)
        double worst;
        int worst_i;
        auto report = [&](const double* y) -> double {
            double R[9], dR[27];
            ctl::angle_axis_rot(y, R, dR);
            double ss = 0.0;
            worst = -1.0;
            worst_i = INT_MAX;
            for (int i = lane; i < n; i += 64) {
                double r0, r1, j0[6], j1[6];
                point(i, R, dR, y, r0, r1, j0, j1);
                const double s = r0 * r0 + r1 * r1;
                L.s2[i] = s;
                ss += s;
                const double nrm = ctm::sqrt64(s);
                if (nrm > worst) {  // ascending i: the first of equal norms stays
                    worst = nrm;
                    worst_i = i;
                }
            }
            ss = wave_sum_f64(ss);
            wave_max_f64(worst, worst_i);
            wave_sync();
            return 0.5 * ss;
        };
        const double cost_ls0 = report(x);
        // ---- rule 4: the lower median of the norms by rank counting (sqrt is monotone: the median of the s_i, then its root)
        {
            const int want = (n - 1) / 2;
            double si[kRobustPer];
            int cnt[kRobustPer];
            if (lane == 0) L.med = 0.0;
#pragma unroll
            for (int k = 0; k < kRobustPer; k++) {
                const int i = lane + 64 * k;
                si[k] = i < n ? L.s2[i] : 0.0;
                cnt[k] = 0;
            }
            wave_sync();
            for (int j = 0; j < n; j++) {
                const double sj = L.s2[j];
#pragma unroll
                for (int k = 0; k < kRobustPer; k++) cnt[k] += (sj < si[k] || (sj == si[k] && j < lane + 64 * k)) ? 1 : 0;
            }
#pragma unroll
            for (int k = 0; k < kRobustPer; k++)
                if (lane + 64 * k < n && cnt[k] == want) L.med = si[k];
            wave_sync();
        }
        const double sigma_hat = ctm::sqrt64(L.med) / kRayleighMedian;
        double a = opts.scale_px;
        if (!(a > 0.0)) {
            a = opts.auto_k * sigma_hat;
            if (!(a > opts.min_scale_px)) a = opts.min_scale_px;
        }
        const double a2 = a * a;
        // ---- one evaluation at pose y: H = J^T W J (upper triangle, 21), g = J^T W r, both of the rows scaled by `scale`; the cost
        double scale[6] = {1, 1, 1, 1, 1, 1};
        auto eval = [&](const double* y, double* H, double* g) -> double {
            double R[9], dR[27];
            ctl::angle_axis_rot(y, R, dR);
            double c = 0.0;
#pragma unroll
            for (int e = 0; e < 21; e++) H[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) g[e] = 0.0;
            for (int i = lane; i < n; i += 64) {
                double r0, r1, j0[6], j1[6], rho, wt;
                point(i, R, dR, y, r0, r1, j0, j1);
                robust_loss(opts.loss, a, a2, r0 * r0 + r1 * r1, rho, wt);
                const double sw = ctm::sqrt64(wt);
#pragma unroll
                for (int e = 0; e < 6; e++) {
                    j0[e] = (j0[e] * sw) * scale[e];
                    j1[e] = (j1[e] * sw) * scale[e];
                }
                gram6_add(j0, j1, H);
                grad6_add(j0, j1, r0 * sw, r1 * sw, g);
                c += rho;
            }
#pragma unroll
            for (int e = 0; e < 21; e++) H[e] = wave_sum_f64(H[e]);
#pragma unroll
            for (int e = 0; e < 6; e++) g[e] = wave_sum_f64(g[e]);
            return 0.5 * wave_sum_f64(c);
        };
        auto gradient_max = [&](const double* g) {
            double m = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) {
                const double v = ctm::fabs64(g[e] / scale[e]);
                if (v > m) m = v;
            }
            return m;
        };
        double H[21], g[6];
        double cost = eval(x, H, g);
        const double cost0 = cost;
        if (!ctl::finite64(cost0)) {
            robust_store_status(O, CTAG_ROBUST_DEGENERATE, lane);
            continue;
        }
        // Jacobi scaling from the first evaluation: the column norms are the diagonal of its H
        {
            int e = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                scale[k] = 1.0 / (1.0 + ctm::sqrt64(H[e]));
                e += 6 - k;
            }
            e = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
#pragma unroll
                for (int c = k; c < 6; c++) H[e++] *= scale[k] * scale[c];
                g[k] *= scale[k];
            }
        }
        bool live = gradient_max(g) > 1e-15;
        bool moved = false;
        int iter = 0;
        double radius = 1e4, decrease_factor = 2.0;
        while (live && iter < opts.max_iterations) {
            iter++;
            if (radius < 1e-32) break;
            double Hf[36], A[36], rhs[6], delta[6];
            {
                int e = 0;
#pragma unroll
                for (int k = 0; k < 6; k++)
#pragma unroll
                    for (int c = k; c < 6; c++) {
                        Hf[k * 6 + c] = H[e];
                        Hf[c * 6 + k] = H[e];
                        e++;
                    }
            }
#pragma unroll
            for (int k = 0; k < 36; k++) A[k] = Hf[k];
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double d = Hf[k * 6 + k];
                d = d < 1e-6 ? 1e-6 : (d > 1e32 ? 1e32 : d);
                A[k * 6 + k] += d / radius;
                rhs[k] = -g[k];
            }
            ok = ctl::chol6_solve(A, rhs, delta);
            double model_cost_change = 0.0;
            if (ok) {
                double dg = 0.0, dHd = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    dg += delta[k] * g[k];
                    double hd = 0.0;
#pragma unroll
                    for (int c = 0; c < 6; c++) hd += Hf[k * 6 + c] * delta[c];
                    dHd += delta[k] * hd;
                }
                model_cost_change = -(dg + 0.5 * dHd);
#pragma unroll
                for (int k = 0; k < 6; k++) ok = ok && ctl::finite64(delta[k]);
            }
            if (!ok || !(model_cost_change > 0.0)) {
                radius = radius / decrease_factor;
                decrease_factor *= 2.0;
                continue;
            }
            double xc[6], step2 = 0.0, x2 = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const double du = delta[k] * scale[k];
                xc[k] = x[k] + du;
                step2 += du * du;
                x2 += x[k] * x[k];
            }
            double Hc[21], gc[6];
            const double cost_c = eval(xc, Hc, gc);
            const bool finite = ctl::finite64(cost_c);
            if (ctm::sqrt64(step2) <= 1e-10 * (ctm::sqrt64(x2) + 1e-10)) break;
            const double cost_change = cost - cost_c;
            if (finite && ctm::fabs64(cost_change) <= 1e-15 * cost) break;
            const double rho = cost_change / model_cost_change;
            if (finite && rho > 1e-3) {
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    x[k] = xc[k];
                    g[k] = gc[k];
                }
#pragma unroll
                for (int e = 0; e < 21; e++) H[e] = Hc[e];
                cost = cost_c;
                moved = true;
                const double t = 2.0 * rho - 1.0;
                double f = 1.0 - t * t * t;
                if (f < 1.0 / 3.0) f = 1.0 / 3.0;
                radius = radius / f;
                if (radius > 1e16) radius = 1e16;
                decrease_factor = 2.0;
                if (gradient_max(g) <= 1e-15) break;
            } else {
                radius = radius / decrease_factor;
                decrease_factor *= 2.0;
            }
        }
        // ---- rule 7 at the final pose
        double cost_ls = cost_ls0;
        if (moved) cost_ls = report(x);
        int n_in = 0;
        if (lane < kRobustMaskWords) {
            uint32_t m = 0u;
            for (int b = 0; b < 32; b++) {
                const int i = 32 * lane + b;
                if (i < n && L.s2[i] <= a2) m |= 1u << b;
            }
            O->inlier_mask[lane] = m;
            n_in = __popc(m);
        }
        n_in = sg_sum<64>(n_in);
        if (lane == 0) {
            O->status = CTAG_ROBUST_OK;
            O->n_points = n;
            O->n_inliers = n_in;
            O->iterations = iter;
            O->loss = opts.loss;
            O->worst_point = worst_i;
            O->reserved = 0;
            O->scale_px = a;
            O->sigma_hat = sigma_hat;
            O->cost_ls0 = cost_ls0;
            O->cost_ls = cost_ls;
            O->cost0 = cost0;
            O->cost = cost;
            O->max_residual_px = worst;
            for (int k = 0; k < 3; k++) {
                O->rvec[k] = x[k];  // the source's bytes when no step was accepted
                O->tvec[k] = x[3 + k];
            }
        }
    }
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
namespace {

struct RobustState {  // scratch of the one-frame calls
    ctag::DevBuf<ctag_frame_result> d_result;  // one record per camera
    ctag::DevBuf<unsigned char> d_src;         // the source pose records
    ctag::DevBuf<int32_t> d_offsets;
    ctag::DevBuf<ctag_robust_pose_rec> d_out;
};

void robust_state_free(void* p) { delete static_cast<RobustState*>(p); }

RobustState* robust_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kRobustState, robust_state_free);
    if (!*slot) *slot = new (std::nothrow) RobustState();
    return static_cast<RobustState*>(*slot);
}

// rule 9; null: the defaults
int robust_opts(const ctag_robust_opts* o, ctag::RobustOpts& r) {
    ctag_robust_opts d;
    ctag_robust_opts_default(&d);
    if (!o) o = &d;
    if (o->struct_size != sizeof(ctag_robust_opts)) return CTAG_ERR_ARG;
    if (o->loss != CTAG_LOSS_HUBER && o->loss != CTAG_LOSS_CAUCHY) return CTAG_ERR_ARG;
    if (o->max_iterations < 0 || o->max_iterations > ctag::kRobustMaxIter) return CTAG_ERR_ARG;
    if (!ctl::finite64(o->scale_px) || !ctl::finite64(o->auto_k) || !ctl::finite64(o->min_scale_px)) return CTAG_ERR_ARG;
    if (o->scale_px <= 0.0 && (o->auto_k <= 0.0 || o->min_scale_px <= 0.0)) return CTAG_ERR_ARG;
    r.loss = o->loss;
    r.max_iterations = o->max_iterations;
    r.scale_px = o->scale_px;
    r.auto_k = o->auto_k;
    r.min_scale_px = o->min_scale_px;
    return CTAG_OK;
}

template <class Src>
int robust_launch(const Src& src, int n_records, const ctag::PoseModelDev& md, const ctag::RobustOpts& opts, ctag_robust_pose_rec* out_dev, hipStream_t s) {
    hipLaunchKernelGGL(ctag::k_pose_robust<Src>, dim3(std::min(n_records, ctag::kRobustGrid)), dim3(64), 0, s, src, md, opts, out_dev);
    return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

// host records to the one-frame scratch: the detection record(s), the source pose records and room for n_recs results
template <class Rec>
int robust_upload(RobustState* st, hipStream_t s, const ctag_frame_result* results, int n_results, const Rec* recs, int n_recs) {
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

int robust_download(RobustState* st, hipStream_t s, ctag_robust_pose_rec* out, int n) {
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_robust_pose_rec) * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_robust_opts_default(ctag_robust_opts* o) {
    if (!o) return;
    o->struct_size = (uint32_t)sizeof(ctag_robust_opts);
    o->loss = CTAG_LOSS_CAUCHY;
    o->max_iterations = ctag::kRobustMaxIter;
    o->reserved = 0;
    o->scale_px = 0.0;
    o->auto_k = 2.5;
    o->min_scale_px = 0.05;
}

int ctag_pose_robust_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                                  const ctag_camera* camera, const int32_t* offsets_dev, const ctag_pose_rec* poses_dev, int capacity,
                                  const ctag_robust_opts* opts, ctag_robust_pose_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model || !offsets_dev || !poses_dev || capacity < 0 || !out_dev) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag::RobustOpts o;
    if (robust_opts(opts, o) != CTAG_OK) return CTAG_ERR_ARG;
    if (n_frames == 0 || capacity == 0) return CTAG_OK;
    ctag::PoseModelDev md;
    hipStream_t s;
    const int rc = ctag::cov_prepare(h, model, md, s);
    if (rc != CTAG_OK) return rc;
    const ctag::CovMarkerSrc src{results_dev, n_frames, offsets_dev, poses_dev, capacity, ctag::make_pose_cam(camera)};
    return robust_launch(src, capacity, md, o, out_dev, s);
}

int ctag_rig_pose_robust_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                                      const ctag_rigs* rigs, const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses_dev,
                                      const ctag_robust_opts* opts, ctag_robust_pose_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model || !rigs || !rig_poses_dev || !out_dev) return CTAG_ERR_ARG;
    if (rigs->n_models != model->n_models) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    ctag::RobustOpts o;
    if (robust_opts(opts, o) != CTAG_OK) return CTAG_ERR_ARG;
    const long long n_items = (long long)n_frames * rigs->n_rigs;
    if (n_items > INT_MAX / 2) return CTAG_ERR_LIMIT;
    if (n_items == 0) return CTAG_OK;
    ctag::PoseModelDev md;
    hipStream_t s;
    const int rc = ctag::cov_prepare(h, model, md, s);
    if (rc != CTAG_OK) return rc;
    const ctag::CovRigSrc src{results_dev, n_frames, (int)n_items, rig_poses_dev, ctag::make_pose_cam(camera)};
    return robust_launch(src, (int)n_items, md, o, out_dev, s);
}

int ctag_mv_rig_pose_robust_batch_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_frames, const ctag_model* model,
                                         const ctag_rigs* rigs, const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses_dev,
                                         const ctag_robust_opts* opts, ctag_robust_pose_rec* out_dev) {
    if (!h || !results_dev || n_frames < 0 || !model || !rigs || !cams || !mv_poses_dev || !out_dev) return CTAG_ERR_ARG;
    if (rigs->n_models != model->n_models) return CTAG_ERR_ARG;
    ctag::CovMvSrc src;
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) {
        src.res.p[c] = c < cams->dev.n ? results_dev[c] : nullptr;
        if (c < cams->dev.n && !src.res.p[c]) return CTAG_ERR_ARG;
    }
    ctag::RobustOpts o;
    if (robust_opts(opts, o) != CTAG_OK) return CTAG_ERR_ARG;
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
    return robust_launch(src, (int)n_items, md, o, out_dev, s);
}

int ctag_estimate_pose_robust(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_camera* camera,
                              const ctag_pose_rec* poses, const ctag_robust_opts* opts, ctag_robust_pose_rec* out) {
    if (!h || !result || !model || !camera) return CTAG_ERR_ARG;
    if (result->status != CTAG_OK || result->n_markers <= 0) return CTAG_OK;
    if (!poses || !out || result->n_markers > CTAG_MAX_MARKERS) return CTAG_ERR_ARG;
    const int n = result->n_markers;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    RobustState* st = robust_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    int rc = robust_upload(st, s, result, 1, poses, n);
    if (rc != CTAG_OK) return rc;
    const int32_t offsets[2] = {0, n};
    if (hipMemcpyAsync(st->d_offsets.p, offsets, sizeof(offsets), hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    rc = ctag_pose_robust_batch_device(h, st->d_result.p, 1, model, camera, st->d_offsets.p, reinterpret_cast<const ctag_pose_rec*>(st->d_src.p), n, opts,
                                       st->d_out.p);
    if (rc != CTAG_OK) return rc;
    return robust_download(st, s, out, n);
}

int ctag_estimate_rig_pose_robust(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_rigs* rigs,
                                  const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses, const ctag_robust_opts* opts,
                                  ctag_robust_pose_rec* out) {
    if (!h || !result || !model || !rigs || !camera || !rig_poses || !out) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    RobustState* st = robust_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    int rc = robust_upload(st, s, result, 1, rig_poses, rigs->n_rigs);
    if (rc != CTAG_OK) return rc;
    rc = ctag_rig_pose_robust_batch_device(h, st->d_result.p, 1, model, rigs, camera, reinterpret_cast<const ctag_rig_pose_rec*>(st->d_src.p), opts,
                                           st->d_out.p);
    if (rc != CTAG_OK) return rc;
    return robust_download(st, s, out, rigs->n_rigs);
}

int ctag_estimate_mv_rig_pose_robust(ctag_handle* h, const ctag_frame_result* results, const ctag_model* model, const ctag_rigs* rigs,
                                     const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses, const ctag_robust_opts* opts,
                                     ctag_robust_pose_rec* out) {
    if (!h || !results || !model || !rigs || !cams || !mv_poses || !out) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    RobustState* st = robust_state(h);
    if (!st) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const int n = cams->dev.n;
    int rc = robust_upload(st, s, results, n, mv_poses, rigs->n_rigs);
    if (rc != CTAG_OK) return rc;
    const ctag_frame_result* ptrs[CTAG_MV_MAX_CAMERAS];
    for (int c = 0; c < CTAG_MV_MAX_CAMERAS; c++) ptrs[c] = c < n ? st->d_result.p + c : nullptr;
    rc = ctag_mv_rig_pose_robust_batch_device(h, ptrs, 1, model, rigs, cams, reinterpret_cast<const ctag_mv_pose_rec*>(st->d_src.p), opts, st->d_out.p);
    if (rc != CTAG_OK) return rc;
    return robust_download(st, s, out, rigs->n_rigs);
}

}  // extern "C"
