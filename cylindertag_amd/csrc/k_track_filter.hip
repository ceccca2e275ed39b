// k_track_filter.hip -- the causal counterpart of k_track.hip: per rig an extended Kalman filter on (R, t, w, v) under the smoother's
// constant-velocity model, whose state stays in device memory between calls.  The semantics are stated in include/ctag_pose.h (track
// filtering, rules 1-10).
//
// Mapping.  One launch a call, one wavefront a rig.  The frames of the call are taken 64 at a time:
//   (a) lane = frame: rule 1 for 64 frames side by side (angle_axis_rot and the covariance's validity factorisation), Rm, tm and cov_f
//       into LDS (48 doubles a frame), the measured mask by a ballot; bad input is found by a scan over the whole call before that;
//   (b) the wave walks the 64 frames in order.  The pose, the velocities and every 3x3 / 6x6 quantity (E, Jl, phi, Jl^-1, S and its
//       factorisation) are wave-uniform: every lane computes the same value in registers.  The 12x12 P and the blocks derived from it
//       live in LDS under ctag_m12.h's convention: entry e belongs to lane e % 64, one order of summation, symmetric results computed
//       at (min, max).  F is 3x3-block sparse (six terms a row, not twelve), I - K H differs from I in six columns, S is 6x6;
//   (c) a record's 58 doubles are written by 58 lanes.
// A block is one wave: the phases are ordered by lds_wait(), not by a block barrier.  Everything is FP64 VALU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_tf_step.h"

static_assert(sizeof(ctag_track_rec) == 464, "ctag_track_rec layout");
static_assert(sizeof(ctag_track_filter_opts) == 72, "ctag_track_filter_opts layout");

namespace ctag {

constexpr int kTfStateDoubles = 164;  // P 144, R 9, t 3, w 3, v 3, t_prev, one spare
constexpr int kTfStateInts = 2;       // tracking, consecutive frames without an update
constexpr int kTfRecWords = 58;       // a ctag_track_rec in 8-byte words
// the per-frame step (rules 2-5), the pre-pass and their LDS layout: ctag_tf_step.h, shared with k_track_noise.hip

// one record: words 0-13 and 56, 57 from S.rec (lane 0 wrote them), the covariance and the velocity sigmas from S.P when `full`
__device__ __forceinline__ double words_as_double(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }

__device__ __forceinline__ void tf_write_rec(TfLds& S, double* __restrict__ out, bool full, int lane) {
    lds_wait();
    if (lane < kTfRecWords) {
        double val;
        if (lane < 14) {
            val = S.rec[lane];
        } else if (lane < 50) {
            const int r = (lane - 14) / 6, c = (lane - 14) % 6;
            val = full ? S.P.v[min(r, c) * 12 + max(r, c)] : 0.0;
        } else if (lane < 56) {
            const int d = lane - 44;
            val = full ? ctm::sqrt64(S.P.v[d * 12 + d]) : 0.0;
        } else {
            val = S.rec[lane - 42];
        }
        out[lane] = val;
    }
    lds_wait();
}

// predict_only: rule 7 -- one unmeasured frame at t0 for every rig, nothing stored
template <class Rec>
__global__ __launch_bounds__(64) void k_track_filter(const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov, int n_frames, int n_rigs,
                                                     const double* __restrict__ times, double t0, TfP p, double* __restrict__ state,
                                                     int32_t* __restrict__ istate, ctag_track_rec* __restrict__ out_recs, int predict_only) {
    __shared__ TfLds S;
    const int g = blockIdx.x, lane = threadIdx.x;
    double* __restrict__ out = reinterpret_cast<double*>(out_recs);
    // ---- rule 1's bad input, over the whole call ----
    if (!predict_only && tf_bad_input(recs, cov, n_frames, n_rigs, g, lane)) {
        for (long long idx = lane; idx < (long long)n_frames * kTfRecWords; idx += 64) {
            const int f = (int)(idx / kTfRecWords), wd = (int)(idx % kTfRecWords);
            const double val = wd == 0 ? words_as_double((uint32_t)CTAG_TRACK_BAD_INPUT, (uint32_t)g) : (wd == 1 ? words_as_double((uint32_t)f, 0u) : 0.0);
            out[((size_t)f * n_rigs + g) * kTfRecWords + wd] = val;
        }
        return;
    }
    // ---- the state: P into LDS, the rest wave-uniform ----
    double* __restrict__ st = state + (size_t)g * kTfStateDoubles;
    m_load(S.P, st, lane);
    m_identity(S.F, lane);
    double R[9], t[3], w[3], v[3], tprev;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = st[144 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = st[153 + k], w[k] = st[156 + k], v[k] = st[159 + k];
    tprev = st[162];
    int tracking = istate[g * kTfStateInts], misses = istate[g * kTfStateInts + 1];
    lds_wait();

    TfClk clk;
#if CTAG_TF_CLOCKS
    clk.last = wall_clock64();
#endif
    for (int f0 = 0; f0 < n_frames; f0 += 64) {  // wave-uniform
        // ---- (a) lane = frame ----
        const unsigned long long Mmask = tf_prepass(S, recs, cov, f0, n_frames, n_rigs, g, p.cov_scale, !predict_only, lane);
        const int cnt = min(64, n_frames - f0);
        TF_CLK(clk, 0);
        // ---- (b) the walk ----
        for (int kk = 0; kk < cnt; kk++) {  // wave-uniform
            const int f = f0 + kk;
            const double tf = times ? times[f] : t0;
            TfOut o;
            tf_step<false>(S, R, t, w, v, tprev, tracking, misses, p, ((Mmask >> kk) & 1ull) != 0ull, kk, tf, predict_only != 0, lane, clk, o);
            // ---- (c) the record ----
            if (lane == 0) {
                double rv[3] = {0.0, 0.0, 0.0};
                if (o.full) so3_log(R, rv);
                S.rec[0] = words_as_double((uint32_t)o.status, (uint32_t)g);
                S.rec[1] = words_as_double((uint32_t)(predict_only ? 0 : f), o.flags);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    S.rec[2 + k] = rv[k];
                    S.rec[5 + k] = o.full ? t[k] : 0.0;
                    S.rec[8 + k] = o.full ? w[k] : 0.0;
                    S.rec[11 + k] = o.full ? v[k] : 0.0;
                }
                S.rec[14] = o.full ? o.m2 : 0.0;
                S.rec[15] = o.full ? o.wt : 0.0;
            }
            tf_write_rec(S, out + ((size_t)(predict_only ? 0 : f) * n_rigs + g) * kTfRecWords, o.full, lane);
            TF_CLK(clk, 5);
        }
    }
#if CTAG_TF_CLOCKS
    if (g == 0 && lane == 0)
        printf("tf_clocks frames %d prepass %lld predict %lld innovation %lld gain %lld joseph %lld record %lld\n", n_frames, clk.c[0], clk.c[1], clk.c[2], clk.c[3],
               clk.c[4], clk.c[5]);
#endif
    if (predict_only) return;
    lds_wait();
    m_store(st, S.P, lane);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) st[144 + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) st[153 + k] = t[k], st[156 + k] = w[k], st[159 + k] = v[k];
        st[162] = tprev;
        istate[g * kTfStateInts] = tracking;
        istate[g * kTfStateInts + 1] = misses;
    }
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
struct ctag_track_filter {
    ctag_handle* h = nullptr;
    int n_rigs = 0;
    ctag::TfP P;
    double dt = 0.0;
    ctag::DevBuf<double> d_state, d_times[2];
    ctag::DevBuf<int32_t> d_istate;
    ctag::DevBuf<unsigned char> d_in;  // the host forms' records
    ctag::DevBuf<ctag_pose_cov_rec> d_cov;
    ctag::DevBuf<ctag_track_rec> d_out;
    std::vector<double> times[2];      // the times of the last two multi-frame calls, in turn: the caller's array may go once the call returns
    hipEvent_t done[2] = {nullptr, nullptr}, ev[2] = {nullptr, nullptr};  // done[k]: behind the call that used slot k
    bool in_flight[2] = {false, false}, timed = false, has_last = false;
    int slot = 0;
    float ms = 0.f;
    long long frames_given = 0;
    double last_time = 0.0;
};

namespace {

bool tf_pos_finite(double v) { return std::isfinite(v) && v > 0.0; }

hipStream_t tf_stream(ctag_track_filter* F) { return static_cast<hipStream_t>(ctag_stream(F->h)); }

int tf_clear(ctag_track_filter* F) {
    hipStream_t s = tf_stream(F);
    if (hipMemsetAsync(F->d_state.p, 0, sizeof(double) * (size_t)F->n_rigs * ctag::kTfStateDoubles, s) != hipSuccess ||
        hipMemsetAsync(F->d_istate.p, 0, sizeof(int32_t) * (size_t)F->n_rigs * ctag::kTfStateInts, s) != hipSuccess)
        return CTAG_ERR_HIP;
    F->frames_given = 0;
    F->has_last = false;
    return CTAG_OK;
}

// rule 9 for a step call's sizes and times, on the host and before anything is enqueued
int tf_step_args(const ctag_track_filter* F, int n_frames, const double* times) {
    if (n_frames < 1 || (long long)n_frames * F->n_rigs > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    if (times) {
        for (int f = 0; f < n_frames; f++) {
            if (!std::isfinite(times[f])) return CTAG_ERR_ARG;
            if (f > 0 ? !(times[f] > times[f - 1]) : (F->has_last && !(times[0] > F->last_time))) return CTAG_ERR_ARG;
        }
    } else if (F->has_last && !((double)F->frames_given * F->dt > F->last_time)) {
        return CTAG_ERR_ARG;
    }
    return CTAG_OK;
}

template <class Rec>
int tf_step_device(ctag_track_filter* F, const Rec* recs_dev, const ctag_pose_cov_rec* cov_dev, int n_frames, const double* times, ctag_track_rec* out_dev) {
    if (!F || !recs_dev || !cov_dev || !out_dev) return CTAG_ERR_ARG;
    if (tf_step_args(F, n_frames, times) != CTAG_OK) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = tf_stream(F);
    const double* T = nullptr;
    double t0 = 0.0, t_last;
    if (n_frames == 1) {  // a single time travels as a kernel argument
        t0 = times ? times[0] : (double)F->frames_given * F->dt;
        t_last = t0;
    } else {
        const int k = F->slot;  // two staging slots in turn: only the multi-frame call before the previous one is waited for
        if (F->in_flight[k] && hipEventSynchronize(F->done[k]) != hipSuccess) return CTAG_ERR_HIP;
        F->in_flight[k] = false;
        if (F->d_times[k].grow((size_t)n_frames) != hipSuccess) return CTAG_ERR_HIP;
        std::vector<double>& tt = F->times[k];
        tt.resize(n_frames);
        for (int f = 0; f < n_frames; f++) tt[f] = times ? times[f] : (double)(F->frames_given + f) * F->dt;
        if (hipMemcpyAsync(F->d_times[k].p, tt.data(), sizeof(double) * (size_t)n_frames, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
        T = F->d_times[k].p;
        t_last = tt[n_frames - 1];
    }
    const bool timing = ctag::handle_timing(F->h);
    F->timed = timing;
    if (timing && hipEventRecord(F->ev[0], s) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_track_filter<Rec>, dim3(F->n_rigs), dim3(64), 0, s, recs_dev, cov_dev, n_frames, F->n_rigs, T, t0, F->P, F->d_state.p,
                       F->d_istate.p, out_dev, 0);
    if (hipGetLastError() != hipSuccess) return CTAG_ERR_HIP;
    if (timing && hipEventRecord(F->ev[1], s) != hipSuccess) return CTAG_ERR_HIP;
    if (n_frames > 1) {
        if (hipEventRecord(F->done[F->slot], s) != hipSuccess) return CTAG_ERR_HIP;
        F->in_flight[F->slot] = true;
        F->slot ^= 1;
    }
    F->frames_given += n_frames;
    F->last_time = t_last;
    F->has_last = true;
    return CTAG_OK;
}

template <class Rec>
int tf_step_host(ctag_track_filter* F, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, const double* times, ctag_track_rec* out) {
    if (!F || !recs || !cov || !out) return CTAG_ERR_ARG;
    if (tf_step_args(F, n_frames, times) != CTAG_OK) return CTAG_ERR_ARG;  // a refused call enqueues nothing
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = tf_stream(F);
    const size_t n = (size_t)n_frames * F->n_rigs;  // every earlier host form has waited for its own work: the buffers are free
    if (F->d_in.grow(sizeof(Rec) * n) != hipSuccess || F->d_cov.grow(n) != hipSuccess || F->d_out.grow(n) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpyAsync(F->d_in.p, recs, sizeof(Rec) * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(F->d_cov.p, cov, sizeof(ctag_pose_cov_rec) * n, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    const int rc = tf_step_device<Rec>(F, reinterpret_cast<const Rec*>(F->d_in.p), F->d_cov.p, n_frames, times, F->d_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, F->d_out.p, sizeof(ctag_track_rec) * n, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_track_filter_opts_default(ctag_track_filter_opts* o) {
    if (!o) return;
    ctag_track_opts t;
    ctag_track_opts_default(&t);
    o->struct_size = (uint32_t)sizeof(ctag_track_filter_opts);
    o->loss = CTAG_TRACK_LOSS_NONE;
    o->max_gap = 5;
    o->reserved = 0;
    o->dt = 1.0 / 30.0;
    o->q_rot = t.q_rot;
    o->q_trans = t.q_trans;
    o->vel0_sigma_rot = t.vel0_sigma_rot;
    o->vel0_sigma_trans = t.vel0_sigma_trans;
    o->loss_scale = t.loss_scale;
    o->gate = 0.0;  // off: tools/track_filter_study.py found no gate of 3 .. 8 that spares every good frame at these q
}

int ctag_track_filter_create(ctag_handle* h, const ctag_rigs* rigs, const ctag_track_filter_opts* opts, ctag_track_filter** filter) {
    if (!h || !rigs || !filter) return CTAG_ERR_ARG;
    *filter = nullptr;
    ctag_track_filter_opts d;
    ctag_track_filter_opts_default(&d);
    const ctag_track_filter_opts* o = opts ? opts : &d;
    if (o->struct_size != sizeof(ctag_track_filter_opts)) return CTAG_ERR_ARG;
    if (o->loss != CTAG_LOSS_HUBER && o->loss != CTAG_LOSS_CAUCHY && o->loss != CTAG_TRACK_LOSS_NONE) return CTAG_ERR_ARG;
    if (o->max_gap < 1 || rigs->n_rigs < 1 || rigs->n_rigs > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    for (double v : {o->dt, o->q_rot, o->q_trans, o->vel0_sigma_rot, o->vel0_sigma_trans, o->loss_scale})
        if (!tf_pos_finite(v)) return CTAG_ERR_ARG;
    if (!std::isfinite(o->gate) || o->gate < 0.0) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    ctag_track_filter* F = new (std::nothrow) ctag_track_filter();
    if (!F) return CTAG_ERR_HIP;
    F->h = h;
    F->n_rigs = rigs->n_rigs;
    F->dt = o->dt;
    F->P.loss = o->loss;
    F->P.max_gap = o->max_gap;
    F->P.q_rot = o->q_rot;
    F->P.q_trans = o->q_trans;
    F->P.vr2 = o->vel0_sigma_rot * o->vel0_sigma_rot;
    F->P.vt2 = o->vel0_sigma_trans * o->vel0_sigma_trans;
    F->P.a = o->loss_scale;
    F->P.a2 = o->loss_scale * o->loss_scale;
    F->P.gate2 = o->gate * o->gate;
    F->P.cov_scale = 1.0;
    bool ok = F->d_state.grow((size_t)F->n_rigs * ctag::kTfStateDoubles) == hipSuccess && F->d_istate.grow((size_t)F->n_rigs * ctag::kTfStateInts) == hipSuccess &&
              F->d_out.grow((size_t)F->n_rigs) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&F->done[0], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&F->done[1], hipEventDisableTiming) == hipSuccess && hipEventCreate(&F->ev[0]) == hipSuccess &&
         hipEventCreate(&F->ev[1]) == hipSuccess && tf_clear(F) == CTAG_OK;
    if (!ok) {
        ctag_track_filter_free(F);
        return CTAG_ERR_HIP;
    }
    *filter = F;
    return CTAG_OK;
}

void ctag_track_filter_free(ctag_track_filter* F) {
    if (!F) return;
    (void)hipSetDevice(ctag::handle_device(F->h));
    (void)hipStreamSynchronize(tf_stream(F));  // nothing may still read the state or the times
    for (auto& e : F->done)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : F->ev)
        if (e) (void)hipEventDestroy(e);
    delete F;
}

int ctag_track_filter_set_cov_scale(ctag_track_filter* F, double s) {
    if (!F || !tf_pos_finite(s)) return CTAG_ERR_ARG;
    F->P.cov_scale = s;  // a kernel argument: calls already enqueued keep the value they were given
    return CTAG_OK;
}

int ctag_track_filter_reset(ctag_track_filter* F) {
    if (!F) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    return tf_clear(F);
}

int ctag_rig_track_filter_device(ctag_track_filter* F, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev, int n_frames,
                                 const double* times, ctag_track_rec* out_dev) {
    return tf_step_device<ctag_rig_pose_rec>(F, rig_poses_dev, cov_dev, n_frames, times, out_dev);
}

int ctag_mv_rig_track_filter_device(ctag_track_filter* F, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev, int n_frames,
                                    const double* times, ctag_track_rec* out_dev) {
    return tf_step_device<ctag_mv_pose_rec>(F, mv_poses_dev, cov_dev, n_frames, times, out_dev);
}

int ctag_rig_track_filter(ctag_track_filter* F, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                          ctag_track_rec* out) {
    return tf_step_host<ctag_rig_pose_rec>(F, rig_poses, cov, n_frames, times, out);
}

int ctag_mv_rig_track_filter(ctag_track_filter* F, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                             ctag_track_rec* out) {
    return tf_step_host<ctag_mv_pose_rec>(F, mv_poses, cov, n_frames, times, out);
}

int ctag_track_filter_predict_device(ctag_track_filter* F, double t, ctag_track_rec* out_dev) {
    if (!F || !out_dev || !std::isfinite(t) || (F->has_last && !(t > F->last_time))) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipLaunchKernelGGL(ctag::k_track_filter<ctag_rig_pose_rec>, dim3(F->n_rigs), dim3(64), 0, tf_stream(F), (const ctag_rig_pose_rec*)nullptr,
                       (const ctag_pose_cov_rec*)nullptr, 1, F->n_rigs, (const double*)nullptr, t, F->P, F->d_state.p, F->d_istate.p, out_dev, 1);
    return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

int ctag_track_filter_predict(ctag_track_filter* F, double t, ctag_track_rec* out) {
    if (!F || !out) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(F->h)) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = tf_stream(F);
    if (hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;  // d_out is the host forms' buffer: nothing reads it now
    if (F->d_out.grow((size_t)F->n_rigs) != hipSuccess) return CTAG_ERR_HIP;
    const int rc = ctag_track_filter_predict_device(F, t, F->d_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, F->d_out.p, sizeof(ctag_track_rec) * (size_t)F->n_rigs, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

int ctag_track_filter_last_ms(ctag_track_filter* F, float* out1) {
    if (!F || !out1) return CTAG_ERR_ARG;
    if (F->timed) {
        F->timed = false;
        F->ms = 0.f;
        if (hipEventSynchronize(F->ev[1]) == hipSuccess) (void)hipEventElapsedTime(&F->ms, F->ev[0], F->ev[1]);
    }
    *out1 = F->ms;
    return CTAG_OK;
}

}  // extern "C"
