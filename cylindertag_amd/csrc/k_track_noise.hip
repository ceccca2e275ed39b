// k_track_noise.hip -- the track noise fit: q_rot, q_trans and the covariance scale of the track filter by maximum likelihood on the
// filter's own innovations over a recorded batch.  The semantics are stated in include/ctag_pose.h (track noise fit, rules 1-11).
//
// Mapping.  k_track_noise: one wavefront per (candidate, rig) item, a grid-stride loop over the items.  An item is the
// filter's walk (ctag_tf_step.h: the lane = frame pre-pass 64 frames at a time into LDS, then the wave-uniform step with P in LDS) from an
// EMPTY track; no state is loaded or stored and no record is written: four sums an item, L = sum of log det S + d^2 over the updates in
// frame order among them.  k_track_noise_select: one block per search and one launch per round; it makes the pooled sums in rig order,
// the argmin, the trace row, the next round's candidates and, when the search ends, the result record.  A fit is rounds x (score, select)
// launches behind one another on the handle's stream; the host waits for none of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_tf_step.h"

static_assert(sizeof(ctag_track_noise_opts) == 80, "ctag_track_noise_opts layout");
static_assert(sizeof(ctag_track_noise_rec) == 96, "ctag_track_noise_rec layout");
static_assert(sizeof(ctag_track_noise_round) == 64, "ctag_track_noise_round layout");
static_assert(sizeof(ctag_track_noise_score) == 32, "ctag_track_noise_score layout");

namespace ctag {

constexpr int kNoiseMaxCand = 125;     // 5^3
constexpr int kNoiseMaxBlocks = 1024;  // 256 CUs x 4 SIMDs, one wave each: more items take the grid-stride loop
constexpr double kLn2 = 0.6931471805599453;

struct NoiseSel {
    int mode, free_mask, n_free, n_cand, rounds, min_terms, n_rigs;
    double start[3], span;
};

struct NoiseSearch {  // one per search, in device memory between the rounds
    double uc[3];
    double score_start;
    int32_t done, pad;
};

// cand: three doubles a candidate; item (c, g) reads candidate g * cand_rig_stride + c (the fit's per-rig searches have their own
// candidates, stride n_cand; a pooled search and a score call share them, stride 0).  out: entry c * n_rigs + g.
template <class Rec>
__global__ __launch_bounds__(64) void k_track_noise(const Rec* __restrict__ recs, const ctag_pose_cov_rec* __restrict__ cov, int n_frames, int n_rigs,
                                                    const double* __restrict__ times, TfP p, const double* __restrict__ cand, int n_cand,
                                                    int cand_rig_stride, ctag_track_noise_score* __restrict__ out) {
    __shared__ TfLds S;
    const int lane = threadIdx.x;
    const int n_items = n_cand * n_rigs;
    TfClk clk;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {  // wave-uniform
        const int c = item / n_rigs, g = item % n_rigs;
        const double* __restrict__ th = cand + ((size_t)g * cand_rig_stride + c) * 3;
        p.q_rot = th[0];
        p.q_trans = th[1];
        p.cov_scale = th[2];
        double L = 0.0, m2 = 0.0;
        int n_terms = 0, n_sing = 0;
        const bool bad = tf_bad_input(recs, cov, n_frames, n_rigs, g, lane);
        if (!bad) {
            double R[9], t[3], w[3], v[3], tprev = 0.0;  // EMPTY
            int tracking = 0, misses = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = 0.0, w[k] = 0.0, v[k] = 0.0;
            m_zero(S.P, lane);
            m_identity(S.F, lane);
            lds_wait();
            for (int f0 = 0; f0 < n_frames; f0 += 64) {  // wave-uniform
                const unsigned long long Mmask = tf_prepass(S, recs, cov, f0, n_frames, n_rigs, g, p.cov_scale, true, lane);
                const int cnt = min(64, n_frames - f0);
                for (int kk = 0; kk < cnt; kk++) {  // wave-uniform
                    TfOut o;
                    tf_step<true>(S, R, t, w, v, tprev, tracking, misses, p, ((Mmask >> kk) & 1ull) != 0ull, kk, times[f0 + kk], false, lane, clk, o);
                    if (o.updated) {
                        L += o.logdet + o.m2;
                        m2 += o.m2;
                        n_terms++;
                    } else if (o.status == CTAG_TRACK_SINGULAR) {
                        n_sing++;
                    }
                }
            }
        }
        if (lane == 0) {
            ctag_track_noise_score e;
            e.L = L;
            e.sum_m2 = m2;
            e.n_terms = n_terms;
            e.n_singular = n_sing;
            e.status = bad ? CTAG_NOISE_BAD_INPUT : CTAG_NOISE_OK;
            e.reserved = 0;
            out[item] = e;
        }
        lds_wait();
    }
}

__device__ __forceinline__ int pow5(int j) { return j == 0 ? 1 : (j == 1 ? 5 : 25); }

// the candidates of a round around uc with step h, by all lanes
__device__ __forceinline__ void noise_write_candidates(const NoiseSel& P, const double* uc, double h, double* __restrict__ cand, int lane) {
    for (int c = lane; c < P.n_cand; c += 64) {
        int j = 0;
        for (int a = 0; a < 3; a++) {
            double u = uc[a];
            if ((P.free_mask >> a) & 1) {
                u = uc[a] + (double)((c / pow5(j)) % 5 - 2) * h;
                j++;
            }
            cand[c * 3 + a] = P.start[a] * ctm::exp64(u * kLn2);
        }
    }
}

// r = -1: every search starts at u = 0 and round 0's candidates are written.  r >= 0: round r is decided from sc, the scores of its candidates.
__global__ __launch_bounds__(64) void k_track_noise_select(NoiseSel P, int r, const ctag_track_noise_score* __restrict__ sc, double* __restrict__ cand,
                                                           NoiseSearch* __restrict__ st, ctag_track_noise_rec* __restrict__ out,
                                                           ctag_track_noise_round* __restrict__ trace) {
    __shared__ double sL[kNoiseMaxCand], sM2[kNoiseMaxCand], s_uc[3];
    __shared__ int sNt[kNoiseMaxCand], sNs[kNoiseMaxCand], sBad[kNoiseMaxCand], s_next;
    const int q = blockIdx.x, lane = threadIdx.x;
    NoiseSearch* me = st + q;
    double* __restrict__ mycand = cand + (size_t)q * P.n_cand * 3;
    if (r < 0) {
        const double uc0[3] = {0.0, 0.0, 0.0};
        if (lane == 0) {
            me->uc[0] = me->uc[1] = me->uc[2] = 0.0;
            me->score_start = 0.0;
            me->done = 0;
            me->pad = 0;
        }
        noise_write_candidates(P, uc0, P.span / 2.0, mycand, lane);
        return;
    }
    ctag_track_noise_round row;
    row.u[0] = row.u[1] = row.u[2] = 0.0;
    row.value[0] = row.value[1] = row.value[2] = 0.0;
    row.L = 0.0;
    row.winner = -1;
    row.reserved = 0;
    if (me->done) {  // wave-uniform
        if (lane == 0 && trace) trace[(size_t)q * P.rounds + r] = row;
        return;
    }
    // ---- the sums of every candidate: the rig's own, or over the rigs that are not bad input in rig order ----
    for (int c = lane; c < P.n_cand; c += 64) {
        double L = 0.0, m2 = 0.0;
        int nt = 0, ns = 0, n_good = 0;
        const int g0 = P.mode == CTAG_NOISE_POOLED ? 0 : q, g1 = P.mode == CTAG_NOISE_POOLED ? P.n_rigs : q + 1;
        for (int g = g0; g < g1; g++) {
            const ctag_track_noise_score e = sc[(size_t)c * P.n_rigs + g];
            if (e.status != CTAG_NOISE_OK) continue;
            L = n_good ? L + e.L : e.L;
            m2 = n_good ? m2 + e.sum_m2 : e.sum_m2;
            nt += e.n_terms;
            ns += e.n_singular;
            n_good++;
        }
        sL[c] = L, sM2[c] = m2, sNt[c] = nt, sNs[c] = ns, sBad[c] = n_good == 0;
    }
    __syncthreads();
    // ---- the decision has one owner ----
    if (lane == 0) {
        const double h = P.span / (double)(1 << (r + 1));
        ctag_track_noise_rec R;
        R.status = CTAG_NOISE_OK;
        R.rig = P.mode == CTAG_NOISE_POOLED ? -1 : q;
        R.n_terms = 0;
        R.n_free = P.n_free;
        R.rounds = r + 1;
        R.flags = 0u;
        R.q_rot = P.start[0], R.q_trans = P.start[1], R.cov_scale = P.start[2];
        R.log2_sigma[0] = R.log2_sigma[1] = R.log2_sigma[2] = 0.0;
        R.score = 0.0;
        R.score_start = me->score_start;
        R.mean_m2 = 0.0;
        bool finished = false;
        const int c0 = (P.n_cand - 1) / 2;
        if (sBad[c0]) {
            R.status = CTAG_NOISE_BAD_INPUT;
            R.rounds = 0;
            finished = true;
        } else if (r == 0) {
            me->score_start = R.score_start = sL[c0];
            if (sNt[c0] < P.min_terms) {
                R.status = CTAG_NOISE_TOO_FEW;
                R.n_terms = sNt[c0];
                R.score = sL[c0];
                R.mean_m2 = sNt[c0] > 0 ? sM2[c0] / (double)sNt[c0] : 0.0;
                finished = true;
            }
        }
        if (!finished) {
            int win = -1;
            for (int c = 0; c < P.n_cand; c++)
                if (sNs[c] == 0 && (win < 0 || sL[c] < sL[win])) win = c;
            if (win < 0) {
                R.status = CTAG_NOISE_SINGULAR;
                R.q_rot = P.start[0] * ctm::exp64(me->uc[0] * kLn2);
                R.q_trans = P.start[1] * ctm::exp64(me->uc[1] * kLn2);
                R.cov_scale = P.start[2] * ctm::exp64(me->uc[2] * kLn2);
                finished = true;
            } else {
                int j = 0;
                for (int a = 0; a < 3; a++) {
                    double u = me->uc[a];
                    if ((P.free_mask >> a) & 1) {
                        u = me->uc[a] + (double)((win / pow5(j)) % 5 - 2) * h;
                        j++;
                    }
                    row.u[a] = u;
                    row.value[a] = mycand[win * 3 + a];
                }
                row.L = sL[win];
                row.winner = win;
                if (r == P.rounds - 1) {
                    R.q_rot = row.value[0], R.q_trans = row.value[1], R.cov_scale = row.value[2];
                    R.n_terms = sNt[win];
                    R.score = sL[win];
                    R.mean_m2 = sM2[win] / (double)sNt[win];
                    j = 0;
                    for (int a = 0; a < 3; a++) {
                        if (!((P.free_mask >> a) & 1)) continue;
                        const int stride = pow5(j), k = (win / stride) % 5;
                        j++;
                        if (k == 0 || k == 4) {
                            R.flags |= CTAG_NOISE_FLAG_EDGE << a;
                            continue;
                        }
                        const int lo = win - stride, hi = win + stride;
                        if (sNs[lo] != 0 || sNs[hi] != 0) continue;
                        const double cv = ((sL[hi] - 2.0 * sL[win]) + sL[lo]) / (h * h);
                        if (cv > 0.0) R.log2_sigma[a] = ctm::sqrt64(2.0 / cv);
                    }
                    finished = true;
                } else {
                    me->uc[0] = row.u[0], me->uc[1] = row.u[1], me->uc[2] = row.u[2];
                }
            }
        }
        if (finished) {
            out[q] = R;
            me->done = 1;
        }
        if (trace) trace[(size_t)q * P.rounds + r] = row;
        s_next = !finished;
        s_uc[0] = row.u[0], s_uc[1] = row.u[1], s_uc[2] = row.u[2];
    }
    __syncthreads();
    if (s_next) {
        const double uc[3] = {s_uc[0], s_uc[1], s_uc[2]};
        noise_write_candidates(P, uc, P.span / (double)(1 << (r + 2)), mycand, lane);
    }
}

}  // namespace ctag

// =====================================================================================================
// host side
// =====================================================================================================
namespace {

struct NoiseState {
    ctag::DevBuf<double> d_times, d_cand;
    ctag::DevBuf<ctag_track_noise_score> d_scores;
    ctag::DevBuf<ctag::NoiseSearch> d_search;
    ctag::DevBuf<unsigned char> d_in;  // the host forms' records and results
    ctag::DevBuf<ctag_pose_cov_rec> d_cov;
    ctag::DevBuf<ctag_track_noise_rec> d_out;
    ctag::DevBuf<ctag_track_noise_round> d_trace;
    ctag::DevBuf<ctag_track_noise_score> d_score_out;
    std::vector<double> times, cand;  // of the call in flight: the caller's arrays may go once the call returns
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t done = nullptr;        // behind the last noise call's kernels: the workspace, `times` and `cand` are free again
    bool in_flight = false, timed = false;
    float ms = 0.f;
};

void noise_state_free(void* p) {
    NoiseState* s = static_cast<NoiseState*>(p);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->done) (void)hipEventDestroy(s->done);
    delete s;
}

NoiseState* noise_state(ctag_handle* h) {
    void** slot = ctag::handle_state_slot(h, ctag::kTrackNoiseState, noise_state_free);
    if (!*slot) {
        NoiseState* s = new (std::nothrow) NoiseState();
        if (!s) return nullptr;
        if (hipEventCreate(&s->ev[0]) != hipSuccess || hipEventCreate(&s->ev[1]) != hipSuccess ||
            hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess) {
            noise_state_free(s);
            return nullptr;
        }
        *slot = s;
    }
    return static_cast<NoiseState*>(*slot);
}

bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }

int noise_opts(const ctag_track_noise_opts* o, ctag::NoiseSel& sel, ctag::TfP& p, double& dt) {
    ctag_track_noise_opts d;
    ctag_track_noise_opts_default(&d);
    if (!o) o = &d;
    if (o->struct_size != sizeof(ctag_track_noise_opts)) return CTAG_ERR_ARG;
    if (o->mode != CTAG_NOISE_PER_RIG && o->mode != CTAG_NOISE_POOLED) return CTAG_ERR_ARG;
    if (o->free_mask < 0 || o->free_mask > 7 || o->rounds < 1 || o->rounds > 16 || o->max_gap < 1 || o->min_terms < 1) return CTAG_ERR_ARG;
    for (double v : {o->dt, o->q_rot, o->q_trans, o->cov_scale, o->vel0_sigma_rot, o->vel0_sigma_trans, o->span})
        if (!pos_finite(v)) return CTAG_ERR_ARG;
    sel.mode = o->mode;
    sel.free_mask = o->free_mask;
    sel.n_free = (o->free_mask & 1) + ((o->free_mask >> 1) & 1) + ((o->free_mask >> 2) & 1);
    sel.n_cand = 1;
    for (int k = 0; k < sel.n_free; k++) sel.n_cand *= 5;
    sel.rounds = o->rounds;
    sel.min_terms = o->min_terms;
    sel.start[0] = o->q_rot, sel.start[1] = o->q_trans, sel.start[2] = o->cov_scale;
    sel.span = o->span;
    p.loss = CTAG_TRACK_LOSS_NONE;
    p.max_gap = o->max_gap;
    p.q_rot = o->q_rot;
    p.q_trans = o->q_trans;
    p.vr2 = o->vel0_sigma_rot * o->vel0_sigma_rot;
    p.vt2 = o->vel0_sigma_trans * o->vel0_sigma_trans;
    p.a = 1.0;
    p.a2 = 1.0;
    p.gate2 = 0.0;
    p.cov_scale = o->cov_scale;
    dt = o->dt;
    return CTAG_OK;
}

// the checks and the staging every noise call shares; on CTAG_OK the times are on their way to st->d_times and ev[0] is recorded
int noise_begin(ctag_handle* h, const ctag_rigs* rigs, int n_frames, const double* times, double dt, NoiseState*& st, hipStream_t& s) {
    const int n_rigs = rigs->n_rigs;
    if (n_frames < 1 || n_rigs < 1 || (long long)n_frames * n_rigs > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    if (times) {
        for (int f = 0; f < n_frames; f++)
            if (!std::isfinite(times[f]) || (f > 0 && !(times[f] > times[f - 1]))) return CTAG_ERR_ARG;
    }
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    st = noise_state(h);
    if (!st) return CTAG_ERR_HIP;
    s = static_cast<hipStream_t>(ctag_stream(h));
    // an earlier noise call's kernels may still read the workspace, the times and the candidates: that call is waited for, nothing else on the stream is
    if (st->in_flight && hipEventSynchronize(st->done) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = false;
    if (st->d_times.grow((size_t)n_frames) != hipSuccess) return CTAG_ERR_HIP;
    st->times.resize(n_frames);
    for (int f = 0; f < n_frames; f++) st->times[f] = times ? times[f] : (double)f * dt;
    if (hipMemcpyAsync(st->d_times.p, st->times.data(), sizeof(double) * (size_t)n_frames, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    st->timed = ctag::handle_timing(h);
    if (st->timed && hipEventRecord(st->ev[0], s) != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

int noise_end(NoiseState* st, hipStream_t s) {
    if (hipGetLastError() != hipSuccess) return CTAG_ERR_HIP;
    if (st->timed && hipEventRecord(st->ev[1], s) != hipSuccess) return CTAG_ERR_HIP;
    if (hipEventRecord(st->done, s) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = true;
    return CTAG_OK;
}

unsigned noise_blocks(long long items) { return (unsigned)std::min<long long>(items, ctag::kNoiseMaxBlocks); }

template <class Rec>
int noise_fit_device(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs_dev, const ctag_pose_cov_rec* cov_dev, int n_frames, const double* times,
                     const ctag_track_noise_opts* opts, ctag_track_noise_rec* out_dev, ctag_track_noise_round* trace_dev) {
    if (!h || !rigs || !recs_dev || !cov_dev || !out_dev) return CTAG_ERR_ARG;
    ctag::NoiseSel sel;
    ctag::TfP P;
    double dt = 0.0;
    if (noise_opts(opts, sel, P, dt) != CTAG_OK) return CTAG_ERR_ARG;
    NoiseState* st = nullptr;
    hipStream_t s = nullptr;
    const int rc = noise_begin(h, rigs, n_frames, times, dt, st, s);
    if (rc != CTAG_OK) return rc;
    const int n_rigs = rigs->n_rigs, n_search = sel.mode == CTAG_NOISE_POOLED ? 1 : n_rigs;
    sel.n_rigs = n_rigs;
    const size_t n_items = (size_t)sel.n_cand * n_rigs;
    if (st->d_cand.grow((size_t)n_search * sel.n_cand * 3) != hipSuccess || st->d_scores.grow(n_items) != hipSuccess ||
        st->d_search.grow((size_t)n_search) != hipSuccess)
        return CTAG_ERR_HIP;
    const int stride = sel.mode == CTAG_NOISE_POOLED ? 0 : sel.n_cand;
    hipLaunchKernelGGL(ctag::k_track_noise_select, dim3(n_search), dim3(64), 0, s, sel, -1, st->d_scores.p, st->d_cand.p, st->d_search.p, out_dev, trace_dev);
    for (int r = 0; r < sel.rounds; r++) {
        hipLaunchKernelGGL(ctag::k_track_noise<Rec>, dim3(noise_blocks((long long)n_items)), dim3(64), 0, s, recs_dev, cov_dev, n_frames, n_rigs,
                           st->d_times.p, P, st->d_cand.p, sel.n_cand, stride, st->d_scores.p);
        hipLaunchKernelGGL(ctag::k_track_noise_select, dim3(n_search), dim3(64), 0, s, sel, r, st->d_scores.p, st->d_cand.p, st->d_search.p, out_dev, trace_dev);
    }
    return noise_end(st, s);
}

template <class Rec>
int noise_score_device(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs_dev, const ctag_pose_cov_rec* cov_dev, int n_frames, const double* times,
                       const ctag_track_noise_opts* opts, const double* cand, int n_cand, ctag_track_noise_score* out_dev) {
    if (!h || !rigs || !recs_dev || !cov_dev || !cand || !out_dev) return CTAG_ERR_ARG;
    ctag::NoiseSel sel;
    ctag::TfP P;
    double dt = 0.0;
    if (noise_opts(opts, sel, P, dt) != CTAG_OK) return CTAG_ERR_ARG;
    if (n_cand < 1 || n_cand > CTAG_NOISE_MAX_SCORE_CAND) return CTAG_ERR_ARG;
    for (int k = 0; k < 3 * n_cand; k++)
        if (!pos_finite(cand[k])) return CTAG_ERR_ARG;
    NoiseState* st = nullptr;
    hipStream_t s = nullptr;
    const int rc = noise_begin(h, rigs, n_frames, times, dt, st, s);
    if (rc != CTAG_OK) return rc;
    if (st->d_cand.grow((size_t)n_cand * 3) != hipSuccess) return CTAG_ERR_HIP;
    st->cand.assign(cand, cand + 3 * (size_t)n_cand);
    if (hipMemcpyAsync(st->d_cand.p, st->cand.data(), sizeof(double) * 3 * (size_t)n_cand, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    const long long n_items = (long long)n_cand * rigs->n_rigs;
    hipLaunchKernelGGL(ctag::k_track_noise<Rec>, dim3(noise_blocks(n_items)), dim3(64), 0, s, recs_dev, cov_dev, n_frames, rigs->n_rigs, st->d_times.p, P,
                       st->d_cand.p, n_cand, 0, out_dev);
    return noise_end(st, s);
}

// the host forms' records onto the device (every earlier host form has waited for its own work: the buffers are free)
template <class Rec>
int noise_stage(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, NoiseState*& st, hipStream_t& s) {
    if (n_frames < 1 || rigs->n_rigs < 1 || (long long)n_frames * rigs->n_rigs > CTAG_TRACK_MAX_ITEMS) return CTAG_ERR_ARG;
    if (hipSetDevice(ctag::handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    st = noise_state(h);
    if (!st) return CTAG_ERR_HIP;
    s = static_cast<hipStream_t>(ctag_stream(h));
    if (st->in_flight && hipEventSynchronize(st->done) != hipSuccess) return CTAG_ERR_HIP;
    st->in_flight = false;
    const size_t n = (size_t)n_frames * rigs->n_rigs;
    if (st->d_in.grow(sizeof(Rec) * n) != hipSuccess || st->d_cov.grow(n) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpyAsync(st->d_in.p, recs, sizeof(Rec) * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(st->d_cov.p, cov, sizeof(ctag_pose_cov_rec) * n, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    return CTAG_OK;
}

template <class Rec>
int noise_fit_host(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                   const ctag_track_noise_opts* opts, ctag_track_noise_rec* out, ctag_track_noise_round* trace) {
    if (!h || !rigs || !recs || !cov || !out) return CTAG_ERR_ARG;
    ctag::NoiseSel sel;
    ctag::TfP P;
    double dt = 0.0;
    if (noise_opts(opts, sel, P, dt) != CTAG_OK) return CTAG_ERR_ARG;
    NoiseState* st = nullptr;
    hipStream_t s = nullptr;
    int rc = noise_stage(h, rigs, recs, cov, n_frames, st, s);
    if (rc != CTAG_OK) return rc;
    const size_t n_search = sel.mode == CTAG_NOISE_POOLED ? 1 : (size_t)rigs->n_rigs, n_rows = n_search * sel.rounds;
    if (st->d_out.grow(n_search) != hipSuccess || (trace && st->d_trace.grow(n_rows) != hipSuccess)) return CTAG_ERR_HIP;
    rc = noise_fit_device<Rec>(h, rigs, reinterpret_cast<const Rec*>(st->d_in.p), st->d_cov.p, n_frames, times, opts, st->d_out.p, trace ? st->d_trace.p : nullptr);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_out.p, sizeof(ctag_track_noise_rec) * n_search, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (trace && hipMemcpyAsync(trace, st->d_trace.p, sizeof(ctag_track_noise_round) * n_rows, hipMemcpyDeviceToHost, s) != hipSuccess))
        return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

template <class Rec>
int noise_score_host(ctag_handle* h, const ctag_rigs* rigs, const Rec* recs, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                     const ctag_track_noise_opts* opts, const double* cand, int n_cand, ctag_track_noise_score* out) {
    if (!h || !rigs || !recs || !cov || !cand || !out) return CTAG_ERR_ARG;
    if (n_cand < 1 || n_cand > CTAG_NOISE_MAX_SCORE_CAND) return CTAG_ERR_ARG;
    ctag::NoiseSel sel;
    ctag::TfP P;
    double dt = 0.0;
    if (noise_opts(opts, sel, P, dt) != CTAG_OK) return CTAG_ERR_ARG;
    NoiseState* st = nullptr;
    hipStream_t s = nullptr;
    int rc = noise_stage(h, rigs, recs, cov, n_frames, st, s);
    if (rc != CTAG_OK) return rc;
    const size_t n = (size_t)n_cand * rigs->n_rigs;
    if (st->d_score_out.grow(n) != hipSuccess) return CTAG_ERR_HIP;
    rc = noise_score_device<Rec>(h, rigs, reinterpret_cast<const Rec*>(st->d_in.p), st->d_cov.p, n_frames, times, opts, cand, n_cand, st->d_score_out.p);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpyAsync(out, st->d_score_out.p, sizeof(ctag_track_noise_score) * n, hipMemcpyDeviceToHost, s) != hipSuccess) return CTAG_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace

extern "C" {

void ctag_track_noise_opts_default(ctag_track_noise_opts* o) {
    if (!o) return;
    ctag_track_filter_opts f;
    ctag_track_filter_opts_default(&f);
    o->struct_size = (uint32_t)sizeof(ctag_track_noise_opts);
    o->mode = CTAG_NOISE_PER_RIG;
    o->free_mask = CTAG_NOISE_FREE_Q_ROT | CTAG_NOISE_FREE_Q_TRANS | CTAG_NOISE_FREE_COV_SCALE;
    o->rounds = 10;
    o->max_gap = f.max_gap;
    o->min_terms = 8;
    o->dt = f.dt;
    o->q_rot = f.q_rot;
    o->q_trans = f.q_trans;
    o->cov_scale = 1.0;
    o->vel0_sigma_rot = f.vel0_sigma_rot;
    o->vel0_sigma_trans = f.vel0_sigma_trans;
    o->span = 16.0;
}

int ctag_rig_track_noise_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                    int n_frames, const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out_dev,
                                    ctag_track_noise_round* trace_dev) {
    return noise_fit_device<ctag_rig_pose_rec>(h, rigs, rig_poses_dev, cov_dev, n_frames, times, opts, out_dev, trace_dev);
}

int ctag_mv_rig_track_noise_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                       int n_frames, const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out_dev,
                                       ctag_track_noise_round* trace_dev) {
    return noise_fit_device<ctag_mv_pose_rec>(h, rigs, mv_poses_dev, cov_dev, n_frames, times, opts, out_dev, trace_dev);
}

int ctag_rig_track_noise_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                             const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out, ctag_track_noise_round* trace) {
    return noise_fit_host<ctag_rig_pose_rec>(h, rigs, rig_poses, cov, n_frames, times, opts, out, trace);
}

int ctag_mv_rig_track_noise_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                                const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out, ctag_track_noise_round* trace) {
    return noise_fit_host<ctag_mv_pose_rec>(h, rigs, mv_poses, cov, n_frames, times, opts, out, trace);
}

int ctag_rig_track_noise_score_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                      int n_frames, const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand,
                                      ctag_track_noise_score* out_dev) {
    return noise_score_device<ctag_rig_pose_rec>(h, rigs, rig_poses_dev, cov_dev, n_frames, times, opts, cand, n_cand, out_dev);
}

int ctag_mv_rig_track_noise_score_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                         int n_frames, const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand,
                                         ctag_track_noise_score* out_dev) {
    return noise_score_device<ctag_mv_pose_rec>(h, rigs, mv_poses_dev, cov_dev, n_frames, times, opts, cand, n_cand, out_dev);
}

int ctag_rig_track_noise_score(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                               const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand, ctag_track_noise_score* out) {
    return noise_score_host<ctag_rig_pose_rec>(h, rigs, rig_poses, cov, n_frames, times, opts, cand, n_cand, out);
}

int ctag_mv_rig_track_noise_score(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                                  const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand, ctag_track_noise_score* out) {
    return noise_score_host<ctag_mv_pose_rec>(h, rigs, mv_poses, cov, n_frames, times, opts, cand, n_cand, out);
}

int ctag_track_noise_last_ms(ctag_handle* h, float* out1) {
    if (!h || !out1) return CTAG_ERR_ARG;
    NoiseState* st = noise_state(h);
    if (!st) return CTAG_ERR_HIP;
    if (st->timed) {
        st->timed = false;
        st->ms = 0.f;
        if (hipEventSynchronize(st->ev[1]) == hipSuccess) (void)hipEventElapsedTime(&st->ms, st->ev[0], st->ev[1]);
    }
    *out1 = st->ms;
    return CTAG_OK;
}

}  // extern "C"
