// ctag_fit_host.h -- the host side that the four fits share (k_model_fit.hip: the corners of a model against marker poses;
// k_rig_fit.hip: the member transforms of a rig against rig poses; k_cam_fit.hip: the camera poses of a set against multi-view rig
// poses, one group; k_intr_fit.hip: the intrinsics of a camera against its own view poses, one group of 16 rows; nothing else
// includes it).  All minimise a reprojection cost over per-group unknowns (group = model / rig /
// the camera set) by Levenberg-Marquardt rounds on a Schur-reduced system: a pose pass, a record
// kernel and an assemble kernel over the observation records, a damped solve per group, and a decision per group.  Stated here
// once: the timed state on the handle, the context of a call, the working model, the systems on the device with their pass loop
// and solve, and the LM bookkeeping with its constants, its options check and its decision; for the two fits whose unknowns are
// 6-parameter slots (rig, camera set) also the slot systems with their workspace, assemble and solve launches and the probe's
// hand-out, and the co-visibility tree of their initial assembly.  Each fit keeps its kernels and its own round loop: the
// four loops have the same shape (rebuild the systems if a trial was accepted, solve, make the trials, one pose pass, decide per
// group) and differ in what a trial and an accepted state are; stated once with five callbacks the loop came out longer than the
// plain loops together (tried with the first two) and harder to follow, so the shape is repeated and everything the loops call is shared.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/ctag_pose.h"
#include "ctag_fit_solve.h"
#include "ctag_internal.h"
#include "ctag_lm.h"
#include "ctag_pose_dev.h"
#include "ctag_schur6.h"

#define FIT_HIP(call)                                  \
    do {                                               \
        if ((call) != hipSuccess) return CTAG_ERR_HIP; \
    } while (0)

namespace ctag {
namespace fit {

// ---- the state a fit keeps on the handle (its SiblingState slot): three events and the four slots of its *_last_ms
struct Timed {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
};

inline void timed_free(void* p) {
    Timed* s = static_cast<Timed*>(p);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

inline Timed* timed_state(ctag_handle* h, SiblingState which) {
    void** slot = handle_state_slot(h, which, timed_free);
    if (!*slot) {
        Timed* s = new (std::nothrow) Timed();
        if (!s) return nullptr;
        for (auto& e : s->ev)
            if (hipEventCreate(&e) != hipSuccess) {
                timed_free(s);
                return nullptr;
            }
        *slot = s;
    }
    return static_cast<Timed*>(*slot);
}

inline int last_ms(ctag_handle* h, SiblingState which, float* out4) {
    if (!h || !out4) return CTAG_ERR_ARG;
    Timed* st = timed_state(h, which);
    if (!st) return CTAG_ERR_HIP;
    for (int i = 0; i < 4; i++) out4[i] = st->ms[i];
    return CTAG_OK;
}

inline int launched() { return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP; }

// ---- the context of one call
struct Call {
    ctag_handle* h = nullptr;
    hipStream_t s = nullptr;
    Timed* st = nullptr;
    bool timing = false;
    const ctag_frame_result* res = nullptr;  // device
    int n_frames = 0;
    PoseCam cam{};

    int prepare(ctag_handle* h_, SiblingState which, const ctag_frame_result* results_dev, int n_frames_, const ctag_camera* camera) {
        h = h_;
        FIT_HIP(hipSetDevice(handle_device(h)));
        st = timed_state(h, which);
        if (!st) return CTAG_ERR_HIP;
        s = static_cast<hipStream_t>(ctag_stream(h));
        timing = handle_timing(h);
        for (float& v : st->ms) v = 0.f;
        res = results_dev;
        n_frames = n_frames_;
        cam = make_pose_cam(camera);
        return CTAG_OK;
    }

    // Timing, all of it nothing unless the handle has timing on: mark(i) records event i on the stream; reached(i) waits for it;
    // add_ms(k, i) adds the milliseconds between events i and i + 1, both reached, to slot k.
    int mark(int i) { return !timing || hipEventRecord(st->ev[i], s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP; }
    int reached(int i) { return !timing || hipEventSynchronize(st->ev[i]) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP; }
    void add_ms(int k, int i) {
        float ms = 0.f;
        if (timing && hipEventElapsedTime(&ms, st->ev[i], st->ev[i + 1]) == hipSuccess) st->ms[k] += ms;
    }

    // n records from the device to `host`.  Waits.
    template <class Rec>
    int fetch(const Rec* recs_dev, size_t n, std::vector<Rec>& host) {
        host.resize(n);
        FIT_HIP(hipMemcpyAsync(host.data(), recs_dev, sizeof(Rec) * n, hipMemcpyDeviceToHost, s));
        FIT_HIP(hipStreamSynchronize(s));
        return CTAG_OK;
    }

    // a pose pass: pose() (timed in slot k) writes n records to recs_dev, which then come to the host.  Waits.
    template <class Rec, class F>
    int pose_pass(int k, F&& pose, const Rec* recs_dev, size_t n, std::vector<Rec>& host) {
        if (mark(0) != CTAG_OK) return CTAG_ERR_HIP;
        const int rc = pose();
        if (rc != CTAG_OK) return rc;
        if (mark(1) != CTAG_OK || fetch(recs_dev, n, host) != CTAG_OK) return CTAG_ERR_HIP;
        add_ms(k, 0);
        return CTAG_OK;
    }
};

// the host entry of a fit: the detection records to the device, then the device entry on them
template <class DeviceEntry>
int with_results_on_device(ctag_handle* h, const ctag_frame_result* results, int n_frames, DeviceEntry&& entry) {
    if (hipSetDevice(handle_device(h)) != hipSuccess) return CTAG_ERR_HIP;
    DevBuf<ctag_frame_result> d_res;
    FIT_HIP(d_res.grow((size_t)n_frames));
    FIT_HIP(hipMemcpy(d_res.p, results, sizeof(ctag_frame_result) * (size_t)n_frames, hipMemcpyHostToDevice));
    return entry(d_res.p);
}

// what a probe is given on the host, on the device: c.res and d_recs
template <class Rec>
int upload_probe_inputs(Call& c, const ctag_frame_result* results, DevBuf<ctag_frame_result>& d_res, const Rec* recs, size_t n_recs, DevBuf<Rec>& d_recs) {
    FIT_HIP(d_res.grow(c.n_frames));
    FIT_HIP(d_recs.grow(n_recs));
    FIT_HIP(hipMemcpyAsync(d_res.p, results, sizeof(ctag_frame_result) * (size_t)c.n_frames, hipMemcpyHostToDevice, c.s));
    FIT_HIP(hipMemcpyAsync(d_recs.p, recs, sizeof(Rec) * n_recs, hipMemcpyHostToDevice, c.s));
    c.res = d_res.p;
    return CTAG_OK;
}

// The per-marker pose records of every frame under `model`: a first call with capacity 1 is made for the offsets (off, on the
// host too: off[n_frames] is the record count) and for the model's device copy, the one pose it solves is discarded; d_poses
// then has room for all of them.
inline int count_pose_records(Call& c, const ctag_model* model, const ctag_camera* camera, DevBuf<int32_t>& d_off, DevBuf<ctag_pose_rec>& d_poses,
                              std::vector<int32_t>& off) {
    FIT_HIP(d_off.grow((size_t)c.n_frames + 1));
    FIT_HIP(d_poses.grow(1));
    const int rc = ctag_pose_batch_device(c.h, c.res, c.n_frames, model, camera, d_off.p, d_poses.p, 1);
    if (rc != CTAG_OK) return rc;
    if (c.fetch(d_off.p, (size_t)c.n_frames + 1, off) != CTAG_OK) return CTAG_ERR_HIP;
    if (off[c.n_frames] > 0) FIT_HIP(d_poses.grow((size_t)off[c.n_frames]));
    return CTAG_OK;
}

// ---- the working model of a call
struct ModelGuard {  // frees the working model unless it is handed out
    ctag_model* m = nullptr;
    ~ModelGuard() {
        if (m) ctag_model_free(m);
    }
};

inline int clone_model(const ctag_model* in, ctag_model** out) {
    ctag_model_view v;
    if (ctag_model_get_view(in, &v) != CTAG_OK) return CTAG_ERR_ARG;
    return ctag_model_create(&v, out);
}

// the working model's corners to its device copy, behind what is enqueued on the stream
inline int push_corners(Call& c, ctag_model* W) {
    return hipMemcpyAsync(W->d_corners.p, W->corners.data(), sizeof(float) * W->corners.size(), hipMemcpyHostToDevice, c.s) == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

// the device copies belong to the trial states of the call: the model handed out makes its own at its first use
inline void release_device_copies(ctag_model* W) {
    W->d_ids.release();
    W->d_corners.release();
    W->d_base_axis.release();
    W->d_base = W->d_axis = nullptr;
    W->device = -1;
}

inline double det3(const double* M) { return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]); }

// the rotation nearest to M (Frobenius): R = U diag(1, 1, sg) V^T of M = U sv V^T, sg = +-1 the sign of det(U V^T), which is returned
inline double nearest_rotation(const double* M, double* R, double* sv) {
    double U[9], V[9];
    ctl::svd3(M, U, sv, V);
    const double sg = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) R[a * 3 + b] = U[a * 3] * V[b * 3] + U[a * 3 + 1] * V[b * 3 + 1] + sg * U[a * 3 + 2] * V[b * 3 + 2];
    return sg;
}

inline void mat_mul(const double* A, const double* B, double* C) {  // C = A B, 3x3 row-major, sums in index order
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

inline void mat_vec(const double* A, const double* v, double* o) {
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}

// ---- the initial assembly's tree (rule 2 of the rig assembly and of the camera set fit) over k nodes with the symmetric co-visibility
// counts cnt[k x k]: the anchor is the first node with an edge of at least min_count, and the tree grows from it by the edge of the
// largest count (at least min_count) between a node in it and one outside.  edge(parent, child, count) is called for every edge in
// the order the tree grows, in_tree[k] marks its nodes.  Returns the anchor, -1 when no edge counts.
template <class Edge>
int covisibility_tree(int k, const std::vector<int>& cnt, int min_count, std::vector<uint8_t>& in_tree, Edge&& edge) {
    in_tree.assign(k, 0);
    int anchor = -1;
    for (int a = 0; a < k && anchor < 0; a++)
        for (int b = 0; b < k; b++)
            if (cnt[(size_t)a * k + b] >= min_count) {
                anchor = a;
                break;
            }
    if (anchor < 0) return -1;
    in_tree[anchor] = 1;
    for (;;) {
        int best = min_count - 1, ba = -1, bb = -1;
        for (int b = 0; b < k; b++) {  // ascending b, then ascending a: the first of equal counts stays
            if (in_tree[b]) continue;
            for (int a = 0; a < k; a++)
                if (in_tree[a] && cnt[(size_t)a * k + b] > best) {
                    best = cnt[(size_t)a * k + b];
                    ba = a;
                    bb = b;
                }
        }
        if (bb < 0) return anchor;
        edge(ba, bb, best);
        in_tree[bb] = 1;
    }
}

// ---- the observation records and the reduced systems of every group, on the device
struct Systems {
    int n_groups = 0, N = 0, R = 0, pass = 0;    // N: rows of a group's S, g and delta
    std::vector<int32_t> obs, rec_group, flags;  // [R]: the pose record observed, its group, the record kernel's verdict (kRec*)
    DevBuf<int32_t> d_obs, d_rec_group, d_flags, d_active, d_bad;
    DevBuf<double> d_S, d_g, d_delta, d_lambda;

    // after obs and rec_group are filled; one pass of the record workspace holds pass_records records (default_pass if not positive)
    int setup(Call& c, int n_groups_, int N_, int pass_records, int default_pass) {
        n_groups = n_groups_;
        N = N_;
        R = (int)obs.size();
        pass = std::max(1, std::min(R, pass_records > 0 ? pass_records : default_pass));
        FIT_HIP(d_obs.grow(std::max(R, 1)));
        FIT_HIP(d_rec_group.grow(std::max(R, 1)));
        FIT_HIP(d_flags.grow(std::max(R, 1)));
        FIT_HIP(d_S.grow((size_t)n_groups * N * N));
        FIT_HIP(d_g.grow((size_t)n_groups * N));
        FIT_HIP(d_delta.grow((size_t)n_groups * N));
        FIT_HIP(d_lambda.grow(n_groups));
        FIT_HIP(d_active.grow(n_groups));
        FIT_HIP(d_bad.grow(n_groups));
        if (R > 0) {
            FIT_HIP(hipMemcpyAsync(d_obs.p, obs.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, c.s));
            FIT_HIP(hipMemcpyAsync(d_rec_group.p, rec_group.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, c.s));
        }
        flags.assign(R, 0);
        return CTAG_OK;
    }

    // S and g of every group, pass by pass: launch(r0, r1) enqueues the record and the assemble kernel of records r0 .. r1-1.
    // The flags come back to the host.  Waits.
    template <class Launch>
    int build(Call& c, Launch&& launch) {
        FIT_HIP(hipMemsetAsync(d_S.p, 0, sizeof(double) * (size_t)n_groups * N * N, c.s));
        FIT_HIP(hipMemsetAsync(d_g.p, 0, sizeof(double) * (size_t)n_groups * N, c.s));
        for (int r0 = 0; r0 < R; r0 += pass) {
            const int rc = launch(r0, std::min(R, r0 + pass));
            if (rc != CTAG_OK) return rc;
        }
        if (R > 0) FIT_HIP(hipMemcpyAsync(flags.data(), d_flags.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, c.s));
        FIT_HIP(hipStreamSynchronize(c.s));
        return CTAG_OK;
    }

    // build() for a fit whose record and assemble kernel are timed together in slot 2: enqueue(r0, r1) launches the two
    template <class Enqueue>
    int build_timed(Call& c, Enqueue&& enqueue) {
        return build(c, [&](int r0, int r1) {
            if (c.mark(0) != CTAG_OK) return CTAG_ERR_HIP;
            enqueue(r0, r1);
            if (launched() != CTAG_OK || c.mark(1) != CTAG_OK || c.reached(1) != CTAG_OK) return CTAG_ERR_HIP;
            c.add_ms(2, 0);
            return CTAG_OK;
        });
    }

    // delta[n_groups][N] and bad[n_groups] of the groups with active[g] != 0: launch() enqueues the solve kernel (timed in slot 3).
    // A group is bad for a pivot of its system that is not positive, and when a record of it carries one of bad_flags.  Waits.
    template <class Launch>
    int solve(Call& c, const std::vector<double>& lambda, const std::vector<int32_t>& active, int bad_flags, std::vector<double>& delta,
              std::vector<int32_t>& bad, Launch&& launch) {
        FIT_HIP(hipMemcpyAsync(d_lambda.p, lambda.data(), sizeof(double) * n_groups, hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipMemcpyAsync(d_active.p, active.data(), sizeof(int32_t) * n_groups, hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int32_t) * n_groups, c.s));
        FIT_HIP(hipMemsetAsync(d_delta.p, 0, sizeof(double) * (size_t)n_groups * N, c.s));
        if (c.mark(0) != CTAG_OK) return CTAG_ERR_HIP;
        launch();
        if (launched() != CTAG_OK || c.mark(1) != CTAG_OK) return CTAG_ERR_HIP;
        delta.resize((size_t)n_groups * N);
        bad.resize(n_groups);
        FIT_HIP(hipMemcpyAsync(delta.data(), d_delta.p, sizeof(double) * delta.size(), hipMemcpyDeviceToHost, c.s));
        FIT_HIP(hipMemcpyAsync(bad.data(), d_bad.p, sizeof(int32_t) * n_groups, hipMemcpyDeviceToHost, c.s));
        FIT_HIP(hipStreamSynchronize(c.s));
        c.add_ms(3, 0);
        for (int r = 0; r < R; r++)
            if (flags[r] & bad_flags) bad[rec_group[r]] = 1;
        return CTAG_OK;
    }

    // cost of every group over its observation records among P, in record order (skip[r] != 0: not this one); all_ok[g] = 0 when
    // one of them is not CTAG_POSE_OK
    template <class Rec>
    void costs_of(const std::vector<Rec>& P, const std::vector<uint8_t>* skip, std::vector<double>& cost, std::vector<uint8_t>& all_ok) const {
        cost.assign(n_groups, 0.0);
        all_ok.assign(n_groups, 1);
        for (int r = 0; r < R; r++) {
            if (skip && (*skip)[r]) continue;
            const Rec& p = P[obs[r]];
            if (p.status != CTAG_POSE_OK) all_ok[rec_group[r]] = 0;
            cost[rec_group[r]] += p.cost;
        }
    }

    // group g accepts its trial: its observation records of `trial` replace those of `acc`
    template <class Rec>
    void take_records(int g, const std::vector<Rec>& trial, std::vector<Rec>& acc) const {
        for (int r = 0; r < R; r++)
            if (rec_group[r] == g) acc[obs[r]] = trial[obs[r]];
    }
};

// ---- the systems of a fit whose unknowns are 6-parameter slots (the rig assembly: a group per rig, a slot per placed model; the camera
// set fit: one group, a slot per placed camera): STRIDE = 6 x the most slots of a group is the row stride of S, g and delta, and a
// record's workspace holds STRIDE / 6 slot blocks (ctag_schur6.h) for k_fit_assemble<STRIDE> and k_fit_solve<STRIDE>
template <int STRIDE>
struct SlotSystems : Systems {
    Call c;
    std::vector<int32_t> n_slots, drop;  // [n_groups]: the slots of a group's system, and the one whose rows are dropped (the anchor's)
    DevBuf<int32_t> d_n_slots, d_drop;
    DevBuf<double> d_ws;

    // after obs, rec_group, n_slots and drop are filled
    int setup(int pass_records, int default_pass) {
        const int ng = (int)n_slots.size();
        if ((size_t)ng * STRIDE * STRIDE * 8 > ((size_t)2 << 30)) return CTAG_ERR_LIMIT;
        const int rc = Systems::setup(c, ng, STRIDE, pass_records, default_pass);
        if (rc != CTAG_OK) return rc;
        FIT_HIP(d_ws.grow((size_t)pass * (STRIDE / 6) * kSlotDoubles));
        FIT_HIP(d_n_slots.grow(ng));
        FIT_HIP(d_drop.grow(ng));
        FIT_HIP(hipMemcpyAsync(d_n_slots.p, n_slots.data(), sizeof(int32_t) * ng, hipMemcpyHostToDevice, c.s));
        FIT_HIP(hipMemcpyAsync(d_drop.p, drop.data(), sizeof(int32_t) * ng, hipMemcpyHostToDevice, c.s));
        return CTAG_OK;
    }

    // the launch of the assemble kernel behind the record kernel of records r0 .. r1-1
    template <class SlotOf>
    void assemble(SlotOf slot_of, int r0, int r1) {
        hipLaunchKernelGGL((k_fit_assemble<STRIDE, SlotOf>), dim3(fit_assemble_blocks<STRIDE>(), n_groups), dim3(kFitAssembleThreads), 0, c.s, d_ws.p, slot_of, d_flags.p,
                           r0, r1, d_S.p, d_g.p);
    }

    int solve(const std::vector<double>& lambda, const std::vector<int32_t>& active, int bad_flags, std::vector<double>& delta, std::vector<int32_t>& bad) {
        return Systems::solve(c, lambda, active, bad_flags, delta, bad, [&]() {
            hipLaunchKernelGGL(k_fit_solve<STRIDE>, dim3(n_groups), dim3(kFitSolveThreads), 0, c.s, d_S.p, d_g.p, d_n_slots.p, d_drop.p, d_lambda.p, d_active.p, d_delta.p,
                               d_bad.p);
        });
    }

    // what a probe hands out: group grp's system at `lambda` solved alone (a caller's record may be left out; that does not make the
    // group bad here), its S, g and delta compacted from row stride STRIDE to N = 6 n_slots[grp]
    int probe(int grp, double lambda, double* S, double* g, double* delta, int32_t* n_unknowns, int32_t* bad_pivot) {
        std::vector<double> lam(n_groups, lambda), d;
        std::vector<int32_t> active(n_groups, 0), bad;
        active[grp] = 1;
        const int rc = solve(lam, active, kRecSingular, d, bad);
        if (rc != CTAG_OK) return rc;
        const int N = 6 * n_slots[grp];
        std::vector<double> Sf((size_t)STRIDE * STRIDE), gf(STRIDE);
        FIT_HIP(hipMemcpy(Sf.data(), d_S.p + (size_t)grp * STRIDE * STRIDE, sizeof(double) * Sf.size(), hipMemcpyDeviceToHost));
        FIT_HIP(hipMemcpy(gf.data(), d_g.p + (size_t)grp * STRIDE, sizeof(double) * STRIDE, hipMemcpyDeviceToHost));
        for (int i = 0; i < N; i++) {
            for (int j = 0; j < N; j++) S[(size_t)i * N + j] = Sf[(size_t)i * STRIDE + j];
            g[i] = gf[i];
            delta[i] = d[(size_t)grp * STRIDE + i];
        }
        *n_unknowns = N;
        *bad_pivot = bad[grp];
        return CTAG_OK;
    }
};

// the options every fit's Levenberg-Marquardt takes: lambda0, lambda_max and rel_tol are positive and finite
template <class Opts>
bool lm_opts_ok(const Opts& o) {
    for (double v : {o.lambda0, o.lambda_max, o.rel_tol})
        if (!std::isfinite(v) || !(v > 0.0)) return false;
    return true;
}

// ---- Levenberg-Marquardt per group
struct Lm {
    std::vector<double> lambda, cost;  // the damping and the cost of the accepted state
    std::vector<int32_t> active, rounds;

    void start(int n_groups, double lambda0) {
        lambda.assign(n_groups, lambda0);
        cost.assign(n_groups, 0.0);
        active.assign(n_groups, 0);
        rounds.assign(n_groups, 0);
    }

    bool any_active() const {
        return std::any_of(active.begin(), active.end(), [](int32_t a) { return a != 0; });
    }

    // One round of group g is over.  A usable trial that lowers the cost is accepted: lambda / 3 (not below 1e-9), and the group
    // stops when the drop is below rel_tol of the new cost.  Otherwise lambda x 4, and the group stops above lambda_max.  It
    // stops after max_rounds rounds either way.  Returns whether the trial is accepted.
    template <class Opts>
    bool decide(int g, bool trial_usable, double cost_trial, const Opts& o) {
        LmState s{lambda[g], cost[g], active[g], rounds[g]};
        const bool accept = lm_decide(s, trial_usable, cost_trial, o.rel_tol, o.lambda_max, o.max_rounds);
        lambda[g] = s.lambda;
        cost[g] = s.cost;
        active[g] = s.active;
        rounds[g] = s.rounds;
        return accept;
    }
};

}  // namespace fit
}  // namespace ctag
