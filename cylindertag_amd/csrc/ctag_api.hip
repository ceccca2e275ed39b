// ctag_api.hip -- implementation of the C ABI in include/ctag.h: handle, workspace, batching, probes.
// Host orchestration only; the arithmetic lives in k_sweep.hip / k_quad.hip / k_feature.hip.
// There is deliberately no CPU fallback: if HIP is unavailable every entry point returns CTAG_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ctag.h"
#include "ctag_internal.h"

using namespace ctag;

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            std::snprintf(h->last_error, sizeof(h->last_error), "%s: %s", #expr, hipGetErrorString(e__)); \
            return CTAG_ERR_HIP;                                                                        \
        }                                                                                               \
    } while (0)

// One call -- or the frames [f0, f0 + m) of one (sub) -- as the host layer hands it down: where the frames lie and how they are to be detected
struct Call {
    const uint8_t* frames;
    int n, rows, cols, channels;  // channels 3: 8-bit BGR, 3 bytes per pixel
    ptrdiff_t row_stride, frame_stride;
    int adaptive_thresh, corner_subpix, subpix_dist;
    Call sub(int f0, int m) const {
        Call c = *this;
        c.frames += (ptrdiff_t)f0 * frame_stride;
        c.n = m;
        return c;
    }
};

// One result record in pinned host memory, written by k_markers itself through its device address: no download behind the chain
struct MappedRec {
    ctag_frame_result* host = nullptr;
    ctag_frame_result* dev = nullptr;
    hipError_t ensure() {
        if (host) return hipSuccess;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(ctag_frame_result), hipHostMallocMapped);
        return e != hipSuccess ? e : hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0);
    }
    ~MappedRec() {
        if (host) (void)hipHostFree(host);
    }
};

struct ctag_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;          // side branch of the chain in few-frame calls (launch_quads), joined by events
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<int32_t> dict;
    ctag_params params{};            // the tunables this handle was created with (ctag_params_default unless ctag_create_ex said otherwise)
    KParams kp{};                    // ... as the kernels consume them
    DevBuf<uint8_t> d_thr_table;     // adaptive-threshold bound table for params.dark_cap
    DevBuf<int32_t> d_dict;
    DevBuf<uint32_t> d_dict_pos;     // [dict_rows][64]: columns holding each symbol (k_markers' bit-parallel coverage); null for > 32 columns
    DevBuf<uint8_t> d_pick_table;
    int dict_rows = 0, dict_cols = 0, feature_size = 0;
    // Two kinds of workspace: a batch one holds chunks of frames with pools sized for what a frame of its size ordinarily needs (make_caps);
    // the big one holds ONE frame with pools no frame of that size can exhaust -- a frame that overflowed a batch pool (thousands of
    // blobs, fine texture: CTAG_FLAG_POOL_OVERFLOW -> CTAG_PENDING) is run again there (rerun_frame).  Each is allocated on first use.
    struct WsSlot {
        Workspace ws;
        DevBuf<char> mem;           // ws.base
        int rows = 0, cols = 0, tw = 0, cap = 0;
        DevBuf<double> n0;          // refine_n0, allocated when a chunk of more than kLatencyFrames frames first runs with corner_subpix
    };
    // CTAG_OPT_STREAMS = 2 (default): a chunk of a device-memory batch runs as two halves on two streams (`stream` + `streamx[0]`, workspaces
    // `slot[0]` + `slot[1]`), so that the tail of one half's kernels -- a few long boundary / Welsch blocks -- overlaps the other half's next
    // kernel.  The extra streams fork from `stream` at the head of a call and join it at the end: callers still order against `stream` alone.
    static constexpr int kMaxStreams = 4;
    static constexpr int kBigSlot = kMaxStreams;
    WsSlot slot[kMaxStreams + 1];                   // stream k (0: `stream`, k > 0: streamx[k - 1]) uses slot[k] (comments that speak of `batch` / `batch2` mean slot[0] / slot[1]); slot[kBigSlot] is the any-frame workspace
    hipStream_t streamx[kMaxStreams - 1] = {};
    hipEvent_t ev_joinx[kMaxStreams - 1] = {};
    hipEvent_t ev_fork2 = nullptr;
    int streams = 2;
    const Workspace* last_ws = nullptr;  // whichever ran last (handle_view)
    ChunkPlan last_plan{};  // ... and its plan (fused: its workspace holds the threshold mask, not the half-size image)
    const uint8_t* last_frames = nullptr;  // ... and the frames it read (the test kit decimates them again for CTAG_DBG_HALF)
    ptrdiff_t last_row_stride = 0, last_frame_stride = 0;
    const ctag_frame_result* last_out = nullptr;  // ... and where its records went (ctag_get_counters)
    // frames of device-memory calls that wait for the any-frame pass (k_markers appends, finish_pending drains)
    DevBuf<PendingRec> d_pending;
    DevBuf<int32_t> d_pending_count;  // 256 bytes: the count, and the sums of ctag_get_counters
    int pending_cap = 65536;
    bool pending_dirty = false;      // a device-memory call was enqueued since the list was last read
    uint64_t pending_gen = 0;        // ... and how many such calls there were
    DevBuf<uint8_t> d_big_frame;     // private copy of a pending frame (host-memory calls upload it again; BGR frames are converted into d_big_gray)
    DevBuf<uint8_t> d_big_gray;
    DevBuf<ctag_frame_result> d_big_result;
    int reruns = 0;                  // frames completed through the any-frame workspace so far (ctag_get_counters)
    // ctag_submit_u8 / ctag_collect: frames in flight, one per call (a camera loop, main.cpp:44-61).  Slot k: a device slab for the frame (filled on
    // copy_stream), a device record and its pinned host copy; `up` = upload done, `done` = record downloaded
    struct AsyncSlot {
        DevBuf<uint8_t> d_frame;
        MappedRec res;
        hipEvent_t up = nullptr, done = nullptr;
        Call host{};  // the caller's frame (valid until its ctag_collect: a pending frame is uploaded again from it)
    };
    static constexpr int kAsyncDepth = 2;
    AsyncSlot aslot[kAsyncDepth];
    int a_head = 0, a_count = 0;     // oldest slot in flight, slots in flight
    int max_chunk = 1024;
    int wave_points = 0;  // CTAG_OPT_WAVE_POINTS
    int fuse_mode = -1;   // CTAG_OPT_FUSED_SWEEP
    int bgr_direct = 1;   // CTAG_OPT_BGR_DIRECT
    bool timing = false;
    bool keep_pre = false;
    // timing (CTAG_OPT_TIMING): one set of CTAG_NUM_STAGES + 1 events per chunk of a public call, read back ONCE after the
    // call's last chunk has been enqueued (a read-back per chunk would serialise the upload / detect overlap being measured)
    std::vector<hipEvent_t> ev;
    int ev_sets_used = 0;
    float stage_ms[CTAG_NUM_STAGES] = {};
    // staging for host-memory entry points: two slabs of `host_sub` frames, filled on copy_stream while the
    // other slab is being processed on `stream`
    DevBuf<uint8_t> d_frames;
    DevBuf<ctag_frame_result> d_results;
    MappedRec res1;                            // the record of a one-frame host call
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[2] = {}, ev_done[2] = {};
    // BGR ingest (ctag_detect_*bgr8*): the gray frames of the chunk in flight, written by k_bgr2gray and read by K1 / K8
    DevBuf<uint8_t> d_gray;
    ptrdiff_t gray_row_stride = 0, gray_frame_stride = 0;
    bool last_was_bgr = false;
    int host_sub = 128;
    int last_chunk_frames = 0;
    char last_error[256] = {0};
    // hipGraph cache of the per-chunk kernel chain (CTAG_OPT_GRAPH): a chunk with the same pointers, sizes and parameters is
    // replayed with one hipGraphLaunch instead of ~25 launches / memsets -- what a stream of single frames (main.cpp:52-59)
    // and the small per-GPU shards of a multi-GPU job repeat thousands of times
    struct GraphKey {
        const void* frames = nullptr;
        void* out = nullptr;
        const void* ws_base = nullptr;
        int n = 0, rows = 0, cols = 0, tw = 0, subpix = 0, dist = 0, keep_pre = 0, channels = 1;
        ptrdiff_t row_stride = 0, frame_stride = 0;
        const void* pend_src = nullptr;  // PendingCtx::src baked into k_markers' arguments (null: no list)
        bool operator==(const GraphKey& o) const {
            return frames == o.frames && out == o.out && ws_base == o.ws_base && n == o.n && rows == o.rows && cols == o.cols && tw == o.tw && subpix == o.subpix &&
                   dist == o.dist && keep_pre == o.keep_pre && channels == o.channels && row_stride == o.row_stride && frame_stride == o.frame_stride &&
                   pend_src == o.pend_src;
        }
    };
    struct GraphEntry {
        GraphKey key;
        ChunkPlan plan;  // what the captured chain runs
        hipGraphExec_t exec = nullptr;
        uint64_t last_use = 0;
    };
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    int use_graph = 2;   // CTAG_OPT_GRAPH: 0 off, 1 every chunk, 2 (default) few-frame calls whose pointers / sizes / parameters repeat;
                         // back to 0 after a capture failed once (the direct path takes over for good)
    GraphKey last_key;   // automatic mode: the previous few-frame chunk (a graph is only worth capturing for a repeat)
    // states of the back ends (SiblingState, ctag_internal.h), each created on first use
    struct {
        void* p = nullptr;
        void (*free_fn)(void*) = nullptr;
    } state[kNumSiblingStates];
};

namespace ctag {
void** handle_state_slot(ctag_handle* h, SiblingState which, void (*free_fn)(void*)) {
    h->state[which].free_fn = free_fn;
    return &h->state[which].p;
}
bool handle_timing(const ctag_handle* h) { return h->timing; }
int handle_device(const ctag_handle* h) { return h->device; }
int handle_dict_cols(const ctag_handle* h) { return h->dict_cols; }
void handle_view(const ctag_handle* h, HandleView* out) {
    out->device = h->device;
    out->ws = h->last_ws && h->last_ws->base ? h->last_ws : nullptr;
    out->last_chunk_frames = h->last_chunk_frames;
    out->keep_pre = h->keep_pre;
    out->dict = h->dict.data();
    out->dict_rows = h->dict_rows;
    out->dict_cols = h->dict_cols;
    out->fused = h->last_plan.fused;
    out->packs1 = !h->last_plan.all_wave && h->last_plan.prescan && h->last_plan.small_cfg;  // (launch_quad_edges' two branches with k_prepack)
    out->frames = h->last_frames;
    out->row_stride = h->last_row_stride;
    out->frame_stride = h->last_frame_stride;
    out->stream = h->stream;
    out->gray = h->last_was_bgr ? h->d_gray.p : nullptr;
    out->gray_row_stride = h->gray_row_stride;
    out->gray_frame_stride = h->gray_frame_stride;
}
}  // namespace ctag

static const char* kStageNames[CTAG_NUM_STAGES] = {"decimate",  "threshold_ccl", "seam_merge", "resolve", "candidates", "quad_pack", "quad_edges", "quad_edges_big",
                                                    "line_sort", "welsch",        "quad_final", "features", "edge_refine", "markers"};

// ---------------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------------
static FrameGeom make_geom(int rows, int cols, int tw, double area_max_fraction = 0.01) {
    FrameGeom g{};
    g.rows = rows;
    g.cols = cols;
    g.hrows = rows / 2;
    g.hcols = cols / 2;
    g.hp = (g.hcols + 63) & ~63;
    g.lp = (g.hcols + 63) & ~63;
    g.tw = tw;
    g.trows = g.hrows / tw + (g.hrows % tw != 0 ? 1 : 0);
    g.tcols = g.hcols / tw + (g.hcols % tw != 0 ? 1 : 0);
    g.tiles_x = (g.hcols + kTileW - 1) / kTileW;
    g.tiles_y = (g.hrows + kTileH - 1) / kTileH;
    g.max_area = (int)std::round(area_max_fraction * g.hcols * g.hrows);  // corner_detector.cpp:88 (0.01 there)
    g.pool_cap = std::max(kPoolCapMin, 256 * g.tiles_x * g.tiles_y);
    return g;
}

// cv::resize INTER_CUBIC tap tables for one axis (resize.cpp: fx = (dx + 0.5) * scale - 0.5 in float, cubic weights with
// A = -0.75 in float, x2048 rounded to nearest-even into short) -- SURVEY App. A.1; CylinderTag.cpp:79.
static void build_resize_tables(int src, int dst, std::vector<int32_t>& ofs, std::vector<int16_t>& coef) {
    ofs.assign((size_t)std::max(dst, 0), 0);
    coef.assign((size_t)std::max(dst, 0) * 4, 0);
    if (dst <= 0) return;
    const double scale = (double)src / dst;
    for (int d = 0; d < dst; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        const int s0 = (int)std::floor(f);
        f -= s0;
        ofs[d] = s0;
        const float A = -0.75f;
        float c[4];
        c[0] = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A;
        c[1] = ((A + 2) * f - (A + 3)) * f * f + 1;
        c[2] = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1;
        c[3] = 1.f - c[0] - c[1] - c[2];
        for (int k = 0; k < 4; k++) {
            long r = std::lrint(c[k] * 2048.f);
            r = std::min(std::max(r, -32768L), 32767L);
            coef[(size_t)d * 4 + k] = (int16_t)r;
        }
    }
}

static void drop_graphs(ctag_handle* h);
static int finish_pending(ctag_handle* h);

// Pool sizes of a workspace.  Batch: what a frame of this size ordinarily needs, scaled with its area so that a 4K frame is not held
// to a 1080p frame's numbers (at 1080p: 2048 candidates, 262 144 cluster points -- a camera frame uses a few hundred / ~50 K).
// Big: bounds no frame can exceed --
//   candidates: components of >= area_min pixels: hw / area_min;
//   cluster points: a component of a pixels has w + h <= 2a, so its reservation min(2(w + h), wh) + 65 <= 4a + 65: 4 hw + 65 candidates;
//   component pool: a 320x30 label tile publishes every component only in the first pass (<= 128); the second publishes the ones
//   of >= area_min pixels (<= 9600 / area_min) or touching the tile border (<= 348 non-adjacent border pixels), at most kSlotCapBig.
struct Caps {
    int pool_cap, cand_cap;
    uint32_t cl_cap;
};
static Caps make_caps(const FrameGeom& g, const ctag_params& prm, bool big) {
    const long long hw = (long long)g.hrows * g.hcols;
    Caps c{};
    if (!big) {
        c.pool_cap = g.pool_cap;
        c.cand_cap = (int)std::max<long long>(kCandCapMin, ((hw / 256 + 63) / 64) * 64);
        c.cl_cap = (uint32_t)std::max<long long>(kClPoolMin, ((hw / 2 + 1023) / 1024) * 1024);
    } else {
        const int amin = std::max(prm.area_min, 1);
        const long long per_tile = std::min<long long>(kSlotCapBig, 352 + (kTileW * kTileH) / amin);
        c.pool_cap = (int)std::max<long long>(g.pool_cap, per_tile * g.tiles_x * g.tiles_y);
        const long long cand = ((hw / amin + 1 + 63) / 64) * 64;
        c.cand_cap = (int)std::max<long long>(kCandCapMin, cand);
        c.cl_cap = (uint32_t)std::max<long long>(kClPoolMin, 4 * hw + 65 * cand + 1024);
    }
    return c;
}

// every stream the handle owns idle: what comes before anything that frees or replaces memory a stream may still read (a workspace, a slab, the
// kernarg storage of a graph exec), and before a failed host-memory call returns.  Never on the path of a call that finds its buffers in place.
// Every stream is waited for whatever the others answered; the first error is returned, and last_error is the caller's to write (HIP_TRY) or to leave.
static hipError_t quiesce(ctag_handle* h) {
    hipError_t first = hipSuccess;
    auto wait = [&](hipStream_t s) {
        const hipError_t e = s ? hipStreamSynchronize(s) : hipSuccess;
        if (first == hipSuccess) first = e;
    };
    wait(h->copy_stream);
    for (hipStream_t x : h->streamx) wait(x);
    wait(h->aux_stream);  // side branch of few-frame calls
    wait(h->stream);
    return first;
}

static size_t label_bytes(const FrameGeom& g, size_t frames) { return frames * g.hrows * g.lp * 2 + 256; }
static size_t tile_bytes(const FrameGeom& g, size_t frames) { return frames * g.tiles_x * g.tiles_y * 4; }

// The arrays of a workspace for `frames` frames (W.g and the caps are set), in the order they lie in its one allocation, each on a 256-byte boundary:
// every array is named here once, with its byte count.  With base == nullptr this only adds up; with the allocation it sets the pointers.  Returns the total.
static size_t carve_workspace(Workspace& W, size_t frames, char* base) {
    const FrameGeom& g = W.g;
    const size_t F = frames, CC = (size_t)W.cand_cap, LC = (size_t)W.line_cap;
    size_t off = 0;
    auto put = [&](auto*& field, size_t bytes) {
        field = base ? reinterpret_cast<std::remove_reference_t<decltype(field)>>(base + off) : nullptr;
        off = (off + bytes + 255) & ~(size_t)255;
    };
    put(W.half, F * g.hrows * g.hp + 256);
    put(W.labels, label_bytes(g, F));
    put(W.tile_base, tile_bytes(g, F));
    put(W.tile_dirty, tile_bytes(g, F));
    put(W.frame_ncomp, F * 4);
    put(W.frame_flags, F * 4);
    put(W.ovf_count, 256);
    put(W.ovf_list, tile_bytes(g, F));
    const size_t pool = F * (size_t)g.pool_cap * 4;
    put(W.parent, pool);
    put(W.root_of, pool);
    put(W.area, pool);
    put(W.xmin, pool);
    put(W.ymin, pool);
    put(W.xmax, pool);
    put(W.ymax, pool);
    put(W.key, pool);
    put(W.pool_tile, pool);
    put(W.member_head, pool);
    put(W.member_next, pool);
    put(W.ncand, F * 4);
    put(W.nroots, F * 4);
    put(W.cand, F * CC * sizeof(Candidate));
    put(W.quads, F * CC * sizeof(QuadOut));
    put(W.line_count, F * 4);
    put(W.clp_used, F * 4);
    put(W.line_long, F * 4);
    put(W.cl_pool, F * (size_t)W.cl_cap * 4 + 16);  // + one element: welsch_restart requests one point past a cluster's last
    put(W.line_desc, F * LC * sizeof(LineDesc));
    put(W.line_sorted, F * LC * 4);
    put(W.line_fit, F * LC * 16);
    put(W.cand_aux, F * CC * sizeof(CandAux));
    put(W.npacks, F * 8);
    put(W.packs, F * CC * 4);
    put(W.pack_order, F * CC * 4);
    put(W.npacks2, F * 8);
    put(W.packs2, F * CC * 4);
    put(W.pack_order2, F * CC * 4);
    put(W.npacks1, F * 8);
    put(W.packs1, F * CC * 4);
    put(W.pack_order1, F * CC * 4);
    put(W.ntotal1, F * CC * 4);
    put(W.welsch_rs, std::min<size_t>(F, kLatencyFrames) * kLatLines * 20 * 6 * 4);
    put(W.quad_derived, F * kQuadStride * 48);
    put(W.quad_index, F * kQuadStride * 4);
    put(W.nquads, F * 4);
    put(W.nfeat, F * 4);
    put(W.status, F * 4);
    put(W.feat0, F * CTAG_MAX_FEATURES * sizeof(FeatureDev));
    put(W.feat1, F * CTAG_MAX_FEATURES * sizeof(FeatureDev));
    put(W.feat2, F * CTAG_MAX_FEATURES * sizeof(FeatureDev));
    put(W.premarkers, F * sizeof(ctag_frame_result));
    put(W.frame_long, F * 4);
    put(W.rz_xofs, (size_t)g.hcols * 4);
    put(W.rz_alpha, (size_t)g.hcols * 8);
    put(W.rz_yofs, (size_t)g.hrows * 4);
    put(W.rz_beta, (size_t)g.hrows * 8);
    return off;
}

static int ensure_workspace(ctag_handle* h, ctag_handle::WsSlot& S, int rows, int cols, int tw, int frames, bool big, bool need_n0) {
    auto refresh = [&](Workspace& W) {
        const Caps c = make_caps(make_geom(rows, cols, tw, h->params.area_max_fraction), h->params, big);
        W.g = make_geom(rows, cols, tw, h->params.area_max_fraction);
        W.g.pool_cap = c.pool_cap;
        W.kp = h->kp;
        W.pick_table = h->d_pick_table.p;
        W.pick_table16 = reinterpret_cast<const uint16_t*>(h->d_pick_table.p + (size_t)kPickN * 200);
        W.aux_stream = h->aux_stream;
        W.ev_fork = h->ev_fork;
        W.ev_join = h->ev_join;
        W.big = big;
    };
    auto ensure_n0 = [&]() -> int {  // the searches -> sums hand-over of k_edge_refine<1> / <2>: 0.8 MB per frame, batches with corner_subpix only
        const size_t need = (size_t)S.cap * CTAG_MAX_FEATURES * 2 * 4 * 128;
        if (need_n0 && S.n0.cap < need) {
            HIP_TRY(quiesce(h));
            drop_graphs(h);
            HIP_TRY(S.n0.grow(need));
        }
        S.ws.refine_n0 = S.n0.p;
        return CTAG_OK;
    };
    if (S.ws.base && S.rows == rows && S.cols == cols && S.cap >= frames) {
        refresh(S.ws);
        S.tw = tw;
        return ensure_n0();
    }
    if (S.ws.base) {
        HIP_TRY(quiesce(h));
        drop_graphs(h);  // they hold pointers into the old workspace
        S.mem.release();
        S.n0.release();
        if (h->last_ws == &S.ws) h->last_ws = nullptr;
        S.ws = Workspace{};
        S.cap = 0;
    }
    Workspace& W = S.ws;
    refresh(W);
    const Caps caps = make_caps(W.g, h->params, big);
    W.cand_cap = caps.cand_cap;
    W.line_cap = 4 * caps.cand_cap;
    W.cl_cap = caps.cl_cap;
    const FrameGeom& g = W.g;
    const size_t F = (size_t)frames;
    HIP_TRY(S.mem.grow(carve_workspace(W, F, nullptr)));
    W.base = S.mem.p;
    W.bytes = carve_workspace(W, F, S.mem.p);
    W.chunk_frames = frames;
    // the label image's invariant: a tile whose tile_dirty is 0 holds zeros
    HIP_TRY(hipMemsetAsync(W.labels, 0, label_bytes(g, F), h->stream));
    HIP_TRY(hipMemsetAsync(W.tile_dirty, 0, tile_bytes(g, F), h->stream));
    HIP_TRY(hipMemsetAsync(W.tile_base, 0, tile_bytes(g, F), h->stream));  // the fused sweep leaves the entries of tiles without foreground alone: they must stay valid offsets
    {   // tap tables of the general decimation (used for odd sizes only; a few KB)
        std::vector<int32_t> xo, yo;
        std::vector<int16_t> al, be;
        build_resize_tables(cols, g.hcols, xo, al);
        build_resize_tables(rows, g.hrows, yo, be);
        HIP_TRY(hipMemcpy(W.rz_xofs, xo.data(), xo.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(W.rz_alpha, al.data(), al.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(W.rz_yofs, yo.data(), yo.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(W.rz_beta, be.data(), be.size() * 2, hipMemcpyHostToDevice));
    }
    S.rows = rows;
    S.cols = cols;
    S.tw = tw;
    S.cap = frames;
    return ensure_n0();
}

// ---------------------------------------------------------------------------------------------------
// which kernel forms a chunk runs
// ---------------------------------------------------------------------------------------------------
namespace ctag {
// The one reader of the chain's developer aids.  Most are read once, at the first call; CTAG_GENERAL_RESIZE and the phase clocks of
// K2 / K6 on every call (a test sets CTAG_GENERAL_RESIZE between calls of one process).
DevKnobs dev_knobs() {
    static const DevKnobs once = [] {
        DevKnobs k;
        const struct { const char* name; int* v; int lo; } num[] = {  // lo: the least value taken
            {"CTAG_FUSED_SWEEP", &k.fused_sweep, INT_MIN}, {"CTAG_FUSE_GENERAL", &k.fuse_general, INT_MIN}, {"CTAG_DEC_MIN_BAND", &k.dec_min_band, INT_MIN},
            {"CTAG_PACK_MAX", &k.pack_max, INT_MIN}, {"CTAG_BIG_POINTS", &k.big_points, INT_MIN}, {"CTAG_PRESCAN", &k.prescan, INT_MIN},
            {"CTAG_MASK_SCAN", &k.mask_scan, INT_MIN}, {"CTAG_PACK_GX", &k.pack_gx, INT_MIN}, {"CTAG_SCAN_GX", &k.scan_gx, 1}, {"CTAG_MSCAN_GX", &k.mscan_gx, 1},
            {"CTAG_BIG_COLS", &k.big_cols, INT_MIN}, {"CTAG_WELSCH_GS", &k.welsch_gs, 1}, {"CTAG_WELSCH_GX", &k.welsch_gx, 1},  // (k_welsch's two row ranges each own a class of edges)
            {"CTAG_REFINE_GX", &k.refine_gx, INT_MIN}, {"CTAG_REFINE_SUMS_GX", &k.refine_sums_gx, INT_MIN}, {"CTAG_REFINE_XCD", &k.refine_xcd, INT_MIN},
            {"CTAG_REFINE_LARGE", &k.refine_large, INT_MIN}, {"CTAG_STREAMS_MIN", &k.streams_min, 2 * kLatencyFrames + 2}};
        for (const auto& e : num)
            if (getenv(e.name)) *e.v = std::max(e.lo, atoi(getenv(e.name)));
        k.feat_stamps = getenv("CTAG_FEAT_STAMPS") != nullptr;
        k.stamps = getenv("CTAG_CCL_STAMPS") != nullptr || getenv("CTAG_QUAD_STAMPS") != nullptr || k.feat_stamps;  // they synchronise inside the chain
        return k;
    }();
    DevKnobs k = once;
    k.general_resize = getenv("CTAG_GENERAL_RESIZE") != nullptr;
    k.ccl_stamps = getenv("CTAG_CCL_STAMPS") != nullptr;
    k.quad_stamps = getenv("CTAG_QUAD_STAMPS") != nullptr;
    return k;
}

unsigned long long* Stamps::zeroed(hipStream_t s) {
    if (!d && hipMalloc(reinterpret_cast<void**>(&d), kSlots * sizeof(*d)) != hipSuccess) return d = nullptr;
    (void)hipMemsetAsync(d, 0, kSlots * sizeof(*d), s);
    return d;
}
void Stamps::read(hipStream_t s, unsigned long long* h, int n) const {
    (void)hipStreamSynchronize(s);
    memset(h, 0, n * sizeof(*h));
    if (d) (void)hipMemcpy(h, d, n * sizeof(*d), hipMemcpyDeviceToHost);
}

void ensure_dynamic_lds(const void* fn, size_t bytes) {
    if (bytes <= 64 * 1024) return;  // what every kernel may ask for as it is
    int dev = 0;
    (void)hipGetDevice(&dev);
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> have;  // (kernel, device) -> bytes it may ask for
    const std::lock_guard<std::mutex> lock(mu);
    size_t& h = have[{fn, dev}];
    if (bytes > h) {
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        h = bytes;
    }
}

ChunkPlan plan_chunk(const PlanIn& in) {
    const DevKnobs& K = in.knobs;
    const int n = in.nframes, hrows = in.rows / 2, hcols = in.cols / 2;
    ChunkPlan pl{};
    pl.nframes = n, pl.channels = in.channels, pl.latency = n <= kLatencyFrames;
    pl.ccl_stamps = K.ccl_stamps, pl.quad_stamps = K.quad_stamps, pl.feat_stamps = K.feat_stamps;
    const bool aligned = (((uintptr_t)in.frames | (uintptr_t)in.frame_stride | (uintptr_t)in.row_stride) & 15) == 0;
    // The fused sweep (k_decimate_mask + the mask front end of K2) takes batches of frames whose half size is a multiple of 320 x 5 (round 6; 1080p, 4K, 8K,
    // 1920x1200, 1280x720, 2560x1440, 640x480 ...) with the reference's 5x5 window and 16-byte aligned rows; everything else keeps the two-kernel form with `half`.
    // CTAG_OPT_FUSED_SWEEP: 0 never, 1 batches (default), 2 whenever the frame size allows.
    const int fuse = in.fuse_mode >= 0 ? in.fuse_mode : K.fused_sweep >= 0 ? K.fused_sweep : 1;
    // half width a multiple of the labelling tile (320 columns: whole mask words, whole threshold tiles, whole 16-pixel lanes), half height of whole
    // threshold-tile rows; 1080p / 4K / 8K take the compile-time-band build, the others the run-time-band one
    const bool fuse_size = fuse && !(in.rows & 1) && !(in.cols & 1) && in.tw == 5 && hcols >= kTileW && hcols % kTileW == 0 && hrows >= 10 && hrows % 5 == 0;
    // bands of the run-time-band build: a multiple of four (the four waves of a block), about 90-150 rows each; reproduces the 135-row bands of 1080p / 4K / 8K
    const int fuse_bands = 4 * ((hrows + 599) / 600), fuse_xb = (hcols + kFuseCols - 1) / kFuseCols;
    // few frames: short bands and the latency-tuned kernels of the two-kernel form instead of one 4-wave block per frame walking 135-row bands
    const bool fuse_batch = fuse >= 2 || (long)n * fuse_xb * fuse_bands >= 2048;
    // BGR frames take the fused sweep or none: a call of a few of them converts first (k_bgr2gray) and takes the gray chain, as gray calls of that size do;
    // so do frames whose 32-bit pixel offsets k_edge_refine could not address (check_args has seen the gray pitch only)
    pl.bgr_direct = in.bgr_direct && fuse_size && fuse_batch && aligned && in.row_stride < (1 << 24) && (long long)in.rows * in.row_stride <= 0xffffffffLL;
    pl.fused = fuse_size && aligned && (in.channels == 3 || fuse_batch);
    // K1.  Batches zero the chain's counters with a kernel of their own at its head; a few frames pass them to the run-time-band decimation,
    // and get the kernel right before the decimation where it takes another form
    const bool general = (in.rows & 1) || (in.cols & 1) || K.general_resize;  // odd sizes (env: developer aid, runs even sizes through the general kernel)
    pl.zero_first = !pl.latency;
    pl.dec_zero_kernel = pl.latency && (pl.fused || general);
    pl.dec_zero_list = pl.latency && !pl.dec_zero_kernel;
    if (pl.fused) {
        const bool exact = hcols % kFuseCols == 0 && hrows % 135 == 0 && (hrows / 135) % 4 == 0;  // (CTAG_FUSE_GENERAL: developer aid, 1 runs 1080p / 4K / 8K through the run-time-band build)
        pl.dec = exact && !K.fuse_general ? DecForm::Mask : DecForm::MaskBands;
        pl.dec_xblocks = fuse_xb, pl.dec_bands = exact && !K.fuse_general ? 0 : fuse_bands, pl.dec_yblocks = pl.dec_bands ? pl.dec_bands / 4 : hrows / 540;
    } else if (general) {
        pl.dec = DecForm::General;
    } else {
        const int xblocks = ((hcols + 7) / 8 + 63) / 64;
        int bands = 4 * ((hrows + 4 * CTAG_DEC_BAND_MAX - 1) / (4 * CTAG_DEC_BAND_MAX));
        // small batches (a single frame through ctag_detect_u8): a band is a sequential walk of a wave, so shorter bands -- more
        // waves -- cut the latency (one 1080p frame: 135-row bands 0.19 ms, 15-row bands 0.034 ms, 8 rows 21 us, 4-row bands < 0.02 ms); a full batch keeps the tall ones
        while ((long)n * xblocks * bands < 2048 && (hrows + 2 * bands - 1) / (2 * bands) >= K.dec_min_band) bands *= 2;
        pl.dec_band_rows = (hrows + bands - 1) / bands, pl.dec_yblocks = bands / 4, pl.dec_xblocks = xblocks;
        const bool has_tail = (hcols & (CTAG_RESIZE_SIMD_LANES - 1)) != 0;
        if (pl.dec_band_rows == 135 && pl.dec_zero_list) pl.dec_zero_kernel = true;  // (a few frames get here only with CTAG_DEC_MIN_BAND) the forms below do not zero
        if (aligned && !has_tail && (hcols & 15) == 0 && pl.dec_band_rows == 135) {
            pl.dec = DecForm::Wide;  // a lane owns 16 output pixels.  Same-box A/B on 4096 1080p frames: 2.276 -> 2.209 ms (5 waves per SIMD: 2.28)
            pl.dec_xblocks = (hcols / 16 + 63) / 64;
        } else {
            pl.dec = !aligned ? DecForm::Unaligned : pl.dec_band_rows == 135 && !has_tail ? DecForm::Banded135 : DecForm::Banded;
        }
    }
    pl.ccl = pl.fused ? CclForm::Mask : in.tw == 5 ? CclForm::Tw5 : CclForm::Any;
    // K6
    pl.refprm = in.kp.thr_line == 1.8f && in.kp.thr_expand == 1.2f && in.kp.c2_far == 2 && in.kp.c2_near == 1 && in.kp.expand_eps == 3.0e-6f;
    pl.pack_max = K.pack_max > 0 ? std::min(K.pack_max, kSG) : kSG;
    pl.big_points = in.wave_points > 0 ? in.wave_points : K.big_points > 0 ? K.big_points : (pl.latency ? kLatencyBigPoints : 0x7fffffff);
    pl.small_cfg = (long long)hrows * hcols <= 960LL * 600;  // up to 1920x1200 frames
    // chunks that took the fused sweep: the silhouettes come from its threshold mask (k_silhouette_mask), whatever the frame size; CTAG_MASK_SCAN=0 (developer aid, A/B) turns it off
    pl.mask_scan = pl.fused && !pl.latency && K.mask_scan != 0 && (hcols & 63) == 0;
    // other batches of frames above 1920x1200: the silhouettes of the packed components come from a kernel of their own (PHASE 3 of k_quad_edges_packed)
    // (measured: 4K frames, quad_edges 4.07 -> 2.78 ms per 1024 frames; 1080p frames 3.88 -> 4.01 per 4096 -- there a component's box is ~75 x 20, the
    // packed build's eight components per wave amortise the chain of dependent loads a component costs better than a wave per component does; a
    // scan-only kernel with the packs' own 8 x 8 lanes at 4 / 5 / 6 waves per SIMD: 4.09 / 4.11 / 4.14 -- the scan is not what the small build waits for)
    pl.prescan = pl.mask_scan || (!pl.latency && (K.prescan == 2 || (K.prescan == 1 && !pl.small_cfg)));
    // A few frames per call fork the whole-wave components off the packs ... unless every component is a whole-wave one (the default of such calls: a frame
    // has a few hundred components and the GPU a thousand SIMDs, so the stage is as long as the longest boundary either way, and without packs there is
    // nothing to fork or join: 0.476 -> 0.46 ms on test.bmp)
    pl.all_wave = pl.latency && pl.big_points <= 1;
    pl.fork = pl.latency && !pl.all_wave;
    pl.pack_gx = K.pack_gx > 0 ? K.pack_gx : 32;
    pl.scan_gx = K.scan_gx, pl.mscan_gx = K.mscan_gx;  // (k_silhouette_mask: blocks of one wave, two components each per trip)
    pl.big_cols = K.big_cols > 0 ? K.big_cols : (pl.latency ? 512 : 4);  // (few frames: every component a block of its own up to 512 per frame; a 2666-blob frame 3.0 -> 2.5 ms against 128)
    pl.big_max_gx = pl.latency ? 8 : 2;
    // k_welsch: welsch_gs blocks for the edges of <= 10 points, 320 per block; welsch_gx groups of kWE edges with a block of their own, a block loops when a frame
    // has more (the synthetic frames have ~210 edges of more than 10 points: 17.8 groups)
    pl.welsch_gs = K.welsch_gs, pl.welsch_gx = K.welsch_gx;
    // K7 - K9: a few frames take the kernels tuned for latency; edgeRefine (corner_subpix) of a batch is split into searches and sums
    if (!in.corner_subpix) pl.refine = RefineForm::None;
    else if (pl.latency || !CTAG_REFINE_SPLIT) pl.refine = RefineForm::One;
    else if (K.refine_large && (long long)in.rows * in.cols > 1920LL * 1200) pl.refine = RefineForm::SplitLarge;  // (CTAG_REFINE_LARGE=0: the small staging region for every frame size, A/B)
    else pl.refine = K.refine_xcd & 1 ? RefineForm::SplitLooping : RefineForm::Split;
    pl.refine_gx = K.refine_gx, pl.refine_sums_gx = K.refine_sums_gx;  // looping blocks per frame of the searches / of k_edge_refine<2>
    return pl;
}
}  // namespace ctag

// (BGR frames: the 32-bit pixel offsets are those of the gray slab the frames are converted into.  The direct form, which reads the BGR rows themselves,
// is only chosen for a row_stride and a frame span within the same limits: plan_chunk, pl.bgr_direct)
static int check_args(ctag_handle* h, const Call& c) {
    const ptrdiff_t gray_stride = c.channels == 3 ? ((ptrdiff_t)c.cols + 15) & ~(ptrdiff_t)15 : c.row_stride;
    if (!h || !c.frames || c.n < 0 || c.rows < 4 || c.cols < 4 || c.row_stride < (ptrdiff_t)c.cols * c.channels || c.adaptive_thresh < 1 || c.subpix_dist < 0)
        return CTAG_ERR_ARG;
    if (c.adaptive_thresh > kMaxThreshWin) return CTAG_ERR_UNSUPPORTED;
    if (c.rows / 2 > 16000 || c.cols / 2 > 16000) return CTAG_ERR_UNSUPPORTED;
    if (gray_stride >= (1 << 24) || (long long)c.rows * gray_stride > 0xffffffffLL) return CTAG_ERR_UNSUPPORTED;  // 32-bit pixel offsets (k_edge_refine)
    return CTAG_OK;
}

static DetectParams detect_params(const ctag_handle* h, const Call& c) {
    DetectParams p{c.adaptive_thresh, c.corner_subpix, c.subpix_dist, h->feature_size, h->dict_rows, h->dict_cols, h->d_dict.p, h->d_dict_pos.p};
    p.channels = c.channels;
    return p;
}
// c: frames in the CALLER's device memory -- what one of them that needs the any-frame pass is read from again
static PendingCtx pending_ctx(const ctag_handle* h, const Call& c) {
    return PendingCtx{h->d_pending.p, h->d_pending_count.p, h->pending_cap, c.frames, (int64_t)c.frame_stride, (int64_t)c.row_stride,
                      c.rows, c.cols, c.channels, c.adaptive_thresh, c.corner_subpix, c.subpix_dist};
}

// "the last chunk" of the probes and counters (handle_view, ctag_get_counters)
static void note_last(ctag_handle* h, const Workspace& ws, const ChunkPlan& pl, const Call& c, const ctag_frame_result* out_dev) {
    h->last_ws = &ws, h->last_plan = pl, h->last_out = out_dev;
    h->last_frames = pl.channels == 3 ? nullptr : c.frames;  // (BGR frames handed to the chain as they are: no gray rows for the half-size probe to decimate)
    h->last_row_stride = c.row_stride, h->last_frame_stride = c.frame_stride;
}

// enqueue the whole pipeline for the c.n device-resident frames of `c` (c.n <= workspace capacity) on stream s; evs: CTAG_NUM_STAGES + 1 timing events or null
static int enqueue_chunk(ctag_handle* h, const Workspace& ws, const Call& c, ctag_frame_result* out_dev, hipEvent_t* evs, const PendingCtx& pend, hipStream_t s) {
    const DetectParams p = detect_params(h, c);
    const ChunkPlan pl = plan_chunk(PlanIn{ws.g.rows, ws.g.cols, ws.g.tw, c.n, p.channels, p.corner_subpix, c.frames, c.frame_stride, c.row_stride, ws.kp,
                                           h->fuse_mode, h->wave_points, h->bgr_direct != 0, dev_knobs()});
    note_last(h, ws, pl, c, out_dev);
    if (pl.zero_first) HIP_TRY(launch_zero_counters(pl, ws, s));
    int st = 0;
    auto mark = [&](int i) -> hipError_t { return evs ? hipEventRecord(evs[i], s) : hipSuccess; };
    HIP_TRY(mark(0));
    if (p.channels == 3 && !pl.fused) return CTAG_ERR_UNSUPPORTED;  // (detect_bgr_device_impl has checked: BGR frames go through k_bgr2gray otherwise)
    HIP_TRY(launch_decimate(pl, c.frames, c.frame_stride, c.row_stride, ws, s));
    HIP_TRY(mark(++st));
    HIP_TRY(launch_threshold_ccl(pl, ws, s));
    HIP_TRY(mark(++st));
    HIP_TRY(launch_seam_merge(pl, ws, s));
    HIP_TRY(mark(++st));
    HIP_TRY(launch_resolve(pl, ws, s));
    HIP_TRY(mark(++st));
    HIP_TRY(launch_candidates(pl, ws, s));
    HIP_TRY(mark(++st));
    HIP_TRY(launch_quads(pl, ws, s, evs ? evs + st + 1 : nullptr));  // records one event after each of its first five kernels
    st += 5;
    HIP_TRY(mark(++st));
    HIP_TRY(launch_features(pl, ws, p, s));
    HIP_TRY(mark(++st));
    HIP_TRY(launch_edge_refine(pl, c.frames, c.frame_stride, c.row_stride, ws, p, s));
    HIP_TRY(mark(++st));
    Workspace wtmp = ws;
    if (!h->keep_pre) wtmp.premarkers = nullptr;
    HIP_TRY(launch_markers(pl, wtmp, p, out_dev, pend, s));
    HIP_TRY(mark(++st));
    return CTAG_OK;
}

// an exec owns the kernarg storage of its launches: nothing it enqueued may still be running when it is destroyed
static void graphs_idle(ctag_handle* h) {
    if (!h->graphs.empty()) (void)quiesce(h);
}
static void drop_graphs(ctag_handle* h) {
    graphs_idle(h);
    for (auto& g : h->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
}

// replay (or first capture) the chunk as a hipGraph; any failure disables the graph path for this handle and the caller
// falls back to direct launches -- results are the same either way
static bool run_chunk_graph(ctag_handle* h, const ctag_handle::GraphKey& key, const Call& c, ctag_frame_result* out_dev, const PendingCtx& pend) {
    const Workspace& W = h->slot[0].ws;
    constexpr size_t kMaxGraphs = 8;
    ctag_handle::GraphEntry* hit = nullptr;
    for (auto& g : h->graphs)
        if (g.key == key) hit = &g;
    if (!hit) {
        if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed) != hipSuccess) return false;
        const int r = enqueue_chunk(h, W, c, out_dev, nullptr, pend, h->stream);
        hipGraph_t graph = nullptr;
        const hipError_t e = hipStreamEndCapture(h->stream, &graph);
        if (r != CTAG_OK || e != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            return false;
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess || !exec) {
            (void)hipGetLastError();
            return false;
        }
        if (h->graphs.size() >= kMaxGraphs) {  // evict the least recently used
            size_t lru = 0;
            for (size_t i = 1; i < h->graphs.size(); i++)
                if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
            graphs_idle(h);  // the victim may still be executing
            (void)hipGraphExecDestroy(h->graphs[lru].exec);
            h->graphs.erase(h->graphs.begin() + (ptrdiff_t)lru);
        }
        h->graphs.push_back(ctag_handle::GraphEntry{key, h->last_plan, exec, 0});
        hit = &h->graphs.back();
    }
    hit->last_use = ++h->graph_clock;
    note_last(h, W, hit->plan, c, out_dev);
    return hipGraphLaunch(hit->exec, h->stream) == hipSuccess;
}

// one piece of a call: the frames of `c` through workspace slot k on stream k.  alone: the call's pieces all run on `stream` (slot 0), one
// behind the other -- such a piece may be timed and replayed as a graph
static int run_chunk(ctag_handle* h, int k, bool alone, const Call& c, ctag_frame_result* out_dev, const PendingCtx& pend) {
    const Workspace& W = h->slot[k].ws;
    const hipStream_t s = k ? h->streamx[k - 1] : h->stream;
    h->last_chunk_frames = c.n;
    if (pend.list) {
        h->pending_dirty = true;
        h->pending_gen++;
    }
    hipEvent_t* evs = nullptr;
    if (h->timing) {  // (the call is `alone`: detect_device_impl)
        const size_t need = (size_t)(h->ev_sets_used + 1) * (CTAG_NUM_STAGES + 1);
        while (h->ev.size() < need) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            h->ev.push_back(e);
        }
        evs = h->ev.data() + (size_t)h->ev_sets_used * (CTAG_NUM_STAGES + 1);
        h->ev_sets_used++;
    }
    static const bool stamps = dev_knobs().stamps;  // developer aids that synchronise inside the chain (no graph capture around them)
    // what a captured chain depends on besides the handle's options (a change of those drops the graphs)
    const ctag_handle::GraphKey key{c.frames, out_dev, W.base, c.n, W.g.rows, W.g.cols, c.adaptive_thresh, c.corner_subpix, c.subpix_dist, h->keep_pre ? 1 : 0,
                                    c.channels, c.row_stride, c.frame_stride, pend.list ? (const void*)pend.src : nullptr};
    bool graph = alone && h->use_graph == 1;
    if (alone && h->use_graph == 2 && c.n <= kLatencyFrames) {  // one frame per call in a loop (main.cpp:52-59): same staging buffers, same sizes every time
        graph = key == h->last_key;
        h->last_key = key;
    }
    if (!evs && graph && !stamps) {
        if (run_chunk_graph(h, key, c, out_dev, pend)) return CTAG_OK;
        h->use_graph = 0;  // capture / instantiate / launch failed: direct launches from now on
        drop_graphs(h);
    }
    return enqueue_chunk(h, W, c, out_dev, evs, pend, s);
}

// public entry points call begin_timings() before their first chunk and collect_timings() after their last
static void begin_timings(ctag_handle* h) {
    h->ev_sets_used = 0;
    for (int i = 0; i < CTAG_NUM_STAGES; i++) h->stage_ms[i] = 0.f;
}
static int collect_timings(ctag_handle* h) {
    const int sets = h->ev_sets_used;
    h->ev_sets_used = 0;
    if (!h->timing || sets == 0) return CTAG_OK;
    HIP_TRY(hipEventSynchronize(h->ev[(size_t)sets * (CTAG_NUM_STAGES + 1) - 1]));
    for (int k = 0; k < sets; k++) {
        const hipEvent_t* evs = h->ev.data() + (size_t)k * (CTAG_NUM_STAGES + 1);
        for (int i = 0; i < CTAG_NUM_STAGES; i++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, evs[i], evs[i + 1]));
            h->stage_ms[i] += ms;
        }
    }
    return finish_pending(h);  // the call has waited anyway: frames that need the any-frame pass are completed now (outside the stage times)
}

// src: where the frames of this call live in the CALLER's device memory (what a frame that needs the any-frame pass is read from
// again: `c` itself for gray calls, the BGR source for colour calls), or null for host-memory calls -- their frames
// pass through staging slabs that are reused, and they find CTAG_PENDING records in the results they download
static int detect_device_impl(ctag_handle* h, const Call& c, ctag_frame_result* out_dev, const Call* src) {
    const int rc = check_args(h, c);
    if (rc != CTAG_OK) return rc;
    if (c.n == 0) return CTAG_OK;
    HIP_TRY(hipSetDevice(h->device));
    const int chunk = std::min(c.n, h->max_chunk);
    static const int streams_min = dev_knobs().streams_min;
    const bool two_env = streams_min > 0;
    const int two_min = two_env ? streams_min : 256;
    // chunks of [448, 1024) frames stay on one stream: their halves (224-511 frames) leave the stage kernels' grids a partial last round of
    // blocks on each stream.  Measured (round 5, 1080p, two handles alternating, K frames/s split / whole): 256: 189 / 178, 384: 213 / 214,
    // 512: 222 / 237, 640: 229 / 234, 768: 232 / 234, 1024: 247 / 241, 2048: 255 / 250 (tools/step_overlap.py).
    // Scope of the rule: it looks at the call's chunk = min(n, max_chunk), measured at 1080p only -- frames of other sizes take it by frame COUNT all
    // the same (a 4K frame is four 1080p frames of blocks: its chunks of 112-255 frames, the equivalent window, are below two_min and stay whole anyway); the ragged tail of
    // a longer call (n = 1100 at max_chunk 1024: 512 + 512 + 76) is a piece of its own on the next stream; CTAG_STREAMS_MIN (developer aid) replaces the rule altogether.
    const bool whole = !two_env && chunk >= 448 && chunk < 1024;
    const bool split = h->streams >= 2 && !h->timing && chunk >= two_min && !whole && h->streamx[0];
    const int ns = split ? std::min(h->streams, (int)ctag_handle::kMaxStreams) : 1;
    // two halves of every chunk side by side (see WsSlot batch2).  With CTAG_OPT_TIMING the chunk stays on one stream: the HIP events
    // around a kernel would otherwise time the other stream's kernels as well.
    // (measured, round 4: pieces of 1024 / 512 frames instead of half a chunk 226 / 203 K frames/s against 231 K; the second stream half a
    // piece out of phase -- one stream in its memory-bound sweep while the other computes -- 216-227 K: the kernels' tails want large pieces)
    const int piece = (chunk + ns - 1) / ns;
    for (int k = 0; k < ns; k++) {
        ctag_handle::WsSlot& S = h->slot[k];
        const int wr = ensure_workspace(h, S, c.rows, c.cols, c.adaptive_thresh, std::max(piece, S.rows == c.rows && S.cols == c.cols ? S.cap : 0), false,
                                        c.corner_subpix != 0 && chunk > kLatencyFrames);
        if (wr != CTAG_OK) return wr;
    }
    if (split) HIP_TRY(hipEventRecord(h->ev_fork2, h->stream));
    for (int k = 1; k < ns; k++) HIP_TRY(hipStreamWaitEvent(h->streamx[k - 1], h->ev_fork2, 0));
    for (int f0 = 0, k = 0; f0 < c.n; f0 += piece, k = (k + 1) % ns) {
        const int m = std::min(piece, c.n - f0);
        const int r = run_chunk(h, k, !split, c.sub(f0, m), out_dev + f0, src ? pending_ctx(h, src->sub(f0, m)) : PendingCtx{});
        if (r != CTAG_OK) return r;
    }
    for (int j = 1; j < ns; j++) {
        HIP_TRY(hipEventRecord(h->ev_joinx[j - 1], h->streamx[j - 1]));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_joinx[j - 1], 0));
    }
    return CTAG_OK;
}

// ---------------------------------------------------------------------------------------------------
// BGR ingest: cvtColor(BGR2GRAY) of the reference's stream loop (main.cpp:36,52-54) on the device
// ---------------------------------------------------------------------------------------------------
// OpenCV's 8-bit BGR2GRAY is fixed point: (B*1868 + G*9617 + R*4899 + 8192) >> 14 (RGB2Gray<uchar>: B2Y, G2Y, R2Y at yuv_shift 14,
// [OCV-recall of color_rgb.simd.hpp]; the same formula as the host BMP reader, csrc/ctag_io.h).  A lane converts four pixels:
// three aligned words in, one word out -- consecutive lanes read consecutive 12-byte groups, so a wave's loads are contiguous.
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t* __restrict__ bgr, ptrdiff_t frame_stride, ptrdiff_t row_stride, uint8_t* __restrict__ gray,
                                                  ptrdiff_t gframe_stride, ptrdiff_t grow_stride, int rows, int cols, int aligned) {
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, f = blockIdx.z;
    if (x4 >= cols) return;
    const uint8_t* src = bgr + (ptrdiff_t)f * frame_stride + (ptrdiff_t)y * row_stride + (ptrdiff_t)x4 * 3;
    uint8_t* dst = gray + (ptrdiff_t)f * gframe_stride + (ptrdiff_t)y * grow_stride + x4;
    if (aligned && x4 + 3 < cols) {
        const uint32_t w0 = reinterpret_cast<const uint32_t*>(src)[0], w1 = reinterpret_cast<const uint32_t*>(src)[1], w2 = reinterpret_cast<const uint32_t*>(src)[2];
        // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        const uint32_t g0 = gray_of(w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu);
        const uint32_t g1 = gray_of(w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu);
        const uint32_t g2 = gray_of((w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu);
        const uint32_t g3 = gray_of((w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24);
        *reinterpret_cast<uint32_t*>(dst) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    } else {
        for (int k = 0; k < 4 && x4 + k < cols; k++) dst[k] = (uint8_t)gray_of(src[3 * k], src[3 * k + 1], src[3 * k + 2]);
    }
}

// gray slab for `frames` frames of rows x cols (rows padded to 16 bytes); grows only
static int ensure_gray(ctag_handle* h, int frames, int rows, int cols) {
    const ptrdiff_t pitch = ((ptrdiff_t)cols + 15) & ~(ptrdiff_t)15;
    const size_t need = (size_t)pitch * rows * (size_t)frames;
    if (h->d_gray.cap < need) {
        HIP_TRY(quiesce(h));
        drop_graphs(h);  // they hold the old slab's address
        HIP_TRY(h->d_gray.grow(need));
    }
    h->gray_row_stride = pitch;
    h->gray_frame_stride = pitch * rows;
    return CTAG_OK;
}

// the BGR frames of `bgr` -> gray, into `gray` (packed rows of the slab's pitch) or, by default, into the chunk slab
static int enqueue_bgr2gray(ctag_handle* h, const Call& bgr, uint8_t* gray = nullptr) {
    const int aligned = ((reinterpret_cast<uintptr_t>(bgr.frames) | (uintptr_t)bgr.row_stride | (uintptr_t)bgr.frame_stride) & 3u) == 0 ? 1 : 0;
    const ptrdiff_t pitch = ((ptrdiff_t)bgr.cols + 15) & ~(ptrdiff_t)15;  // == gray_row_stride of the chunk slab
    hipLaunchKernelGGL(k_bgr2gray, dim3((bgr.cols + 1023) / 1024, bgr.rows, bgr.n), dim3(256), 0, h->stream, bgr.frames, bgr.frame_stride, bgr.row_stride,
                       gray ? gray : h->d_gray.p, gray ? pitch * bgr.rows : h->gray_frame_stride, gray ? pitch : h->gray_row_stride, bgr.rows, bgr.cols, aligned);
    HIP_TRY(hipGetLastError());
    return CTAG_OK;
}
// `c` with its frames replaced by gray ones
static Call as_gray(const Call& c, const uint8_t* gray, ptrdiff_t row_stride, ptrdiff_t frame_stride) {
    Call g = c;
    g.frames = gray, g.channels = 1, g.row_stride = row_stride, g.frame_stride = frame_stride;
    return g;
}

// ---------------------------------------------------------------------------------------------------
// the any-frame pass: frames that exceeded a pool of the batch workspace
// ---------------------------------------------------------------------------------------------------
// the chain of the handle's own calls idle: `stream` and its side branch.  Not quiesce: this is the wait of finish_pending, which every ctag_sync behind a
// device-memory call goes through -- a steady-state path -- and what it reads was written on `stream` (the extra streams have joined it by event)
static int wait_chain(ctag_handle* h) {
    if (h->aux_stream) HIP_TRY(hipStreamSynchronize(h->aux_stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return CTAG_OK;
}

// One frame in device memory (gray, or BGR for channels == 3) through the workspace whose pools hold any frame of its size; the record
// goes to out_dev.  Enqueued on the handle's stream; the caller waits.  The reference has none of the batch workspace's limits
// (corner_detector.cpp:81-107 keeps every component of [area_min, 1 %], :171-405 walks them all), so neither does a result.
static int rerun_frame(ctag_handle* h, const Call& c, ctag_frame_result* out_dev) {
    ctag_handle::WsSlot& big = h->slot[ctag_handle::kBigSlot];
    const int wr = ensure_workspace(h, big, c.rows, c.cols, c.adaptive_thresh, 1, true, false);
    if (wr != CTAG_OK) return wr;
    Call g = as_gray(c, c.frames, c.row_stride, c.row_stride * c.rows);
    if (c.channels == 3) {
        const ptrdiff_t pitch = ((ptrdiff_t)c.cols + 15) & ~(ptrdiff_t)15;
        HIP_TRY(h->d_big_gray.grow((size_t)pitch * c.rows));
        const int r = enqueue_bgr2gray(h, c, h->d_big_gray.p);
        if (r != CTAG_OK) return r;
        g = as_gray(c, h->d_big_gray.p, pitch, pitch * c.rows);
    }
    h->last_chunk_frames = 1;
    h->reruns++;
    return enqueue_chunk(h, big.ws, g, out_dev, nullptr, PendingCtx{}, h->stream);
}

// drain the list device-memory calls left (see handle_finish_pending, ctag_internal.h)
static int finish_pending(ctag_handle* h) {
    if (!h->pending_dirty) return CTAG_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (wait_chain(h) != CTAG_OK) return CTAG_ERR_HIP;
    int count = 0;
    HIP_TRY(hipMemcpy(&count, h->d_pending_count.p, 4, hipMemcpyDeviceToHost));
    h->pending_dirty = false;
    if (count <= 0) return CTAG_OK;
    const int take = std::min(count, h->pending_cap);
    std::vector<PendingRec> recs((size_t)take);
    HIP_TRY(hipMemcpy(recs.data(), h->d_pending.p, sizeof(PendingRec) * (size_t)take, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(h->d_pending_count.p, 0, 4));
    // "the last chunk" (ctag_get_counters, the parity probes) stays the caller's chunk, not the one-frame passes below (round-4 ADVICE)
    const Workspace* const keep_ws = h->last_ws;
    const ctag_frame_result* const keep_out = h->last_out;
    const int keep_frames = h->last_chunk_frames;
    int rc = CTAG_OK;
    for (const PendingRec& r : recs) {
        rc = rerun_frame(h, Call{r.src, 1, r.rows, r.cols, r.ch, (ptrdiff_t)r.row_stride, 0, r.tw, r.subpix, r.dist}, r.out);
        if (rc != CTAG_OK) break;
    }
    h->last_ws = keep_ws;
    h->last_out = keep_out;
    h->last_chunk_frames = keep_frames;
    if (rc != CTAG_OK) return rc;
    if (wait_chain(h) != CTAG_OK) return CTAG_ERR_HIP;
    if (count > h->pending_cap) {  // more than the list holds between two synchronisation points: k_markers gave the surplus the terminal status CTAG_ERR_LIMIT
        std::snprintf(h->last_error, sizeof(h->last_error), "%d frames waited for the any-frame pass, the list holds %d: the surplus carries CTAG_ERR_LIMIT; synchronise more often",
                      count, h->pending_cap);
        return CTAG_ERR_LIMIT;
    }
    return CTAG_OK;
}
namespace ctag {
int handle_finish_pending(ctag_handle* h) { return h ? finish_pending(h) : CTAG_ERR_ARG; }
bool handle_pending_state(ctag_handle* h, const int32_t** count_dev, uint64_t* gen) {
    *count_dev = h->d_pending_count.p;
    *gen = h->pending_gen;
    return h->pending_dirty && h->d_pending_count.p != nullptr;
}
void handle_pending_clean(ctag_handle* h, uint64_t gen) {
    if (h->pending_gen == gen) h->pending_dirty = false;
}
}  // namespace ctag

// host-memory calls: the records are on the host already; a CTAG_PENDING one is completed from the caller's own frame
static int rerun_host_frames(ctag_handle* h, const Call& c, ctag_frame_result* out) {
    for (int i = 0; i < c.n; i++) {
        if (out[i].status != CTAG_PENDING) continue;
        const ptrdiff_t rowbytes = (ptrdiff_t)c.cols * c.channels, dstride = (rowbytes + 15) & ~(ptrdiff_t)15;
        HIP_TRY(h->d_big_frame.grow((size_t)dstride * c.rows));
        HIP_TRY(h->d_big_result.grow(1));
        HIP_TRY(hipMemcpy2DAsync(h->d_big_frame.p, dstride, c.frames + (ptrdiff_t)i * c.frame_stride, c.row_stride, (size_t)rowbytes, c.rows, hipMemcpyHostToDevice,
                                 h->stream));
        Call one = c.sub(i, 1);
        one.frames = h->d_big_frame.p, one.row_stride = dstride, one.frame_stride = 0;
        const int r = rerun_frame(h, one, h->d_big_result.p);
        if (r != CTAG_OK) return r;
        HIP_TRY(hipMemcpyAsync(out + i, h->d_big_result.p, sizeof(ctag_frame_result), hipMemcpyDeviceToHost, h->stream));
        if (wait_chain(h) != CTAG_OK) return CTAG_ERR_HIP;
    }
    return CTAG_OK;
}

// n BGR frames in device memory -> gray (chunk by chunk, on the handle's stream) -> the detection chain
static int detect_bgr_device_impl(ctag_handle* h, const Call& c, ctag_frame_result* out_dev) {
    const int rc = check_args(h, c);
    if (rc != CTAG_OK) return rc;
    if (c.n == 0) return CTAG_OK;
    HIP_TRY(hipSetDevice(h->device));
    // The direct form (round 5): frames of a size the fused sweep takes (half size a multiple of 320 x 5; adaptiveThresh 5), rows and frames 16-byte aligned -- the
    // decimation kernel loads the BGR bytes themselves and converts as it consumes them, edgeRefine converts the boxes it stages: no gray image is
    // written or read back (8.3 of the 24 MB a 1080p frame moved through the gray slab).  CTAG_OPT_BGR_DIRECT 0 turns it off.
    // Calls of a few frames (round 6): the fused sweep's K1 is one block per frame band group -- 0.19 ms for a single 1080p frame against < 0.02 ms
    // of the short-band kernels -- so they convert first and take the gray chain, as gray calls of that size do (plan_chunk).
    if (plan_chunk(PlanIn{c.rows, c.cols, c.adaptive_thresh, c.n, 3, c.corner_subpix, c.frames, c.frame_stride, c.row_stride, h->kp, h->fuse_mode, h->wave_points,
                          h->bgr_direct != 0, dev_knobs()}).bgr_direct) {
        const int r = detect_device_impl(h, c, out_dev, &c);
        h->last_was_bgr = false;  // no gray image to probe
        return r;
    }
    const int chunk = std::min(c.n, h->max_chunk);
    const int gr = ensure_gray(h, chunk, c.rows, c.cols);
    if (gr != CTAG_OK) return gr;
    for (int f0 = 0; f0 < c.n; f0 += chunk) {
        const Call bgr = c.sub(f0, std::min(chunk, c.n - f0));
        int r = enqueue_bgr2gray(h, bgr);
        if (r != CTAG_OK) return r;
        r = detect_device_impl(h, as_gray(bgr, h->d_gray.p, h->gray_row_stride, h->gray_frame_stride), out_dev + f0, &bgr);
        if (r != CTAG_OK) return r;
    }
    h->last_was_bgr = true;
    return CTAG_OK;
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
extern "C" {

int ctag_version(void) { return 120; }  // 120: the drawAxis overlay (include/ctag_pose.h); 110: ctag_params carries struct_size; CTAG_PENDING; test scaffolding left the product ABI (was 100)

const char* ctag_strerror(int status) {
    switch (status) {
        case CTAG_OK: return "ok";
        case CTAG_NO_CORNER: return "No corner detected!";
        case CTAG_NO_FEATURE: return "No feature detected!";
        case CTAG_ERR_ARG: return "invalid argument";
        case CTAG_ERR_HIP: return "HIP runtime error (no usable gfx950 device?)";
        case CTAG_ERR_LIMIT: return "frame exceeds a fixed-array limit of the reference";
        case CTAG_PENDING: return "frame waits for the any-frame pass (ctag_sync completes it)";
        case CTAG_ERR_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown status";
    }
}
const char* ctag_stage_name(int stage) { return (stage >= 0 && stage < CTAG_NUM_STAGES) ? kStageNames[stage] : ""; }

void ctag_params_default(ctag_params* p) {  // header/corner_detector.h:90,110,122,135-137,144; corner_detector.cpp:71,88,285
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->threshold_line = 1.8f;
    p->threshold_expand = 1.2f;
    p->threshold_RAC = 0.3f;
    p->threshold_angle = 5.f;
    p->threshold_vertical = 0.5f;
    const float id[4] = {1.47f, 1.54f, 1.61f, 1.68f}, lo[4] = {0.1f, 0.035f, 0.035f, 0.035f}, hi[4] = {0.035f, 0.035f, 0.035f, 0.1f};
    for (int j = 0; j < 4; j++) {
        p->ID_cr_correspond[j] = id[j];
        p->cr_covariance_left[j] = lo[j];
        p->cr_covariance_right[j] = hi[j];
    }
    p->dark_cap = 0.3f;
    p->area_min = 30;
    p->area_max_fraction = 0.01;
    p->collinear_cost = 1.05;
}

// ctag_params -> KParams (everything but the device table).  The collinearity test compares cost = (float)sqrt((double)c2), c2 the
// squared integer norm of P0 + P2 - 2 P1, with a double threshold (corner_detector.cpp:285-288 `cost > 1.05`, :337 `cost < 1.05`):
// as bounds on c2, found by stepping from the threshold's square.
static bool derive_kparams(const ctag_params& p, KParams* k) {
    auto ok = [](double v) { return v > 0 && v < 1e30; };
    if (!ok(p.threshold_line) || !ok(p.threshold_expand) || !ok(p.threshold_RAC) || !ok(p.threshold_angle) || !ok(p.threshold_vertical) || p.area_min < 1 ||
        !(p.area_max_fraction > 0 && p.area_max_fraction <= 1) || !(p.collinear_cost > 0 && p.collinear_cost < 1e4))
        return false;
    for (int j = 0; j < 4; j++)
        if (!ok(p.ID_cr_correspond[j]) || !(p.cr_covariance_left[j] >= 0) || !(p.cr_covariance_right[j] >= 0)) return false;
    k->thr_line = p.threshold_line;
    k->thr_expand = p.threshold_expand;
    k->expand_eps = 3.0e-6f;
    k->rac = p.threshold_RAC;
    k->angle = p.threshold_angle;
    k->vertical = p.threshold_vertical;
    for (int j = 0; j < 4; j++) {
        k->cr_id[j] = p.ID_cr_correspond[j];
        k->cr_lo[j] = p.cr_covariance_left[j];
        k->cr_hi[j] = p.cr_covariance_right[j];
    }
    k->dark_cap = p.dark_cap;
    k->area_min = p.area_min;
    k->area_max_fraction = p.area_max_fraction;
    auto cost = [](long long c2) { return (double)(float)std::sqrt((double)c2); };
    long long c = (long long)(p.collinear_cost * p.collinear_cost);
    while (c > 0 && cost(c) > p.collinear_cost) c--;       // largest c2 with cost <= threshold ...
    while (!(cost(c + 1) > p.collinear_cost)) c++;
    k->c2_far = (int)(c + 1);                                // ... so cost > threshold from c + 1 on
    long long d = c;
    while (d >= 0 && !(cost(d) < p.collinear_cost)) d--;     // largest c2 with cost < threshold (-1: none)
    k->c2_near = (int)d;
    return true;
}

int ctag_create(const int32_t* state, int dict_rows, int dict_cols, int feature_size, int device_id, ctag_handle** out) {
    return ctag_create_ex(state, dict_rows, dict_cols, feature_size, device_id, nullptr, out);
}

int ctag_create_ex(const int32_t* state, int dict_rows, int dict_cols, int feature_size, int device_id, const ctag_params* params, ctag_handle** out) {
    if (!out) return CTAG_ERR_ARG;
    *out = nullptr;
    ctag_params prm;
    ctag_params_default(&prm);
    if (params) {
        if (params->struct_size != sizeof(ctag_params)) return CTAG_ERR_ARG;  // built against another version of include/ctag_types.h
        prm = *params;
    }
    KParams kp{};
    if (!derive_kparams(prm, &kp)) return CTAG_ERR_ARG;
    std::vector<uint8_t> thr(256 * 256);
    if (!build_threshold_table(prm.dark_cap, thr.data(), &kp.thr_dim, &kp.tcap)) return CTAG_ERR_ARG;
    kp.tcap4 = (uint32_t)kp.tcap * 0x01010101u;
    if (!state || dict_rows < 1 || dict_cols < 1 || (long)dict_rows * dict_cols > kMaxDictCells) return CTAG_ERR_ARG;
    for (long i = 0; i < (long)dict_rows * dict_cols; i++)
        if (!(state[i] >= 0 && state[i] <= 63)) return CTAG_ERR_ARG;  // check_dictionary, CylinderTag.cpp:56-65
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return CTAG_ERR_HIP;
    ctag_handle* h = new (std::nothrow) ctag_handle();
    if (!h) return CTAG_ERR_HIP;
    h->device = device_id;
    h->params = prm;
    h->dict.assign(state, state + (size_t)dict_rows * dict_cols);
    h->dict_rows = dict_rows;
    h->dict_cols = dict_cols;
    h->feature_size = feature_size;
    bool ok = hipSetDevice(device_id) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < ctag_handle::kMaxStreams - 1; k++) {
        ok = ok && hipStreamCreateWithFlags(&h->streamx[k], hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&h->ev_joinx[k], hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&h->ev_fork2, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) == hipSuccess;
    ok = ok && h->d_dict.grow(h->dict.size()) == hipSuccess;
    ok = ok && hipMemcpy(h->d_dict.p, h->dict.data(), h->dict.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && dict_cols <= 32) {
        std::vector<uint32_t> pos((size_t)dict_rows * 64, 0u);
        for (int i = 0; i < dict_rows; i++)
            for (int c = 0; c < dict_cols; c++) pos[(size_t)i * 64 + (state[(size_t)i * dict_cols + c] & 63)] |= 1u << c;
        ok = h->d_dict_pos.grow(pos.size()) == hipSuccess && hipMemcpy(h->d_dict_pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        // fitLine2D's initial samples: cv::RNG is seeded the same way for every fit, so the ten points a restart starts from depend on the edge's
        // point count alone -- tabulated for every count below kPickN2 (bytes below kPickN, halfwords above, one allocation)
        const size_t nb = (size_t)kPickN * 200, nh = (size_t)(kPickN2 - kPickN) * 200;
        std::vector<uint8_t> tab(nb);
        std::vector<uint16_t> tab16(nh);
        build_pick_table(tab.data(), tab16.data());
        ok = h->d_pick_table.grow(nb + nh * 2) == hipSuccess && hipMemcpy(h->d_pick_table.p, tab.data(), nb, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(h->d_pick_table.p + nb, tab16.data(), nh * 2, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        const size_t tb = (size_t)kp.thr_dim * kp.thr_dim;
        ok = h->d_thr_table.grow(tb) == hipSuccess && hipMemcpy(h->d_thr_table.p, thr.data(), tb, hipMemcpyHostToDevice) == hipSuccess;
        kp.thr_table = h->d_thr_table.p;
        h->kp = kp;
    }
    ok = ok && h->d_pending.grow((size_t)h->pending_cap) == hipSuccess;
    ok = ok && h->d_pending_count.grow(64) == hipSuccess && hipMemset(h->d_pending_count.p, 0, 256) == hipSuccess;
    if (!ok) {
        ctag_destroy(h);
        return CTAG_ERR_HIP;
    }
    *out = h;
    return CTAG_OK;
}

// what is not a buffer: the order of things, streams and events (the buffers go with the handle)
void ctag_destroy(ctag_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)quiesce(h);
    drop_graphs(h);
    for (auto& st : h->state)  // pose, draw, rig, gather, multi-view
        if (st.p && st.free_fn) st.free_fn(st.p);
    auto drop = [](hipEvent_t e) {
        if (e) (void)hipEventDestroy(e);
    };
    for (auto& A : h->aslot) drop(A.up), drop(A.done);
    for (hipEvent_t e : h->ev) drop(e);
    for (hipEvent_t e : h->ev_joinx) drop(e);
    for (int i = 0; i < 2; i++) drop(h->ev_copied[i]), drop(h->ev_done[i]);
    drop(h->ev_fork2), drop(h->ev_fork), drop(h->ev_join);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    for (hipStream_t x : h->streamx)
        if (x) (void)hipStreamDestroy(x);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int ctag_load_marker_file(const char* path, int32_t** state, int* dict_rows, int* dict_cols, int* feature_size) {
    if (!path || !state || !dict_rows || !dict_cols || !feature_size) return CTAG_ERR_ARG;
    std::ifstream in(path);
    if (!in.is_open()) return CTAG_ERR_ARG;
    int n = 0, c = 0, fs = 0;
    in >> n >> c >> fs;
    if (!in || n < 1 || c < 1 || (long)n * c > (1L << 24)) return CTAG_ERR_ARG;
    int32_t* s = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (size_t)n * c));
    if (!s) return CTAG_ERR_ARG;
    for (long i = 0; i < (long)n * c; i++) {
        int v = 0;
        in >> v;  // like the reference, a short file leaves the remaining entries at their last parsed value (0)
        s[i] = v;
        if (!(v >= 0 && v <= 63)) {
            std::free(s);
            return CTAG_ERR_ARG;
        }
    }
    *state = s;
    *dict_rows = n;
    *dict_cols = c;
    *feature_size = fs;
    return CTAG_OK;
}
void ctag_free(void* p) { std::free(p); }

int ctag_set_option(ctag_handle* h, int option, int64_t value) {
    if (!h) return CTAG_ERR_ARG;
    switch (option) {
        case CTAG_OPT_MAX_CHUNK:
            if (value < 1 || value > (1 << 20)) return CTAG_ERR_ARG;
            h->max_chunk = (int)value;
            return CTAG_OK;
        case CTAG_OPT_TIMING: h->timing = value != 0; return CTAG_OK;
        case CTAG_OPT_KEEP_PREMARKERS: h->keep_pre = value != 0; return CTAG_OK;
        case CTAG_OPT_GRAPH:
            if (value < 0 || value > 2) return CTAG_ERR_ARG;
            h->use_graph = (int)value;
            if (!h->use_graph) drop_graphs(h);
            return CTAG_OK;
        case CTAG_OPT_WAVE_POINTS:
            if (value < 0 || value > 0x7fffffff) return CTAG_ERR_ARG;
            h->wave_points = (int)value;
            drop_graphs(h);  // a captured chain holds the old value
            return CTAG_OK;
        case CTAG_OPT_EXPAND_EXACT:
            h->kp.expand_eps = value ? INFINITY : 3.0e-6f;
            drop_graphs(h);
            return CTAG_OK;
        case CTAG_OPT_STREAMS:
            if (value < 1 || value > ctag_handle::kMaxStreams) return CTAG_ERR_ARG;
            h->streams = (int)value;
            return CTAG_OK;
        case CTAG_OPT_FUSED_SWEEP:
            if (value < 0 || value > 2) return CTAG_ERR_ARG;
            h->fuse_mode = (int)value;
            drop_graphs(h);
            return CTAG_OK;
        case CTAG_OPT_BGR_DIRECT:
            h->bgr_direct = value != 0;
            drop_graphs(h);
            return CTAG_OK;
        case CTAG_OPT_HOST_SUBCHUNK:
            if (value < 1 || value > (1 << 20)) return CTAG_ERR_ARG;
            h->host_sub = (int)value;
            return CTAG_OK;
        default: return CTAG_ERR_ARG;
    }
}

int ctag_get_timings(ctag_handle* h, float* ms, int capacity) {
    if (!h || !ms) return 0;
    const int n = std::min(capacity, (int)CTAG_NUM_STAGES);
    for (int i = 0; i < n; i++) ms[i] = h->stage_ms[i];
    return n;
}

int ctag_get_counters(ctag_handle* h, ctag_counters* out) {
    if (!h || !out) return CTAG_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    out->reruns = h->reruns;
    if (!h->last_ws || !h->last_ws->base || h->last_chunk_frames <= 0) return CTAG_OK;
    HIP_TRY(hipSetDevice(h->device));
    const int fr = finish_pending(h);
    if (fr != CTAG_OK) return fr;
    out->reruns = h->reruns;
    long long* d = reinterpret_cast<long long*>(h->d_pending_count.p + 16);  // 80 bytes of the 256-byte counter block
    HIP_TRY(launch_counters(h->last_chunk_frames, *h->last_ws, h->last_out, d, h->stream));
    long long v[10];
    HIP_TRY(hipMemcpyAsync(v, d, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    out->frames = h->last_chunk_frames;
    for (int k = 0; k < 5; k++) {
        out->sum[k] = v[k];
        out->max[k] = (int32_t)v[5 + k];
    }
    return CTAG_OK;
}

void* ctag_stream(ctag_handle* h) { return h ? (void*)h->stream : nullptr; }

int ctag_sync(ctag_handle* h) {
    if (!h) return CTAG_ERR_ARG;
    h->last_error[0] = 0;
    const int r = finish_pending(h);  // frames that wait for the any-frame pass (CTAG_PENDING) are completed here
    if (r != CTAG_OK) return r;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return CTAG_OK;
}

int ctag_detect_batch_device(ctag_handle* h, const uint8_t* frames_dev, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                             int adaptive_thresh, int corner_subpix, int subpix_dist, ctag_frame_result* out_dev) {
    if (!h || !out_dev) return CTAG_ERR_ARG;
    begin_timings(h);
    h->last_was_bgr = false;
    const Call c{frames_dev, n, rows, cols, 1, row_stride, frame_stride, adaptive_thresh, corner_subpix, subpix_dist};
    const int r = detect_device_impl(h, c, out_dev, &c);
    if (r != CTAG_OK) {
        h->ev_sets_used = 0;
        return r;
    }
    return collect_timings(h);  // with CTAG_OPT_TIMING the call waits for its last chunk (and completes CTAG_PENDING frames); otherwise it returns at once
}

// the copy stream of the host-memory entry points and its events, created on first use
static int ensure_copy_stream(ctag_handle* h) {
    if (h->copy_stream) return CTAG_OK;
    HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        HIP_TRY(hipEventCreateWithFlags(&h->ev_copied[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_done[i], hipEventDisableTiming));
    }
    return CTAG_OK;
}

// a host-memory call failed with r: uploads / kernels may still be in flight, and nothing may outlive the call (the caller frees its frames)
static int fail_idle(ctag_handle* h, int r) {
    h->ev_sets_used = 0;
    (void)quiesce(h);  // (last_error stays that of the failure)
    return r;
}

static int detect_batch_u8_impl(ctag_handle* h, const Call& c, ctag_frame_result* out) {
    // Frames stream through two device slabs: while slab k is processed on the compute stream, slab k+1 is filled over
    // PCIe on the copy stream (main.cpp:29,36,52-54 feed one frame at a time; this is the batched equivalent).  The
    // copies only overlap when the frames are pinned (ctag_host_alloc / hipHostRegister); pageable memory still works.
    const int n = c.n, rows = c.rows;
    const int sub = std::min(n, std::min(h->max_chunk, h->host_sub));
    // channels = 3: BGR frames (3 bytes per pixel) are uploaded as they are and converted on the device (k_bgr2gray) into the gray slab
    const ptrdiff_t rowbytes = (ptrdiff_t)c.cols * c.channels;
    const ptrdiff_t dstride = (rowbytes + 15) & ~(ptrdiff_t)15;  // packed, 16-byte aligned rows on the device
    if (c.channels == 3) {
        const int gr = ensure_gray(h, sub, rows, c.cols);
        if (gr != CTAG_OK) return gr;
    }
    const size_t dframe = (size_t)dstride * rows;
    if (h->d_frames.cap < dframe * sub * 2) {
        HIP_TRY(quiesce(h));  // (an upload still running on copy_stream must not lose its destination)
        HIP_TRY(h->d_frames.grow(dframe * sub * 2));
    }
    if (h->d_results.cap < (size_t)sub * 2) {
        HIP_TRY(quiesce(h));
        HIP_TRY(h->d_results.grow((size_t)sub * 2));
    }
    const int cs = ensure_copy_stream(h);
    if (cs != CTAG_OK) return cs;
    const bool packed = c.row_stride == rowbytes && dstride == rowbytes && c.frame_stride == (ptrdiff_t)rows * rowbytes;
    const size_t slab_frames = h->d_frames.cap / dframe / 2;
    const int nsub = (n + sub - 1) / sub;
    // the frames [f0, f0 + m) as they lie in a slab
    auto in_slab = [&](uint8_t* slab, int f0, int m) {
        Call d = c.sub(f0, m);
        d.frames = slab, d.row_stride = dstride, d.frame_stride = (ptrdiff_t)dframe;
        return d;
    };
    auto upload = [&](int k) -> int {  // enqueue the upload of sub-chunk k on the copy stream
        const int f0 = k * sub, m = std::min(sub, n - f0), slot = k & 1;
        uint8_t* slab = h->d_frames.p + dframe * slab_frames * slot;
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->ev_done[slot], 0));  // the slab's previous sub-chunk is finished
        if (packed) {
            HIP_TRY(hipMemcpyAsync(slab, c.frames + (ptrdiff_t)f0 * c.frame_stride, dframe * m, hipMemcpyHostToDevice, h->copy_stream));
        } else {
            for (int i = 0; i < m; i++)
                HIP_TRY(hipMemcpy2DAsync(slab + dframe * i, dstride, c.frames + (ptrdiff_t)(f0 + i) * c.frame_stride, c.row_stride, (size_t)rowbytes, rows,
                                         hipMemcpyHostToDevice, h->copy_stream));
        }
        HIP_TRY(hipEventRecord(h->ev_copied[slot], h->copy_stream));
        return CTAG_OK;
    };
    if (n == 1 && c.channels == 1) {
        // One frame (main.cpp:52-59: the reference's loop): everything on the compute stream -- a second stream and its event cost the call more than
        // they could hide -- and the record written by the last kernel straight into pinned host memory instead of fetched by a copy behind it
        HIP_TRY(h->res1.ensure());
        uint8_t* slab = h->d_frames.p;
        if (packed) HIP_TRY(hipMemcpyAsync(slab, c.frames, dframe, hipMemcpyHostToDevice, h->stream));
        else HIP_TRY(hipMemcpy2DAsync(slab, dstride, c.frames, c.row_stride, (size_t)rowbytes, rows, hipMemcpyHostToDevice, h->stream));
        const int r1 = detect_device_impl(h, in_slab(slab, 0, 1), h->res1.dev, nullptr);
        if (r1 != CTAG_OK) return r1;
        HIP_TRY(hipStreamSynchronize(h->stream));
        std::memcpy(out, h->res1.host, sizeof(ctag_frame_result));
        return rerun_host_frames(h, c, out);
    }
    int r = upload(0);
    if (r != CTAG_OK) return r;
    for (int k = 0; k < nsub; k++) {
        const int f0 = k * sub, m = std::min(sub, n - f0), slot = k & 1;
        const Call slab = in_slab(h->d_frames.p + dframe * slab_frames * slot, f0, m);
        ctag_frame_result* res = h->d_results.p + (h->d_results.cap / 2) * slot;
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_copied[slot], 0));
        if (c.channels == 3) {
            r = enqueue_bgr2gray(h, slab);
            if (r != CTAG_OK) return r;
            r = detect_device_impl(h, as_gray(slab, h->d_gray.p, h->gray_row_stride, h->gray_frame_stride), res, nullptr);
        } else {
            r = detect_device_impl(h, slab, res, nullptr);
        }
        if (r != CTAG_OK) return r;
        HIP_TRY(hipEventRecord(h->ev_done[slot], h->stream));
        // the next upload is enqueued before the result download: a download into pageable memory blocks the host
        if (k + 1 < nsub && (r = upload(k + 1)) != CTAG_OK) return r;
        HIP_TRY(hipMemcpyAsync(out + f0, res, sizeof(ctag_frame_result) * m, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    // a frame that exceeded a pool of the batch workspace came back CTAG_PENDING: complete it through the any-frame workspace
    return rerun_host_frames(h, c, out);
}

// the host-memory batch entry points: gray (channels 1) and BGR (3)
static int detect_batch_host(ctag_handle* h, const Call& c, ctag_frame_result* out) {
    if (!h || !out) return CTAG_ERR_ARG;
    const int rc = check_args(h, c);
    if (rc != CTAG_OK) return rc;
    if (c.n == 0) return CTAG_OK;
    HIP_TRY(hipSetDevice(h->device));
    begin_timings(h);
    if (c.channels == 1) h->last_was_bgr = false;
    const int r = detect_batch_u8_impl(h, c, out);
    if (r != CTAG_OK) return fail_idle(h, r);
    if (c.channels == 3) h->last_was_bgr = true;
    return collect_timings(h);
}

int ctag_detect_batch_u8(ctag_handle* h, const uint8_t* frames, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                         int adaptive_thresh, int corner_subpix, int subpix_dist, ctag_frame_result* out) {
    return detect_batch_host(h, Call{frames, n, rows, cols, 1, row_stride, frame_stride, adaptive_thresh, corner_subpix, subpix_dist}, out);
}

// ---- one frame per call, not waited for (include/ctag.h) ----------------------------------------------------------------------------
int ctag_submit_u8(ctag_handle* h, const uint8_t* gray, int rows, int cols, ptrdiff_t row_stride, int adaptive_thresh, int corner_subpix, int subpix_dist) {
    if (!h) return CTAG_ERR_ARG;
    h->last_error[0] = 0;
    const Call c{gray, 1, rows, cols, 1, row_stride, 0, adaptive_thresh, corner_subpix, subpix_dist};
    const int rc = check_args(h, c);
    if (rc != CTAG_OK) return rc;
    if (h->a_count >= ctag_handle::kAsyncDepth) return CTAG_ERR_ARG;  // collect first
    HIP_TRY(hipSetDevice(h->device));
    ctag_handle::AsyncSlot& A = h->aslot[(h->a_head + h->a_count) % ctag_handle::kAsyncDepth];
    const ptrdiff_t dstride = ((ptrdiff_t)cols + 15) & ~(ptrdiff_t)15;
    const size_t need = (size_t)dstride * rows;
    const int cs = ensure_copy_stream(h);
    if (cs != CTAG_OK) return cs;
    if (!A.up) {
        HIP_TRY(hipEventCreateWithFlags(&A.up, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&A.done, hipEventDisableTiming));
        HIP_TRY(A.res.ensure());
    }
    if (A.d_frame.cap < need) {  // the slot is free: nothing reads its slab
        drop_graphs(h);          // ... but a captured chain may hold its address
        HIP_TRY(A.d_frame.grow(need));
    }
    A.host = c;
    // the upload runs on the copy stream while the previous frame's kernels run on the compute stream (the slab's previous reader finished before its
    // ctag_collect returned); the detection waits for it; the record comes back into pinned memory behind the detection
    HIP_TRY(hipMemcpy2DAsync(A.d_frame.p, dstride, gray, row_stride, (size_t)cols, rows, hipMemcpyHostToDevice, h->copy_stream));
    HIP_TRY(hipEventRecord(A.up, h->copy_stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, A.up, 0));
    h->last_was_bgr = false;
    begin_timings(h);
    const int r = detect_device_impl(h, as_gray(c, A.d_frame.p, dstride, (ptrdiff_t)need), A.res.dev, nullptr);
    h->ev_sets_used = 0;
    if (r != CTAG_OK) return fail_idle(h, r);
    HIP_TRY(hipEventRecord(A.done, h->stream));
    h->a_count++;
    return CTAG_OK;
}

int ctag_collect(ctag_handle* h, ctag_frame_result* out) {
    if (!h || !out) return CTAG_ERR_ARG;
    h->last_error[0] = 0;
    if (h->a_count <= 0) return CTAG_ERR_ARG;  // nothing in flight
    HIP_TRY(hipSetDevice(h->device));
    ctag_handle::AsyncSlot& A = h->aslot[h->a_head];
    HIP_TRY(hipEventSynchronize(A.done));
    h->a_head = (h->a_head + 1) % ctag_handle::kAsyncDepth;
    h->a_count--;
    *out = *A.res.host;
    if (out->status == CTAG_PENDING) {  // needs the any-frame workspace: from the caller's frame, like every host-memory call
        const int r = rerun_host_frames(h, A.host, out);
        if (r != CTAG_OK) return r;
    }
    return out->status;
}

void* ctag_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void ctag_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int ctag_detect_u8(ctag_handle* h, const uint8_t* gray, int rows, int cols, ptrdiff_t row_stride, int adaptive_thresh, int corner_subpix,
                   int subpix_dist, ctag_frame_result* out) {
    if (!h || !out) return CTAG_ERR_ARG;
    const int r = ctag_detect_batch_u8(h, gray, 1, rows, cols, row_stride, (ptrdiff_t)row_stride * rows, adaptive_thresh, corner_subpix, subpix_dist, out);
    if (r != CTAG_OK) return r;
    return out->status;
}

int ctag_detect_batch_bgr8_device(ctag_handle* h, const uint8_t* bgr_dev, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                  int adaptive_thresh, int corner_subpix, int subpix_dist, ctag_frame_result* out_dev) {
    if (!h || !out_dev) return CTAG_ERR_ARG;
    begin_timings(h);
    const int r = detect_bgr_device_impl(h, Call{bgr_dev, n, rows, cols, 3, row_stride, frame_stride, adaptive_thresh, corner_subpix, subpix_dist}, out_dev);
    if (r != CTAG_OK) {
        h->ev_sets_used = 0;
        return r;
    }
    return collect_timings(h);
}

int ctag_detect_batch_bgr8(ctag_handle* h, const uint8_t* bgr, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride, int adaptive_thresh,
                           int corner_subpix, int subpix_dist, ctag_frame_result* out) {
    return detect_batch_host(h, Call{bgr, n, rows, cols, 3, row_stride, frame_stride, adaptive_thresh, corner_subpix, subpix_dist}, out);
}

int ctag_detect_bgr8(ctag_handle* h, const uint8_t* bgr, int rows, int cols, ptrdiff_t row_stride, int adaptive_thresh, int corner_subpix, int subpix_dist,
                     ctag_frame_result* out) {
    if (!h || !out) return CTAG_ERR_ARG;
    const int r = ctag_detect_batch_bgr8(h, bgr, 1, rows, cols, row_stride, (ptrdiff_t)row_stride * rows, adaptive_thresh, corner_subpix, subpix_dist, out);
    if (r != CTAG_OK) return r;
    return out->status;
}

}  // extern "C"
