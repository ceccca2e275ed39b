// ctag_testkit.hip -- implementation of include/ctag_testkit.h (libctag_testkit.so): test and bench scaffolding that lives
// OUTSIDE the product library.  Links against libctag_hip.so; reaches into a handle only through ctag::handle_view and
// ctag::gather_unpack_gathered (cylindertag_amd/csrc/ctag_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../include/ctag_testkit.h"
#include "../cylindertag_amd/csrc/ctag_internal.h"
#include "../cylindertag_amd/csrc/ctag_math.h"
#include "../cylindertag_amd/csrc/ctag_wave.h"
#include "ctag_synth.h"

using namespace ctag;

#define TK_TRY(expr)                              \
    do {                                          \
        if ((expr) != hipSuccess) return CTAG_ERR_HIP; \
    } while (0)

namespace {

__global__ void k_math_probe(int op, int n, const double* a, const double* b, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b[i];
    double r = 0;
    switch (op) {
        case 0: r = ctm::atan2_64(x, y); break;
        case 1: r = ctm::sin64(x); break;
        case 2: r = ctm::cos64(x); break;
        case 3: r = ctm::exp64(x); break;
        case 4: r = ctm::acos64(x); break;
        case 5: r = ctm::atan2_32((float)x, (float)y); break;
        case 6: r = ctm::sin32((float)x); break;
        case 7: r = ctm::cos32((float)x); break;
        case 8: r = ctm::exp32((float)x); break;
        case 9: r = ctm::fast_atan2_deg((float)x, (float)y); break;
        case 10: r = x / y; break;
        case 11: r = ctm::sqrt64(x); break;
        case 12: r = (float)x / (float)y; break;
        case 13: r = ctm::sqrt32((float)x); break;
        case 14: r = ctm::round32((float)x); break;
        case 15: r = ctm::exp32_nonpos((float)x); break;  // x <= 0, not NaN
        case 16: r = ctm::div64(x, ctm::recip64(y)); break;  // x / y through the shared-reciprocal form (device) or `/` (host)
        case 17: r = ctm::exp32_nonpos_k0((float)x); break;  // x <= 0 with ctm::exp32_k_is_zero(x)
        case 18: r = ctm::log64(x); break;
        default: break;
    }
    out[i] = r;
}

// One primitive of ctag_wave.h per launch, one wave per 64 consecutive threads.  Every lane first writes the sentinel; the lanes of the wave's `active` mask
// then call the primitive inside the branch, so the other lanes are off in EXEC where it runs.  `op` is uniform: the switch is a scalar branch.
__global__ void k_wave_probe(int op, const unsigned long long* active, const double* a, const long long* ia, double* out, long long* iout) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = CTAG_WAVE_SENTINEL_F64;
    iout[i] = CTAG_WAVE_SENTINEL_I64;
    const double x = a[i];
    const long long w = ia[i];
    const int w32 = (int)(unsigned)((unsigned long long)w & 0xffffffffull);
    const uint32_t whi = (uint32_t)((unsigned long long)w >> 32);
    if (!((active[i >> 6] >> (i & 63)) & 1ull)) return;
    double r = 0.0;
    long long ir = 0;
    auto u32 = [](int v) { return (long long)(unsigned long long)(uint32_t)v; };
    auto nearest = [](float od, int oi, float d, int k) { return od < d || (od == d && oi < k); };   // k_quad.hip: the nearest, ties: the first
    auto farthest = [](float od, int oi, float d, int k) { return od > d || (od == d && oi > k); };  // k_quad.hip: the farthest, ties: the last
    switch (op) {
        case CTAG_WAVE_FROM_PREV: ir = (long long)wave_from_prev((uint32_t)w32); break;
        case CTAG_WAVE_FROM_NEXT: ir = (long long)wave_from_next((uint32_t)w32); break;
        case CTAG_WAVE_SHR1_I32: ir = u32(dpp_shr<1>(w32)); break;
        case CTAG_WAVE_SHR2_I32: ir = u32(dpp_shr<2>(w32)); break;
        case CTAG_WAVE_SHR4_I32: ir = u32(dpp_shr<4>(w32)); break;
        case CTAG_WAVE_SHR1_F32: ir = u32(__float_as_int(dpp_shr<1>(__int_as_float(w32)))); break;
        case CTAG_WAVE_SHR1_F64: r = dpp_shr<1>(x); break;
        case CTAG_WAVE_XOR1_I32: ir = u32(dpp_mov<kDppXor1>(w32)); break;
        case CTAG_WAVE_XOR2_I32: ir = u32(dpp_mov<kDppXor2>(w32)); break;
        case CTAG_WAVE_HALF_MIRROR_I32: ir = u32(dpp_mov<kDppHalfMirror>(w32)); break;
        case CTAG_WAVE_ROW_MIRROR_I32: ir = u32(dpp_mov<kDppRowMirror>(w32)); break;
        case CTAG_WAVE_XOR1_I64: ir = dpp_mov<kDppXor1>(w); break;
        case CTAG_WAVE_XOR2_I64: ir = dpp_mov<kDppXor2>(w); break;
        case CTAG_WAVE_HALF_MIRROR_I64: ir = dpp_mov<kDppHalfMirror>(w); break;
        case CTAG_WAVE_ROW_MIRROR_I64: ir = dpp_mov<kDppRowMirror>(w); break;
        case CTAG_WAVE_INCL_SCAN: ir = u32(wave_incl_scan(w32)); break;
        case CTAG_WAVE_SG_SUM8_I32: ir = u32(sg_sum<8>(w32)); break;
        case CTAG_WAVE_SG_SUM64_I32: ir = u32(sg_sum<64>(w32)); break;
        case CTAG_WAVE_SG_SUM8_I64: ir = sg_sum<8>(w); break;
        case CTAG_WAVE_SG_SUM64_I64: ir = sg_sum<64>(w); break;
        case CTAG_WAVE_SG_BEST8_NEAREST:
        case CTAG_WAVE_SG_BEST8_FARTHEST:
        case CTAG_WAVE_SG_BEST64_NEAREST:
        case CTAG_WAVE_SG_BEST64_FARTHEST: {
            float bd = (float)x;  // -0, +-inf and every float-valued double pass unchanged
            int bi = w32;
            if (op == CTAG_WAVE_SG_BEST8_NEAREST) sg_best<8>(bd, bi, nearest);
            else if (op == CTAG_WAVE_SG_BEST8_FARTHEST) sg_best<8>(bd, bi, farthest);
            else if (op == CTAG_WAVE_SG_BEST64_NEAREST) sg_best<64>(bd, bi, nearest);
            else sg_best<64>(bd, bi, farthest);
            r = (double)bd;
            ir = (long long)bi;
            break;
        }
        case CTAG_WAVE_SUM_F64: r = wave_sum_f64(x); break;
        case CTAG_WAVE_MAX_F64: {
            double bd = x;
            int bi = w32;
            wave_max_f64(bd, bi);
            r = bd;
            ir = (long long)bi;
            break;
        }
        case CTAG_WAVE_ALL: ir = wave_all(w != 0) ? 1 : 0; break;
        case CTAG_WAVE_PK_MIN_U16: ir = (long long)pk_min_u16((uint32_t)w32, whi); break;
        case CTAG_WAVE_PK_MAX_U16: ir = (long long)pk_max_u16((uint32_t)w32, whi); break;
        default: break;
    }
    out[i] = r;
    iout[i] = ir;
}

__global__ void k_label_roots(const uint16_t* labels, const int32_t* tile_base, const int32_t* root_of, int32_t* out, FrameGeom g) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= g.hcols || y >= g.hrows) return;
    const unsigned l = labels[(size_t)y * g.lp + x];
    int v = 0;
    const int tile = (y / kTileH) * g.tiles_x + (x / kTileW);
    if (l & 0x8000u) v = -(1 + tile * 32768 + (int)(l & 0x7fffu));  // an unpublished speck of the second CCL pass: a private negative id
    else if (l) v = 1 + root_of[tile_base[tile] + (int)l - 1];
    out[(size_t)y * g.hcols + x] = v;
}

__global__ __launch_bounds__(256) void k_synth(const ctag_synth::Frame* frames, uint8_t* out, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride) {
    __shared__ ctag_synth::Frame F;
    const int f = blockIdx.z;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(frames + f);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&F);
        for (int i = threadIdx.x; i < (int)(sizeof(ctag_synth::Frame) / 4); i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    out[(ptrdiff_t)f * frame_stride + (ptrdiff_t)y * row_stride + x] = ctag_synth::pixel(F, x, y, rows, cols);
}

// renders frames [first_frame, first_frame + n) of a synthetic scene into device memory; layouts are computed on the host
int synth_frames_device(ctag_handle* h, uint8_t* frames_dev, int first_frame, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                        uint64_t seed, int markers_per_frame, bool scene3d, double fx, double fy, double cx, double cy) {
    if (!h || !frames_dev || n < 0 || rows < 1 || cols < 1 || row_stride < cols) return CTAG_ERR_ARG;
    if (n == 0) return CTAG_OK;
    HandleView v{};
    handle_view(h, &v);
    TK_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const int step = 512;
    ctag_synth::Frame* d_lay = nullptr;
    TK_TRY(hipMalloc(reinterpret_cast<void**>(&d_lay), sizeof(ctag_synth::Frame) * step));
    std::vector<ctag_synth::Frame> lay(step);
    int rc = CTAG_OK;
    for (int f0 = 0; f0 < n && rc == CTAG_OK; f0 += step) {
        const int m = std::min(step, n - f0);
        for (int i = 0; i < m; i++) {
            if (scene3d)
                ctag_synth::layout3d(v.dict, v.dict_rows, v.dict_cols, seed, first_frame + f0 + i, rows, cols, markers_per_frame, fx, fy, cx, cy, &lay[i], nullptr);
            else
                ctag_synth::layout(v.dict, v.dict_rows, v.dict_cols, seed, first_frame + f0 + i, rows, cols, markers_per_frame, &lay[i], nullptr);
        }
        if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(d_lay, lay.data(), sizeof(ctag_synth::Frame) * m, hipMemcpyHostToDevice) != hipSuccess) {
            rc = CTAG_ERR_HIP;
            break;
        }
        hipLaunchKernelGGL(k_synth, dim3((cols + 255) / 256, rows, m), dim3(256), 0, s, d_lay, frames_dev + (ptrdiff_t)f0 * frame_stride, rows, cols, row_stride,
                           frame_stride);
        if (hipGetLastError() != hipSuccess) rc = CTAG_ERR_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess) rc = CTAG_ERR_HIP;
    (void)hipFree(d_lay);
    return rc;
}

void fill_truth(const ctag_synth::Truth& T, ctag_synth_truth* truth) {
    std::memset(truth, 0, sizeof(*truth));
    truth->n_markers = T.n;
    for (int k = 0; k < T.n && k < 8; k++) {
        truth->dict_row[k] = T.dict_row[k];
        truth->strip_len[k] = T.strip_len[k];
        for (int q = 0; q < 8; q++) truth->corners[k][q] = T.corners[k][q];
    }
}


// ---- edge search of the dense pose-refinement study (include/ctag_testkit.h) --------------------------------------
constexpr int kDenseMaxTaps = 33;  // search_px <= 8 in 0.5-px steps

struct DenseProbeCam {
    double fx, fy, cx, cy;
    double k[14];
};

// cv::projectPoints without tilt, double
__device__ void dense_project(const double* R, const double* t, const DenseProbeCam& c, const double* X, double* u) {
    const double P0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    const double P1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double P2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    if (!(P2 > 0.0)) {
        u[0] = u[1] = __builtin_nan("");
        return;
    }
    const double x = P0 / P2, y = P1 / P2;
    const double* k = c.k;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r2 * r2 * r2;
    const double cd = (1 + k[0] * r2 + k[1] * r4 + k[4] * r6) / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
    const double xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r4;
    const double yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r4;
    u[0] = c.fx * xd + c.cx;
    u[1] = c.fy * yd + c.cy;
}

// one wave; lane = sample (segment-major)
__global__ __launch_bounds__(64) void k_dense_edge_probe(const uint8_t* __restrict__ img, int rows, int cols, ptrdiff_t row_stride,
                                                         const double* __restrict__ seg, int n_seg, DenseProbeCam cam, double R0, double R1,
                                                         double R2, double T0, double T1, double T2, int S, int nt, double r,
                                                         double min_contrast, double* __restrict__ out, int32_t* __restrict__ keep) {
    // Rodrigues as tests/pose_testlib.py states it: cos(th) I + sin(th) [w]x + (1 - cos(th)) w w^T
    double R[9];
    const double th = __builtin_sqrt(R0 * R0 + R1 * R1 + R2 * R2);
    if (th < 1e-12) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double w[3] = {R0 / th, R1 / th, R2 / th}, c = ctm::cos64(th), s = ctm::sin64(th);
        const double Wx[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        for (int i = 0; i < 9; i++) R[i] = (c * ((i % 4 == 0) ? 1.0 : 0.0) + s * Wx[i]) + (1 - c) * (w[i / 3] * w[i % 3]);
    }
    const double t[3] = {T0, T1, T2};
    const int n = n_seg * S;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int sg = i / S;
        const double ss = ((i % S) + 0.5) / S;
        const double* G = seg + (size_t)sg * 12;
        double d[3], X[3], Xp[3], Xm[3], Q[3];
        for (int j = 0; j < 3; j++) {
            d[j] = G[3 + j] - G[j];
            X[j] = G[j] + ss * d[j];
            Xp[j] = X[j] + d[j] / 64;
            Xm[j] = X[j] - d[j] / 64;
            Q[j] = G[6 + j] + ss * (G[9 + j] - G[6 + j]);
        }
        double P[2], up[2], um[2], q[2];
        dense_project(R, t, cam, X, P);
        dense_project(R, t, cam, Xp, up);
        dense_project(R, t, cam, Xm, um);
        dense_project(R, t, cam, Q, q);
        const double Tx = up[0] - um[0], Ty = up[1] - um[1];
        const double tl = __builtin_sqrt(Tx * Tx + Ty * Ty);
        double nx = -Ty / tl, ny = Tx / tl;
        if ((P[0] - q[0]) * nx + (P[1] - q[1]) * ny < 0) {
            nx = -nx;
            ny = -ny;
        }
        // profile; any tap outside the frame (or not finite) drops the sample
        double prof[kDenseMaxTaps];
        bool inside = true;
        for (int k = 0; k < nt; k++) {
            const double o = -r + 0.5 * k;
            const double x = P[0] + o * nx, y = P[1] + o * ny;
            if (!(x >= 0.0 && y >= 0.0 && x <= cols - 1 && y <= rows - 1)) {
                inside = false;
                prof[k] = 0.0;
                continue;
            }
            const int x0 = min((int)floor(x), cols - 2), y0 = min((int)floor(y), rows - 2);
            const double fx = x - x0, fy = y - y0;
            const uint8_t* p0 = img + (ptrdiff_t)y0 * row_stride + x0;
            const uint8_t* p1 = p0 + row_stride;
            const double top = (1 - fx) * (double)p0[0] + fx * (double)p0[1];
            const double bot = (1 - fx) * (double)p1[0] + fx * (double)p1[1];
            prof[k] = (1 - fy) * top + fy * bot;
        }
        // difference at tap j + 1 is D[j] = (prof[j + 2] - prof[j]) / 2, j = 0 .. nt - 3; first maximum
        const int nd = nt - 2;
        int kb = 0;
        double db = 0.5 * (prof[2] - prof[0]);
        for (int j = 1; j < nd; j++) {
            const double dj = 0.5 * (prof[j + 2] - prof[j]);
            if (dj > db) {
                db = dj;
                kb = j;
            }
        }
        const bool kp = inside && kb > 0 && kb < nd - 1 && db >= min_contrast;
        double off = __builtin_nan("");
        if (kp) {
            const double dm = 0.5 * (prof[kb + 1] - prof[kb - 1]), dp = 0.5 * (prof[kb + 3] - prof[kb + 1]);
            const double den = dm - 2 * db + dp;
            const double delta = den < 0 ? 0.5 * (dm - dp) / den : 0.0;
            off = -r + 0.5 * (kb + 1) + 0.5 * delta;
        }
        double* o = out + (size_t)i * 5;
        o[0] = P[0];
        o[1] = P[1];
        o[2] = nx;
        o[3] = ny;
        o[4] = off;
        keep[i] = kp ? 1 : 0;
    }
}

}  // namespace

extern "C" {

long ctag_debug_fetch(ctag_handle* h, int frame, int what, void* dst, size_t cap) {
    if (!h) return -1;
    HandleView v{};
    handle_view(h, &v);
    if (!v.ws || !v.ws->base || frame < 0 || frame >= v.last_chunk_frames) return -1;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    if (hipSetDevice(v.device) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return -2;
    const Workspace& W = *v.ws;
    const FrameGeom& g = W.g;
    auto d2h = [&](void* d, const void* src, size_t bytes) { return hipMemcpy(d, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    switch (what) {
        case CTAG_DBG_HALF: {
            const size_t n = (size_t)g.hrows * g.hcols;
            if (dst && cap >= n) {
                if (v.fused) {
                    // the fused sweep never writes the half-size image (its place holds the threshold mask): decimate this frame again with
                    // the stand-alone kernel into a scratch image (the fused kernel's own pixels are checked through CTAG_DBG_MASK / labels)
                    if (!v.frames) return -1;
                    Workspace T = W;
                    uint8_t* tmp = nullptr;
                    if (hipMalloc(reinterpret_cast<void**>(&tmp), (size_t)g.hrows * g.hp + 256) != hipSuccess) return -2;
                    T.half = tmp;
                    const uint8_t* src = v.frames + (ptrdiff_t)frame * v.frame_stride;
                    ChunkPlan pl = plan_chunk(PlanIn{g.rows, g.cols, g.tw, 1, 1, 0, src, v.frame_stride, v.row_stride, W.kp, 0, 0, false, dev_knobs()});
                    pl.dec_zero_kernel = pl.dec_zero_list = false;  // T shares the chunk's counters: decimate only
                    bool ok = launch_decimate(pl, src, v.frame_stride, v.row_stride, T, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
                    ok = ok && hipMemcpy2D(dst, g.hcols, tmp, g.hp, g.hcols, g.hrows, hipMemcpyDeviceToHost) == hipSuccess;
                    (void)hipFree(tmp);
                    if (!ok) return -2;
                } else if (hipMemcpy2D(dst, g.hcols, W.half + (size_t)frame * g.hrows * g.hp, g.hp, g.hcols, g.hrows, hipMemcpyDeviceToHost) != hipSuccess) {
                    return -2;
                }
            }
            return (long)n;
        }
        case CTAG_DBG_MASK: {
            if (!v.fused) return -1;
            const size_t n = (size_t)g.hrows * g.hcols;
            if (dst && cap >= n) {
                const size_t mb = (size_t)g.hrows * (g.hcols >> 3);
                std::vector<uint8_t> bits(mb);
                if (!d2h(bits.data(), W.half + (size_t)frame * mb, mb)) return -2;
                uint8_t* o = static_cast<uint8_t*>(dst);
                for (size_t i = 0; i < n; i++) o[i] = (bits[i >> 3] >> (i & 7)) & 1u;
            }
            return (long)n;
        }
        case CTAG_DBG_GRAY: {
            if (!v.gray) return -1;
            const size_t n = (size_t)g.rows * g.cols;
            if (dst && cap >= n) {
                if (hipMemcpy2D(dst, g.cols, v.gray + (size_t)frame * v.gray_frame_stride, v.gray_row_stride, g.cols, g.rows, hipMemcpyDeviceToHost) != hipSuccess)
                    return -2;
            }
            return (long)n;
        }
        case CTAG_DBG_LABELS: {
            const size_t n = (size_t)g.hrows * g.hcols;
            if (dst && cap >= n) {
                int32_t* tmp = nullptr;
                if (hipMalloc(reinterpret_cast<void**>(&tmp), n * 4) != hipSuccess) return -2;
                hipLaunchKernelGGL(k_label_roots, dim3((g.hcols + 255) / 256, g.hrows), dim3(256), 0, s, W.labels + (size_t)frame * g.hrows * g.lp,
                                   W.tile_base + (size_t)frame * g.tiles_x * g.tiles_y, W.root_of + (size_t)frame * g.pool_cap, tmp, g);
                const bool ok = hipStreamSynchronize(s) == hipSuccess && d2h(dst, tmp, n * 4);
                (void)hipFree(tmp);
                if (!ok) return -2;
            }
            return (long)n;
        }
        case CTAG_DBG_CANDIDATES:
        case CTAG_DBG_CAND_QUADS: {
            int nc = 0;
            if (!d2h(&nc, W.ncand + frame, 4)) return -2;
            if (dst && cap >= (size_t)nc * 8 && nc > 0) {
                std::vector<Candidate> c(nc);
                std::vector<QuadOut> q(nc);
                if (!d2h(c.data(), W.cand + (size_t)frame * W.cand_cap, sizeof(Candidate) * nc)) return -2;
                if (!d2h(q.data(), W.quads + (size_t)frame * W.cand_cap, sizeof(QuadOut) * nc)) return -2;
                if (what == CTAG_DBG_CANDIDATES) {
                    int32_t* o = static_cast<int32_t*>(dst);
                    for (int i = 0; i < nc; i++) {
                        o[8 * i + 0] = c[i].area;
                        o[8 * i + 1] = c[i].x_min;
                        o[8 * i + 2] = c[i].y_min;
                        o[8 * i + 3] = c[i].x_max;
                        o[8 * i + 4] = c[i].y_max;
                        o[8 * i + 5] = q[i].valid;
                        o[8 * i + 6] = q[i].n_boundary;
                        o[8 * i + 7] = c[i].root;
                    }
                } else {
                    float* o = static_cast<float*>(dst);
                    for (int i = 0; i < nc; i++)
                        for (int k = 0; k < 8; k++) o[8 * i + k] = q[i].valid ? q[i].c[k] : 0.f;
                }
            }
            return (long)nc * 8;
        }
        case CTAG_DBG_FEATURES0:
        case CTAG_DBG_FEATURES1:
        case CTAG_DBG_FEATURES2: {
            int nf = 0;
            if (!d2h(&nf, W.nfeat + frame, 4)) return -2;
            int fst = 0;
            if (!d2h(&fst, W.status + frame, 4)) return -2;
            if (dst && cap >= (size_t)nf * 19 && nf > 0 && fst != CTAG_OK && what != CTAG_DBG_FEATURES0) {
                // early return ("No feature detected!", fewer features than featureSize): cornerObtain / edgeRefine never ran
                std::memset(dst, 0, (size_t)nf * 19 * sizeof(float));
            } else if (dst && cap >= (size_t)nf * 19 && nf > 0) {
                std::vector<FeatureDev> f(nf);
                const FeatureDev* src = what == CTAG_DBG_FEATURES0 ? W.feat0 : what == CTAG_DBG_FEATURES1 ? W.feat1 : W.feat2;
                if (!d2h(f.data(), src + (size_t)frame * CTAG_MAX_FEATURES, sizeof(FeatureDev) * nf)) return -2;
                float* o = static_cast<float*>(dst);
                for (int i = 0; i < nf; i++) {
                    for (int k = 0; k < 16; k++) o[19 * i + k] = f[i].c[k];
                    o[19 * i + 16] = f[i].center[0];
                    o[19 * i + 17] = f[i].center[1];
                    o[19 * i + 18] = f[i].angle;
                }
            }
            return (long)nf * 19;
        }
        case CTAG_DBG_LINES: {
            int nl = 0;
            if (!d2h(&nl, W.line_count + frame, 4)) return -2;
            nl = std::min(nl, W.line_cap);
            if (dst && cap >= (size_t)nl && nl > 0) {
                std::vector<LineDesc> d(nl);
                if (!d2h(d.data(), W.line_desc + (size_t)frame * W.line_cap, sizeof(LineDesc) * nl)) return -2;
                int32_t* o = static_cast<int32_t*>(dst);
                for (int i = 0; i < nl; i++) o[i] = d[i].n;
            }
            return (long)nl;
        }
        case CTAG_DBG_LINE_POINTS:
        case CTAG_DBG_LINE_FITS: {
            int nl = 0;
            if (!d2h(&nl, W.line_count + frame, 4)) return -2;
            nl = std::min(nl, W.line_cap);
            std::vector<LineDesc> d(std::max(nl, 1));
            if (nl > 0 && !d2h(d.data(), W.line_desc + (size_t)frame * W.line_cap, sizeof(LineDesc) * nl)) return -2;
            if (what == CTAG_DBG_LINE_FITS) {
                if (dst && cap >= (size_t)nl * 4 && nl > 0 && !d2h(dst, W.line_fit + (size_t)frame * W.line_cap * 4, (size_t)nl * 16)) return -2;
                return (long)nl * 4;
            }
            size_t total = 0, extent = 0;
            for (int i = 0; i < nl; i++) {
                if (d[i].n < 0 || (size_t)d[i].off + (size_t)d[i].n > (size_t)W.cl_cap) return -2;
                total += (size_t)d[i].n;
                extent = std::max(extent, (size_t)d[i].off + (size_t)d[i].n);
            }
            if (dst && cap >= total * 2 && total > 0) {
                std::vector<uint32_t> pool(extent);
                if (!d2h(pool.data(), W.cl_pool + (size_t)frame * W.cl_cap, extent * 4)) return -2;
                int32_t* o = static_cast<int32_t*>(dst);
                for (int i = 0; i < nl; i++)
                    for (int j = 0; j < d[i].n; j++) {
                        const uint32_t w = pool[(size_t)d[i].off + j];
                        *o++ = (int32_t)(w & 0xffffu);
                        *o++ = (int32_t)(w >> 16);
                    }
            }
            return (long)(total * 2);
        }
        case CTAG_DBG_PACKS: {
            int32_t hd[5] = {0, 0, 0, 0, 0};  // nc, np1, nbig, np2, nel
            if (!d2h(&hd[0], W.ncand + frame, 4) || !d2h(&hd[1], W.npacks + 2 * frame, 8) || !d2h(&hd[3], W.npacks2 + 2 * frame, 8)) return -2;
            hd[0] = std::min(hd[0], W.cand_cap);
            const size_t nc = (size_t)hd[0], np1 = (size_t)hd[1], np2 = (size_t)hd[3], nel = (size_t)hd[4];
            if (hd[1] < 0 || hd[3] < 0 || hd[4] < 0 || np1 > nc || np2 > nc || nel > nc) return -2;
            const size_t total = 5 + np1 + np2 + nc + nel + nc;
            if (dst && cap >= total) {
                int32_t* o = static_cast<int32_t*>(dst);
                std::memcpy(o, hd, sizeof(hd));
                o += 5;
                const size_t fo = (size_t)frame * W.cand_cap;
                if (np1 && !d2h(o, W.packs + fo, np1 * 4)) return -2;
                o += np1;
                if (np2 && !d2h(o, W.packs2 + fo, np2 * 4)) return -2;
                o += np2;
                if (nc && !d2h(o, W.pack_order + fo, nc * 4)) return -2;
                o += nc;
                if (nel && !d2h(o, W.pack_order2 + fo, nel * 4)) return -2;
                o += nel;
                std::vector<CandAux> a(std::max<size_t>(nc, 1));
                if (nc && !d2h(a.data(), W.cand_aux + fo, nc * sizeof(CandAux))) return -2;
                for (size_t i = 0; i < nc; i++) o[i] = a[i].n_boundary;
            }
            return (long)total;
        }
        case CTAG_DBG_PACKS1: {
            int32_t hd[4] = {0, v.packs1 ? 1 : 0, 0, 0};  // nc, built, np, nel
            if (!d2h(&hd[0], W.ncand + frame, 4)) return -2;
            hd[0] = std::min(hd[0], W.cand_cap);
            if (v.packs1 && !d2h(&hd[2], W.npacks1 + 2 * frame, 8)) return -2;
            const size_t nc = (size_t)hd[0], np = (size_t)hd[2], nel = (size_t)hd[3];
            if (hd[2] < 0 || hd[3] < 0 || np > nc || nel > nc) return -2;
            if (!v.packs1) {  // the last chunk's branch built no such lists: the header says so, nothing follows it
                if (dst && cap >= 4) std::memcpy(dst, hd, sizeof(hd));
                return 4;
            }
            const size_t total = 4 + np + nel + nc;
            if (dst && cap >= total) {
                int32_t* o = static_cast<int32_t*>(dst);
                std::memcpy(o, hd, sizeof(hd));
                o += 4;
                const size_t fo = (size_t)frame * W.cand_cap;
                if (np && !d2h(o, W.packs1 + fo, np * 4)) return -2;
                o += np;
                if (nel && !d2h(o, W.pack_order1 + fo, nel * 4)) return -2;
                std::vector<int32_t> nt(std::max<size_t>(nc, 1));
                if (nc && !d2h(nt.data(), W.ntotal1 + fo, nc * 4)) return -2;
                for (size_t i = 0; i < nc; i++) o[nel + i] = -1;  // (k_prepack writes the packed components' entries only: the rest are whatever an earlier chunk left)
                for (size_t i = 0; i < nel; i++)
                    if (o[i] >= 0 && (size_t)o[i] < nc) o[nel + o[i]] = nt[o[i]];
            }
            return (long)total;
        }
        case CTAG_DBG_PREMARKERS: {
            if (!v.keep_pre) return -1;
            if (dst && cap >= 1) {
                if (!d2h(dst, W.premarkers + frame, sizeof(ctag_frame_result))) return -2;
            }
            return 1;
        }
        default: return -1;
    }
}

int ctag_math_probe(ctag_handle* h, int op, int n, const double* a, const double* b, double* out) {
    if (!h || n < 0 || !a || !out) return CTAG_ERR_ARG;
    if (n == 0) return CTAG_OK;
    HandleView v{};
    handle_view(h, &v);
    TK_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    int rc = CTAG_OK;
    if (hipMalloc(reinterpret_cast<void**>(&da), (size_t)n * 8) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&db), (size_t)n * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dout), (size_t)n * 8) != hipSuccess)
        rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK && hipMemcpy(da, a, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK && (b ? hipMemcpy(db, b, (size_t)n * 8, hipMemcpyHostToDevice) : hipMemset(db, 0, (size_t)n * 8)) != hipSuccess) rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK) {
        hipLaunchKernelGGL(k_math_probe, dim3((n + 255) / 256), dim3(256), 0, s, op, n, da, db, dout);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess)
            rc = CTAG_ERR_HIP;
    }
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return rc;
}

int ctag_testkit_wave_probe(ctag_handle* h, int op, int block_threads, int n_waves, const uint64_t* active, const double* a, const int64_t* ia, double* out,
                            int64_t* iout) {
    if (!h || op < 0 || op >= CTAG_WAVE_OPS || (block_threads != 64 && block_threads != 256) || n_waves < 0 || n_waves > 65536 || !active || !a || !ia || !out ||
        !iout)
        return CTAG_ERR_ARG;
    const bool whole = op == CTAG_WAVE_SG_SUM64_I32 || op == CTAG_WAVE_SG_SUM64_I64 || op == CTAG_WAVE_SG_BEST64_NEAREST || op == CTAG_WAVE_SG_BEST64_FARTHEST ||
                       op == CTAG_WAVE_SUM_F64 || op == CTAG_WAVE_MAX_F64 || op == CTAG_WAVE_INCL_SCAN;
    const bool sub8 = op == CTAG_WAVE_SG_SUM8_I32 || op == CTAG_WAVE_SG_SUM8_I64 || op == CTAG_WAVE_SG_BEST8_NEAREST || op == CTAG_WAVE_SG_BEST8_FARTHEST;
    for (int w = 0; w < n_waves; w++) {
        if (whole && active[w] != ~0ull) return CTAG_ERR_ARG;  // all 64 lanes are the caller's duty: a v_readlane would read a masked-off lane's stale register
        if (sub8)
            for (int g = 0; g < 8; g++) {
                const uint64_t m = (active[w] >> (8 * g)) & 0xffull;
                if (m != 0 && m != 0xffull) return CTAG_ERR_ARG;  // a sub-group is on or off as a whole (ctag_wave.h)
            }
    }
    if (n_waves == 0) return CTAG_OK;
    HandleView v{};
    handle_view(h, &v);
    TK_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const int wpb = block_threads / 64, blocks = (n_waves + wpb - 1) / wpb;
    const size_t nw = (size_t)blocks * wpb, nl = nw * 64, n = (size_t)n_waves * 64;  // whole blocks: the waves past n_waves have no active lane
    unsigned long long* dact = nullptr;
    double *da = nullptr, *dout = nullptr;
    long long *dia = nullptr, *diout = nullptr;
    int rc = CTAG_OK;
    if (hipMalloc(reinterpret_cast<void**>(&dact), nw * 8) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&da), nl * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dia), nl * 8) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&dout), nl * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&diout), nl * 8) != hipSuccess)
        rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK && (hipMemset(dact, 0, nw * 8) != hipSuccess || hipMemset(da, 0, nl * 8) != hipSuccess || hipMemset(dia, 0, nl * 8) != hipSuccess)) rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK && (hipMemcpy(dact, active, (size_t)n_waves * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(dia, ia, n * 8, hipMemcpyHostToDevice) != hipSuccess))
        rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK) {
        hipLaunchKernelGGL(k_wave_probe, dim3(blocks), dim3(block_threads), 0, s, op, dact, da, dia, dout, diout);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(iout, diout, n * 8, hipMemcpyDeviceToHost) != hipSuccess)
            rc = CTAG_ERR_HIP;
    }
    (void)hipFree(dact);
    (void)hipFree(da);
    (void)hipFree(dia);
    (void)hipFree(dout);
    (void)hipFree(diout);
    return rc;
}

int ctag_testkit_exp32_k0_sweep(uint32_t first_bits, uint32_t last_bits, uint32_t step, uint64_t* counts, uint32_t* first_bad) {
    if (!counts || step == 0 || first_bits > last_bits) return CTAG_ERR_ARG;
    uint64_t visited = 0, k0 = 0, bad_pred = 0, bad_bits = 0;
    uint32_t bad_at = 0;
    for (uint64_t u = first_bits; u <= last_bits; u += step) {
        const float x = ctm::bits_to_f32((uint32_t)u);
        if (!(x <= 0.0f)) return CTAG_ERR_ARG;  // positive or NaN: outside exp32_nonpos's domain
        const bool is_zero = ctm::exp32_k_is_zero(x);
        bool bad = is_zero != (__builtin_rintf(x * 1.44269502162933349609375f) == 0.0f);
        bad_pred += bad ? 1 : 0;
        if (is_zero && ctm::f32_to_bits(ctm::exp32_nonpos_k0(x)) != ctm::f32_to_bits(ctm::exp32_nonpos(x))) bad_bits++, bad = true;
        if (bad && bad_pred + bad_bits == 1) bad_at = (uint32_t)u;
        visited++;
        k0 += is_zero ? 1 : 0;
    }
    counts[0] = visited, counts[1] = k0, counts[2] = bad_pred, counts[3] = bad_bits;
    if (first_bad) *first_bad = bad_at;
    return CTAG_OK;
}

int ctag_testkit_unpack_gathered(ctag_handle* h, const void* gathered_dev, int n_total, int world, uint64_t width, ctag_frame_result* out_dev) {
    return gather_unpack_gathered(h, gathered_dev, n_total, world, width, out_dev);
}

__global__ void k_stall(long long ticks) {  // s_memrealtime counts at 100 MHz
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
int ctag_testkit_stall_stream(ctag_handle* h, int milliseconds) {
    if (!h || milliseconds < 0 || milliseconds > 10000) return CTAG_ERR_ARG;
    hipLaunchKernelGGL(k_stall, dim3(1), dim3(1), 0, static_cast<hipStream_t>(ctag_stream(h)), (long long)milliseconds * 100000ll);
    return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

int ctag_synth_frames_device(ctag_handle* h, uint8_t* frames_dev, int first_frame, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                             uint64_t seed, int markers_per_frame) {
    return synth_frames_device(h, frames_dev, first_frame, n, rows, cols, row_stride, frame_stride, seed, markers_per_frame, false, 1, 1, 0, 0);
}

int ctag_synth3d_frames_device(ctag_handle* h, uint8_t* frames_dev, int first_frame, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                               uint64_t seed, int markers_per_frame, double fx, double fy, double cx, double cy) {
    if (!(fx > 0) || !(fy > 0)) return CTAG_ERR_ARG;
    return synth_frames_device(h, frames_dev, first_frame, n, rows, cols, row_stride, frame_stride, seed, markers_per_frame, true, fx, fy, cx, cy);
}

int ctag_synth3d_frame_host(const int32_t* state, int dict_rows, int dict_cols, uint8_t* frame, int frame_index, int rows, int cols, ptrdiff_t row_stride,
                            uint64_t seed, int markers_per_frame, double fx, double fy, double cx, double cy, ctag_synth3d_truth* truth) {
    if (!state || !frame || rows < 1 || cols < 1 || row_stride < cols || dict_rows < 1 || dict_cols < 1 || !(fx > 0) || !(fy > 0)) return CTAG_ERR_ARG;
    ctag_synth::Frame F;
    ctag_synth::Truth3D T;
    ctag_synth::layout3d(state, dict_rows, dict_cols, seed, frame_index, rows, cols, markers_per_frame, fx, fy, cx, cy, &F, &T);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) frame[(ptrdiff_t)y * row_stride + x] = ctag_synth::pixel(F, x, y, rows, cols);
    if (truth) {
        std::memset(truth, 0, sizeof(*truth));
        truth->n_markers = T.n;
        for (int k = 0; k < T.n && k < 8; k++) {
            truth->dict_row[k] = T.dict_row[k];
            for (int i = 0; i < 9; i++) truth->R[k][i] = T.R[k][i];
            for (int i = 0; i < 3; i++) truth->t[k][i] = T.t[k][i];
            truth->radius[k] = T.radius[k];
        }
    }
    return CTAG_OK;
}

int ctag_synth3d_model(const int32_t* state, int dict_rows, int dict_cols, float* corners) {
    if (!state || !corners || dict_rows < 1 || dict_cols < 1 || dict_cols > ctag_synth::kMaxCols) return CTAG_ERR_ARG;
    for (int r = 0; r < dict_rows; r++) ctag_synth::model_corners(state, dict_cols, r, corners + (size_t)r * dict_cols * 24);
    return CTAG_OK;
}

int ctag_synth_layout_truth(const int32_t* state, int dict_rows, int dict_cols, int frame_index, int rows, int cols, uint64_t seed, int markers_per_frame,
                            ctag_synth_truth* truth) {
    if (!state || !truth || rows < 1 || cols < 1 || dict_rows < 1 || dict_cols < 1) return CTAG_ERR_ARG;
    ctag_synth::Frame F;
    ctag_synth::Truth T;
    ctag_synth::layout(state, dict_rows, dict_cols, seed, frame_index, rows, cols, markers_per_frame, &F, &T);
    fill_truth(T, truth);
    return CTAG_OK;
}

int ctag_synth_frame_host(const int32_t* state, int dict_rows, int dict_cols, uint8_t* frame, int frame_index, int rows, int cols, ptrdiff_t row_stride,
                          uint64_t seed, int markers_per_frame, ctag_synth_truth* truth) {
    if (!state || !frame || rows < 1 || cols < 1 || row_stride < cols || dict_rows < 1 || dict_cols < 1) return CTAG_ERR_ARG;
    ctag_synth::Frame F;
    ctag_synth::Truth T;
    ctag_synth::layout(state, dict_rows, dict_cols, seed, frame_index, rows, cols, markers_per_frame, &F, &T);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) frame[(ptrdiff_t)y * row_stride + x] = ctag_synth::pixel(F, x, y, rows, cols);
    if (truth) fill_truth(T, truth);
    return CTAG_OK;
}

int ctag_testkit_dense_edge_probe(ctag_handle* h, const uint8_t* gray, int rows, int cols, ptrdiff_t row_stride, const double* segments,
                                  int n_seg, const double* K, const double* dist, const double* rvec, const double* tvec,
                                  int samples_per_edge, double search_px, double min_contrast, double* out, int32_t* keep) {
    if (!h || !gray || !segments || !K || !dist || !rvec || !tvec || !out || !keep) return CTAG_ERR_ARG;
    if (rows < 2 || cols < 2 || rows > 32768 || cols > 32768 || row_stride < cols || n_seg < 1 || n_seg > 4096) return CTAG_ERR_ARG;
    if (samples_per_edge < 1 || samples_per_edge > 64 || !(search_px >= 0.5 && search_px <= 8.0) || !(min_contrast >= 0.0)) return CTAG_ERR_ARG;
    const double q = search_px * 4.0;
    if (q != (double)(int)q) return CTAG_ERR_ARG;
    const int nt = (int)q + 1;  // <= kDenseMaxTaps
    DenseProbeCam cam{};
    cam.fx = K[0];
    cam.fy = K[4];
    cam.cx = K[2];
    cam.cy = K[5];
    for (int i = 0; i < 14; i++) cam.k[i] = dist[i];
    HandleView v{};
    handle_view(h, &v);
    TK_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const size_t img_bytes = (size_t)(rows - 1) * row_stride + cols, n = (size_t)n_seg * samples_per_edge;
    uint8_t* dimg = nullptr;
    double *dseg = nullptr, *dout = nullptr;
    int32_t* dkeep = nullptr;
    int rc = CTAG_OK;
    if (hipMalloc(reinterpret_cast<void**>(&dimg), img_bytes) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&dseg), (size_t)n_seg * 12 * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dout), n * 5 * 8) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&dkeep), n * 4) != hipSuccess)
        rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK && (hipMemcpy(dimg, gray, img_bytes, hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(dseg, segments, (size_t)n_seg * 12 * 8, hipMemcpyHostToDevice) != hipSuccess))
        rc = CTAG_ERR_HIP;
    if (rc == CTAG_OK) {
        hipLaunchKernelGGL(k_dense_edge_probe, dim3(1), dim3(64), 0, s, dimg, rows, cols, row_stride, dseg, n_seg, cam, rvec[0], rvec[1], rvec[2],
                           tvec[0], tvec[1], tvec[2], samples_per_edge, nt, search_px, min_contrast, dout, dkeep);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(out, dout, n * 5 * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(keep, dkeep, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
            rc = CTAG_ERR_HIP;
    }
    (void)hipFree(dimg);
    (void)hipFree(dseg);
    (void)hipFree(dout);
    (void)hipFree(dkeep);
    return rc;
}

int ctag_testkit_welsch_fit(ctag_handle* h, int n_frames, const int32_t* edges_per_frame, const int32_t* points_per_edge, const int32_t* xy, int latency,
                            int welsch_gx, int welsch_gs, int tail_at_pool_end, float* lines) {
    if (!h || n_frames < 1 || !edges_per_frame || welsch_gx < 0 || welsch_gs < 0 || welsch_gx + welsch_gs > 65535) return CTAG_ERR_ARG;
    HandleView v{};
    handle_view(h, &v);
    if (!v.ws || !v.ws->base || n_frames > v.last_chunk_frames) return CTAG_ERR_ARG;
    const Workspace& W = *v.ws;
    if (latency && (n_frames > kLatencyFrames || !W.welsch_rs)) return CTAG_ERR_ARG;
    // the frames' descriptors and packed points as they will lie in the workspace; every limit is checked before anything is written
    std::vector<std::vector<LineDesc>> desc(n_frames);
    std::vector<std::vector<uint32_t>> pool(n_frames);
    std::vector<uint32_t> base(n_frames, 0u);
    size_t e0 = 0, p0 = 0;
    for (int f = 0; f < n_frames; f++) {
        const int L = edges_per_frame[f];
        if (L < 0 || L > W.line_cap || (L > 0 && (!points_per_edge || !xy || !lines))) return CTAG_ERR_ARG;
        size_t total = 0;
        for (int i = 0; i < L; i++) {
            const int n = points_per_edge[e0 + i];
            if (n < 2 || (size_t)n > (size_t)W.cl_cap) return CTAG_ERR_ARG;
            total += (size_t)n;
            if (total > (size_t)W.cl_cap) return CTAG_ERR_ARG;
        }
        base[f] = tail_at_pool_end ? (uint32_t)(W.cl_cap - total) : 0u;
        desc[f].resize(L);
        pool[f].resize(total);
        uint32_t off = 0;
        for (int i = 0; i < L; i++) {
            const int n = points_per_edge[e0 + i];
            desc[f][i] = LineDesc{base[f] + off, n};
            for (int j = 0; j < n; j++) {
                const int32_t x = xy[(p0 + off + j) * 2], y = xy[(p0 + off + j) * 2 + 1];
                if (x < 0 || x > 65535 || y < 0 || y > 65535) return CTAG_ERR_ARG;
                pool[f][off + j] = (uint32_t)x | ((uint32_t)y << 16);
            }
            off += (uint32_t)n;
        }
        e0 += (size_t)L;
        p0 += total;
    }
    TK_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    TK_TRY(hipStreamSynchronize(s));
    TK_TRY(hipMemcpy(W.line_count, edges_per_frame, (size_t)n_frames * 4, hipMemcpyHostToDevice));
    for (int f = 0; f < n_frames; f++) {
        if (desc[f].empty()) continue;
        TK_TRY(hipMemcpy(W.line_desc + (size_t)f * W.line_cap, desc[f].data(), desc[f].size() * sizeof(LineDesc), hipMemcpyHostToDevice));
        TK_TRY(hipMemcpy(W.cl_pool + (size_t)f * W.cl_cap + base[f], pool[f].data(), pool[f].size() * 4, hipMemcpyHostToDevice));
        TK_TRY(hipMemsetAsync(W.line_fit + (size_t)f * W.line_cap * 4, 0xff, desc[f].size() * 16, s));  // a line no kernel writes reads back as NaNs, not as an earlier call's
    }
    const FrameGeom& g = W.g;
    ChunkPlan pl = plan_chunk(PlanIn{g.rows, g.cols, g.tw, n_frames, 1, 1, nullptr, 0, 0, W.kp, 0, 0, false, DevKnobs{}});
    pl.latency = latency != 0;
    if (welsch_gx > 0) pl.welsch_gx = welsch_gx;
    if (welsch_gs > 0) pl.welsch_gs = welsch_gs;
    if (launch_line_fits(pl, W, s) != hipSuccess) {
        (void)hipGetLastError();  // (the launcher leaves it for its caller)
        return CTAG_ERR_HIP;
    }
    TK_TRY(hipStreamSynchronize(s));
    e0 = 0;
    for (int f = 0; f < n_frames; f++) {
        if (desc[f].empty()) continue;
        TK_TRY(hipMemcpy(lines + e0 * 4, W.line_fit + (size_t)f * W.line_cap * 4, desc[f].size() * 16, hipMemcpyDeviceToHost));
        e0 += desc[f].size();
    }
    return CTAG_OK;
}

int ctag_testkit_welsch_limits(int32_t* out, int capacity) { return welsch_limits(out, out ? std::max(capacity, 0) : 0); }

int ctag_testkit_refine_sums(ctag_handle* h, int n_frames, const int32_t* nfeat, const int32_t* status, const float* corners, const double* n0, double* sums) {
    if (!h || n_frames < 1 || !nfeat || !status) return CTAG_ERR_ARG;
    HandleView v{};
    handle_view(h, &v);
    if (!v.ws || !v.ws->base || !v.ws->refine_n0 || n_frames > v.last_chunk_frames) return CTAG_ERR_ARG;
    const Workspace& W = *v.ws;
    size_t total = 0;
    for (int f = 0; f < n_frames; f++) {
        if (nfeat[f] < 0 || nfeat[f] > CTAG_MAX_FEATURES) return CTAG_ERR_ARG;
        total += (size_t)nfeat[f];
    }
    if (total > 0 && (!corners || !n0 || !sums)) return CTAG_ERR_ARG;
    const FrameGeom& g = W.g;
    const ChunkPlan pl = plan_chunk(PlanIn{g.rows, g.cols, g.tw, n_frames, 1, 1, nullptr, 0, 0, W.kp, 0, 0, false, DevKnobs{}});
    if (pl.refine == RefineForm::None || pl.refine == RefineForm::One) return CTAG_ERR_ARG;  // the chain would not launch this kernel for such a call
    constexpr size_t kQuad = 4 * 128;  // doubles of a quad's n0 block
    TK_TRY(hipSetDevice(v.device));
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    TK_TRY(hipStreamSynchronize(s));
    TK_TRY(hipMemcpy(W.nfeat, nfeat, (size_t)n_frames * 4, hipMemcpyHostToDevice));
    TK_TRY(hipMemcpy(W.status, status, (size_t)n_frames * 4, hipMemcpyHostToDevice));
    size_t f0 = 0;
    for (int f = 0; f < n_frames; f++) {
        const size_t nf = (size_t)nfeat[f];
        if (nf == 0) continue;
        std::vector<FeatureDev> feats(nf);
        for (size_t k = 0; k < nf; k++) {
            FeatureDev F{};
            std::memcpy(F.c, corners + (f0 + k) * 16, sizeof(F.c));
            feats[k] = F;
        }
        TK_TRY(hipMemcpy(W.feat1 + (size_t)f * CTAG_MAX_FEATURES, feats.data(), nf * sizeof(FeatureDev), hipMemcpyHostToDevice));
        TK_TRY(hipMemcpy(W.refine_n0 + (size_t)f * (CTAG_MAX_FEATURES * 2) * kQuad, n0 + f0 * 2 * kQuad, nf * 2 * kQuad * 8, hipMemcpyHostToDevice));
        f0 += nf;
    }
    if (launch_edge_refine_sums(pl, W, s) != hipSuccess) {
        (void)hipGetLastError();
        return CTAG_ERR_HIP;
    }
    TK_TRY(hipStreamSynchronize(s));
    f0 = 0;
    for (int f = 0; f < n_frames; f++) {
        const size_t nq = (size_t)nfeat[f] * 2;
        if (nq == 0) continue;
        TK_TRY(hipMemcpy2D(sums + f0 * 49, 49 * 8, W.refine_n0 + (size_t)f * (CTAG_MAX_FEATURES * 2) * kQuad, kQuad * 8, 49 * 8, nq, hipMemcpyDeviceToHost));
        f0 += nq;
    }
    return CTAG_OK;
}

int ctag_testkit_model_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_pose_rec* poses, int n_poses,
                                  const ctag_model* model, const ctag_camera* camera, int model_index, double lambda, int min_obs, int pass_records,
                                  double* S, double* g, double* delta, int32_t* held, int32_t* bad_pivot) {
    return mfit_probe_system(h, results, n_frames, poses, n_poses, model, camera, model_index, lambda, min_obs, pass_records, S, g, delta, held, bad_pivot);
}

int ctag_testkit_model_fit_limits(int32_t* out, int capacity) {
    const int32_t v[2] = {mfit_record_grid(), mfit_pass_records()};
    if (out) std::memcpy(out, v, sizeof(int32_t) * (size_t)std::min(std::max(capacity, 0), 2));
    return 2;
}

int ctag_testkit_rig_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* rig_poses,
                                const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* camera, int rig, double lambda, int pass_records,
                                double* S, double* g, double* delta, int32_t* n_unknowns, int32_t* bad_pivot) {
    return rfit_probe_system(h, results, n_frames, rig_poses, model, rigs, camera, rig, lambda, pass_records, S, g, delta, n_unknowns, bad_pivot);
}

int ctag_testkit_rig_fit_limits(int32_t* out, int capacity) {
    const int32_t v[2] = {rfit_record_grid(), rfit_pass_records()};
    if (out) std::memcpy(out, v, sizeof(int32_t) * (size_t)std::min(std::max(capacity, 0), 2));
    return 2;
}

int ctag_testkit_camera_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_mv_pose_rec* mv_poses,
                                   const ctag_model* model, const ctag_rigs* rigs, const ctag_camera_set* cams, int anchor, double lambda,
                                   int pass_records, double* S, double* g, double* delta, int32_t* n_unknowns, int32_t* bad_pivot) {
    return cfit_probe_system(h, results, n_frames, mv_poses, model, rigs, cams, anchor, lambda, pass_records, S, g, delta, n_unknowns, bad_pivot);
}

int ctag_testkit_intrinsics_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* poses,
                                       const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* camera, uint32_t free_mask, int tie_focal,
                                       double lambda, int pass_records, double* S, double* g, double* delta, int32_t* n_free, int32_t* bad_pivot) {
    return ifit_probe_system(h, results, n_frames, poses, model, rigs, camera, free_mask, tie_focal, lambda, pass_records, S, g, delta, n_free, bad_pivot);
}

int ctag_testkit_intrinsics_fit_poses(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* poses,
                                      const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* camera, ctag_rig_pose_rec* out, int32_t* usable) {
    return ifit_probe_poses(h, results, n_frames, poses, model, rigs, camera, out, usable);
}

int ctag_testkit_intrinsics_fit_limits(int32_t* out, int capacity) {
    const int32_t v[2] = {ifit_record_grid(), ifit_pass_records()};
    if (out) std::memcpy(out, v, sizeof(int32_t) * (size_t)std::min(std::max(capacity, 0), 2));
    return 2;
}

int ctag_testkit_camera_fit_limits(int32_t* out, int capacity) {
    const int32_t v[2] = {cfit_record_grid(), cfit_pass_records()};
    if (out) std::memcpy(out, v, sizeof(int32_t) * (size_t)std::min(std::max(capacity, 0), 2));
    return 2;
}

int ctag_testkit_plan(int rows, int cols, int adaptive_thresh, int nframes, int channels, int corner_subpix, const void* frames, ptrdiff_t frame_stride,
                      ptrdiff_t row_stride, int fuse_mode, int wave_points, int bgr_direct, int expand_exact, int32_t* out, int capacity) {
    // KParams of ctag_params_default as far as the plan reads them (threshold_line 1.8, threshold_expand 1.2, collinear_cost 1.05)
    KParams kp{};
    kp.thr_line = 1.8f;
    kp.thr_expand = 1.2f;
    kp.c2_far = 2;
    kp.c2_near = 1;
    kp.expand_eps = expand_exact ? INFINITY : 3.0e-6f;
    const ChunkPlan p = plan_chunk(PlanIn{rows, cols, adaptive_thresh, nframes, channels, corner_subpix, frames, frame_stride, row_stride, kp, fuse_mode, wave_points,
                                          bgr_direct != 0, DevKnobs{}});
    const int32_t f[] = {p.fused, p.bgr_direct, p.zero_first, p.dec_zero_kernel, p.dec_zero_list, (int32_t)p.dec, p.dec_xblocks, p.dec_yblocks, p.dec_band_rows,
                         p.dec_bands, (int32_t)p.ccl, p.latency, p.small_cfg, p.refprm, p.mask_scan, p.prescan, p.all_wave, p.fork, p.pack_max, p.big_points,
                         p.pack_gx, p.scan_gx, p.mscan_gx, p.big_cols, p.big_max_gx, p.welsch_gs, p.welsch_gx, (int32_t)p.refine, p.refine_gx, p.refine_sums_gx};
    constexpr int n = (int)(sizeof(f) / sizeof(f[0]));
    if (out) std::memcpy(out, f, sizeof(int32_t) * (size_t)std::min(std::max(capacity, 0), n));
    return n;
}

}  // extern "C"
