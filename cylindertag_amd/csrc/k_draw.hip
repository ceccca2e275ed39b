// k_draw.hip -- the overlay of CylinderTag::drawAxis (CylinderTag.cpp:211-246) on the device, from the pose records
// ctag_pose_batch_device leaves in HBM (include/ctag_pose.h: ctag_draw_axis, ctag_draw_axis_batch_device).
//
// Per frame the reference does  cvtColor(GRAY2RGB)  and then, pose record by pose record, draws with OpenCV 4.5.3's
// painter: filled circles (radius 5) at the projected corners, three arrowedLine(thickness 10, LINE_AA, tip 0.2) from the
// projected base and a filled circle (radius 8) at the base.  Two kernels restate that:
//
//   k_draw_expand  gray -> 3 equal channels, a coalesced sweep over every pixel of every frame (the only HBM-sized work:
//                  1 B read + 3 B written per pixel).
//   k_draw_raster  one wavefront per frame.  It walks the frame's records in order; for each it projects the record's
//                  <= 164 model points (lanes over points, cv::projectPoints' full model) into LDS, then runs the
//                  record's primitives in the painter's order, one operation at a time, with that operation's pixels
//                  spread over the 64 lanes and a barrier behind it.  A pixel that several operations touch (the AA
//                  edges of a thick line, its interior fill, its two round caps, the next line, the next marker) sees
//                  them in the sequential painter's order, so the bytes are the painter's bytes.
//
// Third-party arithmetic restated here (OpenCV 4.5.3 modules/imgproc/src/drawing.cpp, modules/calib3d/src/calibration.cpp;
// not vendored by the reference, absent from this image): Circle, ThickLine, FillConvexPoly, LineAA, clipLine, EllipseEx,
// ellipse2Poly, arrowedLine, cvProjectPoints2Internal, Rodrigues.  Integer coordinates carry XY_SHIFT = 16 fraction bits
// as there.  Rules the reference leaves undefined are stated in include/ctag_pose.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <new>

#include "../../include/ctag_pose.h"
#include "ctag_internal.h"
#include "ctag_math.h"

namespace ctag {
namespace {

constexpr int kXYShift = 16;
constexpr long long kXYOne = 1LL << kXYShift;
constexpr int kDrawPts = CTAG_MAX_CODE_POS * 8 + 4;  // corners of 20 code positions + base + three axis ends
constexpr int kWave = 64;

// drawing.cpp: SlopeCorrTable, FilterTable (LineAA's coverage tables)
__constant__ int kSlopeCorr[32] = {181, 181, 181, 182, 182, 183, 184, 185, 187, 188, 190, 192, 194, 196, 198, 201,
                                   203, 206, 209, 211, 214, 218, 221, 224, 227, 231, 235, 238, 242, 246, 250, 254};
__constant__ int kFilter[64] = {168, 177, 185, 194, 202, 210, 218, 224, 231, 236, 241, 246, 249, 252, 254, 254,
                                254, 254, 252, 249, 246, 241, 236, 231, 224, 218, 210, 202, 194, 185, 177, 168,
                                158, 149, 140, 131, 122, 114, 105, 97,  89,  82,  75,  68,  62,  56,  50,  45,
                                40,  35,  31,  27,  24,  20,  18,  15,  13,  11,  9,   7,   6,   5,   3,   2};
// drawing.cpp SinTable[a] at a = 0, 30, ..., 450 degrees (ellipse2Poly with delta 30, the step EllipseEx picks for a radius of 5)
__constant__ float kSin30[16] = {0.0000000f, 0.5000000f, 0.8660254f, 1.0000000f, 0.8660254f, 0.5000000f, 0.0000000f, -0.5000000f,
                                 -0.8660254f, -1.0000000f, -0.8660254f, -0.5000000f, 0.0000000f, 0.5000000f, 0.8660254f, 1.0000000f};

struct DrawCam {
    double fx, fy, cx, cy;
    double k[12];
};

struct DrawModel {
    int n_models, model_size;
    const float* corners;  // [n_models][model_size*8][3]
    const float* base;     // [n_models][3]
    const float* axis;     // [n_models][3]
};

struct Target {
    uint8_t* img;
    ptrdiff_t step;
    int w, h;
};

struct Col {
    int c0, c1, c2;
};

// cvRound: nearest, ties to even; saturated to int (the Point2f -> Point conversion of the reference's circle / arrowedLine calls)
__device__ __forceinline__ int round_sat(double v) {
    const double r = __builtin_rint(v);
    if (r >= 2147483647.0) return INT_MAX;
    if (r <= -2147483648.0) return INT_MIN;
    return (int)r;
}

__device__ __forceinline__ void put_opaque(const Target& t, int x, int y, const Col& c) {
    uint8_t* p = t.img + (ptrdiff_t)y * t.step + (ptrdiff_t)x * 3;
    p[0] = (uint8_t)c.c0;
    p[1] = (uint8_t)c.c1;
    p[2] = (uint8_t)c.c2;
}

// LineAA's ICV_PUT_POINT for 3 channels: the coverage a is applied twice per channel
__device__ __forceinline__ int blend2(int v, int c, int a) {
    v += ((c - v) * a + 127) >> 8;
    v += ((c - v) * a + 127) >> 8;
    return v;
}
__device__ __forceinline__ void put_aa(const Target& t, int x, int y, int a, const Col& c) {
    uint8_t* p = t.img + (ptrdiff_t)y * t.step + (ptrdiff_t)x * 3;
    const int b0 = p[0], b1 = p[1], b2 = p[2];
    p[0] = (uint8_t)blend2(b0, c.c0, a);
    p[1] = (uint8_t)blend2(b1, c.c1, a);
    p[2] = (uint8_t)blend2(b2, c.c2, a);
}

// ------------------------------------------------------------------------------------------------ clipLine (Size2l, Point2l&)
__device__ bool clip_line(long long W, long long H, long long& x1, long long& y1, long long& x2, long long& y2) {
    if (W <= 0 || H <= 0) return false;
    const long long right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// ------------------------------------------------------------------------------------------------ LineAA (Point2l, XY_SHIFT units)
// The sequential loop runs ecount+1 steps; step s touches three pixels of one column (x-major) or one row (y-major), so the
// pixels of one call are distinct and its steps run on the lanes in any order.
__device__ void line_aa(const Target& t, long long x1, long long y1, long long x2, long long y2, const Col& col, int lane) {
    if (!clip_line((long long)t.w << kXYShift, (long long)t.h << kXYShift, x1, y1, x2, y2)) return;
    long long dx = x2 - x1, dy = y2 - y1;
    long long j = dx < 0 ? -1 : 0;
    const long long ax = (dx ^ j) - j;
    long long i = dy < 0 ? -1 : 0;
    const long long ay = (dy ^ i) - i;
    long long x_step, y_step;
    int ecount, slope;
    const bool xmajor = ax > ay;
    if (xmajor) {
        dy = (dy ^ j) - j;
        x1 ^= x2 & j;
        x2 ^= x1 & j;
        x1 ^= x2 & j;
        y1 ^= y2 & j;
        y2 ^= y1 & j;
        y1 ^= y2 & j;
        x_step = kXYOne;
        y_step = (dy * kXYOne) / (ax | 1);
        x2 += kXYOne;
        ecount = (int)((x2 >> kXYShift) - (x1 >> kXYShift));
        j = -(x1 & (kXYOne - 1));
        y1 += ((y_step * j) >> kXYShift) + (kXYOne >> 1);
        slope = (int)((y_step >> (kXYShift - 5)) & 0x3f);
        slope ^= (y_step < 0 ? 0x3f : 0);
        i = (x1 >> (kXYShift - 7)) & 0x78;
        j = (x2 >> (kXYShift - 7)) & 0x78;
    } else {
        dx = (dx ^ i) - i;
        x1 ^= x2 & i;
        x2 ^= x1 & i;
        x1 ^= x2 & i;
        y1 ^= y2 & i;
        y2 ^= y1 & i;
        y1 ^= y2 & i;
        x_step = (dx * kXYOne) / (ay | 1);
        y_step = kXYOne;
        y2 += kXYOne;
        ecount = (int)((y2 >> kXYShift) - (y1 >> kXYShift));
        j = -(y1 & (kXYOne - 1));
        x1 += ((x_step * j) >> kXYShift) + (kXYOne >> 1);
        slope = (int)((x_step >> (kXYShift - 5)) & 0x3f);
        slope ^= (x_step < 0 ? 0x3f : 0);
        i = (y1 >> (kXYShift - 7)) & 0x78;
        j = (y2 >> (kXYShift - 7)) & 0x78;
    }
    slope = (slope & 0x20) ? 0x100 : kSlopeCorr[slope];
    int ep[9];
    {  // end point correction table
        const int ii = (int)i, jj = (int)j;
        const int t0 = slope << 7;
        const int t1 = ((0x78 - ii) | 4) * slope;
        const int t2 = (jj | 4) * slope;
        ep[0] = 0;
        ep[8] = slope;
        ep[1] = ep[3] = ((((jj - ii) & 0x78) | 4) * slope >> 8) & 0x1ff;
        ep[2] = (t1 >> 8) & 0x1ff;
        ep[4] = ((((jj - ii) + 0x80) | 4) * slope >> 8) & 0x1ff;
        ep[5] = ((t1 + t0) >> 8) & 0x1ff;
        ep[6] = (t2 >> 8) & 0x1ff;
        ep[7] = ((t2 + t0) >> 8) & 0x1ff;
    }
    const int major0 = (int)((xmajor ? x1 : y1) >> kXYShift);
    const long long minor0 = xmajor ? y1 : x1, mstep = xmajor ? y_step : x_step;
    const int lim_major = xmajor ? t.w : t.h, lim_minor = xmajor ? t.h : t.w;
    for (int s = lane; s <= ecount; s += kWave) {
        const int m = major0 + s;
        if ((unsigned)m >= (unsigned)lim_major) continue;
        const long long p = minor0 + (long long)s * mstep;
        const int n = (int)((p >> kXYShift) - 1);
        const int sc = s, ec = ecount - s;
        const int epi = (((sc >= 2) + 1) & (sc | 2)) * 3 + (((ec >= 2) + 1) & (ec | 2));
        const int ep_corr = epi == 0 ? ep[0] : epi == 1 ? ep[1] : epi == 2 ? ep[2] : epi == 3 ? ep[3] : epi == 4 ? ep[4]
                          : epi == 5 ? ep[5] : epi == 6 ? ep[6] : epi == 7 ? ep[7] : ep[8];
        const int dist = (int)((p >> (kXYShift - 5)) & 31);
        const int a0 = (ep_corr * kFilter[dist + 32] >> 8) & 0xff;
        const int a1 = (ep_corr * kFilter[dist] >> 8) & 0xff;
        const int a2 = (ep_corr * kFilter[63 - dist] >> 8) & 0xff;
        const int av[3] = {a0, a1, a2};
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if ((unsigned)(n + q) >= (unsigned)lim_minor) continue;
            if (xmajor)
                put_aa(t, m, n + q, av[q], col);
            else
                put_aa(t, n + q, m, av[q], col);
        }
    }
}

// ------------------------------------------------------------------------------------------------ FillConvexPoly (line_type LINE_AA, shift XY_SHIFT)
// The sequential scan walks y from ymin and advances the left and right edge chains at rows where they end.  Row y's span
// follows from the same edge events replayed up to y (at most npts of them) and x = x_set + dx * (y - y_set), which is the
// sequential x += dx exactly (integer arithmetic); so the rows run on the lanes independently.
struct PolyScan {
    int npts, imin, ymin, ymax;  // ymax clamped to the frame as in the sequential loop
};

__device__ bool poly_row(const long long* vx, const long long* vy, const PolyScan& ps, int y, long long* xa, long long* xb) {
    const long long delta = kXYOne >> 1;
    int idx[2] = {ps.imin, ps.imin}, ye[2] = {ps.ymin, ps.ymin}, yset[2] = {ps.ymin, ps.ymin};
    const int di[2] = {1, ps.npts - 1};
    long long ex[2] = {-kXYOne, -kXYOne}, edx[2] = {0, 0};
    int edges = ps.npts;
    int yy = ps.ymin;
    for (;;) {
        if (yy < ps.ymax || yy == ps.ymin) {
            for (int e = 0; e < 2; e++) {
                if (yy < ye[e]) continue;
                int i0 = idx[e], ii = i0 + di[e];
                if (ii >= ps.npts) ii -= ps.npts;
                for (; edges-- > 0;) {
                    const int ty = (int)((vy[ii] + delta) >> kXYShift);
                    if (ty > yy) {
                        const long long xs = vx[i0], xe = vx[ii];
                        ye[e] = ty;
                        edx[e] = ((xe - xs) * 2 + (ty - yy)) / (2 * (long long)(ty - yy));
                        ex[e] = xs;
                        yset[e] = yy;
                        idx[e] = ii;
                        break;
                    }
                    i0 = ii;
                    ii += di[e];
                    if (ii >= ps.npts) ii -= ps.npts;
                }
            }
        }
        if (edges < 0) return false;  // the sequential loop ends at row yy
        const int nxt = ye[0] < ye[1] ? ye[0] : ye[1];
        if (yy >= y || nxt > y) break;
        yy = nxt;
    }
    xa[0] = ex[0] + edx[0] * (long long)(y - yset[0]);
    xb[0] = ex[1] + edx[1] * (long long)(y - yset[1]);
    return true;
}

__device__ void fill_convex_poly_aa(const Target& t, const long long* vx, const long long* vy, int npts, const Col& col, int lane) {
    {  // the edges first, LineAA each, in the polygon's order starting with the closing edge
        int p = npts - 1;
        for (int i = 0; i < npts; i++) {
            line_aa(t, vx[p], vy[p], vx[i], vy[i], col, lane);
            __syncthreads();
            p = i;
        }
    }
    const long long delta = kXYOne >> 1;
    long long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int imin = 0;
    for (int i = 0; i < npts; i++) {
        if (vy[i] < ymin) {
            ymin = vy[i];
            imin = i;
        }
        ymax = vy[i] > ymax ? vy[i] : ymax;
        xmax = vx[i] > xmax ? vx[i] : xmax;
        xmin = vx[i] < xmin ? vx[i] : xmin;
    }
    xmin = (xmin + delta) >> kXYShift;
    xmax = (xmax + delta) >> kXYShift;
    ymin = (ymin + delta) >> kXYShift;
    ymax = (ymax + delta) >> kXYShift;
    if (npts < 3 || (int)xmax < 0 || (int)ymax < 0 || (int)xmin >= t.w || (int)ymin >= t.h) return;
    PolyScan ps{npts, imin, (int)ymin, (int)std::min<long long>(ymax, t.h - 1)};
    const int y0 = ps.ymin > 0 ? ps.ymin : 0;
    for (int y = y0 + lane; y <= ps.ymax; y += kWave) {
        long long e0, e1;
        if (!poly_row(vx, vy, ps, y, &e0, &e1)) continue;
        const long long xl = e0 > e1 ? e1 : e0, xr = e0 > e1 ? e0 : e1;
        int xx1 = (int)((xl + kXYOne - 1) >> kXYShift);
        int xx2 = (int)(xr >> kXYShift);
        if (xx2 < 0 || xx1 >= t.w) continue;
        xx1 = xx1 < 0 ? 0 : xx1;
        xx2 = xx2 >= t.w ? t.w - 1 : xx2;
        for (int x = xx1; x <= xx2; x++) put_opaque(t, x, y, col);
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ ThickLine (thickness 10, LINE_AA, flags 3)
// line(img, p0, p1, color, 10, LINE_AA, 0): the body polygon, then EllipseEx round caps (radius 5 px) at p0 and at p1.
__device__ void thick_line_aa10(const Target& t, int p0x, int p0y, int p1x, int p1y, const Col& col, int lane) {
    long long ax = (long long)p0x << kXYShift, ay = (long long)p0y << kXYShift;
    const long long bx = (long long)p1x << kXYShift, by = (long long)p1y << kXYShift;
    const long long thickness = 10LL << (kXYShift - 1);  // thickness <<= XY_SHIFT - 1; even: no half-pixel term
    long long vx[13], vy[13];
    {
        const double INV = 1. / (double)kXYOne;
        const double dx = (double)(ax - bx) * INV, dy = (double)(by - ay) * INV;
        double r = dx * dx + dy * dy;
        if (ctm::fabs64(r) > 2.220446049250313080847e-16) {
            r = ((double)thickness + 0.0) / __builtin_sqrt(r);
            const long long dpx = round_sat(dy * r), dpy = round_sat(dx * r);
            vx[0] = ax + dpx, vy[0] = ay + dpy;
            vx[1] = ax - dpx, vy[1] = ay - dpy;
            vx[2] = bx - dpx, vy[2] = by - dpy;
            vx[3] = bx + dpx, vy[3] = by + dpy;
            fill_convex_poly_aa(t, vx, vy, 4, col, lane);
        }
    }
    for (int c = 0; c < 2; c++) {
        // EllipseEx(img, p, Size2l(thickness, thickness), 0, 0, 360, color, -1, LINE_AA): ellipse2Poly with delta 30 (radius 5 px),
        // each vertex rounded to whole pixels plus the rounded remainder
        const double cx = (double)ax, cy = (double)ay, rad = (double)thickness;
        for (int k = 0; k < 13; k++) {
            const int ang = 30 * k;
            const double x = rad * (double)kSin30[(450 - ang) / 30];
            const double y = rad * (double)kSin30[ang / 30];
            const double px = cx + x * 1.0 - y * 0.0, py = cy + x * 0.0 + y * 1.0;
            long long qx = (long long)round_sat(px / (double)kXYOne) << kXYShift;
            long long qy = (long long)round_sat(py / (double)kXYOne) << kXYShift;
            qx += round_sat(px - (double)qx);
            qy += round_sat(py - (double)qy);
            vx[k] = qx;
            vy[k] = qy;
        }
        int n = 1;  // consecutive duplicates dropped
        for (int k = 1; k < 13; k++)
            if (vx[k] != vx[n - 1] || vy[k] != vy[n - 1]) {
                vx[n] = vx[k];
                vy[n] = vy[k];
                n++;
            }
        if (n == 1) {
            vx[1] = vx[0] = ax;
            vy[1] = vy[0] = ay;
            n = 2;
        }
        fill_convex_poly_aa(t, vx, vy, n, col, lane);
        ax = bx;
        ay = by;
    }
}

// ------------------------------------------------------------------------------------------------ arrowedLine (thickness 10, LINE_AA, tipLength 0.2)
__device__ void arrowed_line(const Target& t, int p1x, int p1y, int p2x, int p2y, const Col& col, int lane) {
    const double ddx = (double)((long long)p1x - p2x), ddy = (double)((long long)p1y - p2y);
    const double tip = __builtin_sqrt(ddx * ddx + ddy * ddy) * 0.2;
    thick_line_aa10(t, p1x, p1y, p2x, p2y, col, lane);
    const double angle = ctm::atan2_64((double)p1y - (double)p2y, (double)p1x - (double)p2x);
    const double pi4 = 3.14159265358979323846 / 4;
    int qx = round_sat((double)p2x + tip * ctm::cos64(angle + pi4));
    int qy = round_sat((double)p2y + tip * ctm::sin64(angle + pi4));
    thick_line_aa10(t, qx, qy, p2x, p2y, col, lane);
    qx = round_sat((double)p2x + tip * ctm::cos64(angle - pi4));
    qy = round_sat((double)p2y + tip * ctm::sin64(angle - pi4));
    thick_line_aa10(t, qx, qy, p2x, p2y, col, lane);
}

// ------------------------------------------------------------------------------------------------ Circle (filled, LINE_8, shift 0)
// Its hlines are opaque and of one colour, so a run of circles of one colour is the union of their pixels in any order.
// hw[o]: half width of the row o rows off the centre (the midpoint loop's spans, widest wins).
__device__ void circle_half_widths(int radius, int* hw) {
    for (int o = 0; o <= radius; o++) hw[o] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[dy] = hw[dy] > dx ? hw[dy] : dx;
        hw[dx] = hw[dx] > dy ? hw[dx] : dy;
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// disks of `radius` at the listed centres (LDS), union painted with one colour
__device__ void disks(const Target& t, const int* cx, const int* cy, const int* ok, int first, int count, int radius, const int* hw,
                      const Col& col, int lane) {
    const int side = 2 * radius + 1, area = side * side;
    for (int q = lane; q < count * area; q += kWave) {
        const int k = first + q / area, o = q % area;
        if (!ok[k]) continue;
        const int oy = o / side - radius, ox = o % side - radius;
        if ((ox < 0 ? -ox : ox) > hw[oy < 0 ? -oy : oy]) continue;
        const long long x = (long long)cx[k] + ox, y = (long long)cy[k] + oy;
        if (x < 0 || y < 0 || x >= t.w || y >= t.h) continue;
        put_opaque(t, (int)x, (int)y, col);
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ Rodrigues + projectPoints
__device__ void rodrigues(const double* rv, double* R) {
    const double rx = rv[0], ry = rv[1], rz = rv[2];
    const double theta = __builtin_sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < 2.220446049250313080847e-16) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double c = ctm::cos64(theta), s = ctm::sin64(theta), c1 = 1. - c;
    const double it = theta ? 1. / theta : 0.;
    const double x = rx * it, y = ry * it, z = rz * it;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx_[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int i = 0; i < 9; i++) R[i] = (c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * rx_[i];
}

// one point through cvProjectPoints2Internal (no tilt: tau_x = tau_y = 0), output rounded to float as Point2f
__device__ bool project_point(const double* R, const double* tv, const DrawCam& cam, float X_, float Y_, float Z_, float* u, float* v) {
    const double X = X_, Y = Y_, Z = Z_;
    double x = R[0] * X + R[1] * Y + R[2] * Z + tv[0];
    double y = R[3] * X + R[4] * Y + R[5] * Z + tv[1];
    double z = R[6] * X + R[7] * Y + R[8] * Z + tv[2];
    z = z ? 1. / z : 1;
    x *= z;
    y *= z;
    const double* k = cam.k;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
    const double icdist2 = 1. / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
    const double xd0 = x * cdist * icdist2 + k[2] * a1 + k[3] * a2 + k[8] * r2 + k[9] * r4;
    const double yd0 = y * cdist * icdist2 + k[2] * a3 + k[3] * a1 + k[10] * r2 + k[11] * r4;
    // the identity tilt matrix: vecTilt = (1*xd0 + 0*yd0 + 0, 0*xd0 + 1*yd0 + 0, 0*xd0 + 0*yd0 + 1), invProj = 1
    const double t0 = 1. * xd0 + 0. * yd0 + 0., t1 = 0. * xd0 + 1. * yd0 + 0., t2 = 0. * xd0 + 0. * yd0 + 1.;
    const double ip = t2 ? 1. / t2 : 1;
    const double xd = ip * t0, yd = ip * t1;
    *u = (float)(xd * cam.fx + cam.cx);
    *v = (float)(yd * cam.fy + cam.cy);
    const uint32_t bu = ctm::f32_to_bits(*u), bv = ctm::f32_to_bits(*v);
    return (bu & 0x7f800000u) != 0x7f800000u && (bv & 0x7f800000u) != 0x7f800000u;
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_draw_expand(const uint8_t* __restrict__ gray, int n, int rows, int cols, ptrdiff_t row_stride,
                                                     ptrdiff_t frame_stride, uint8_t* __restrict__ out, ptrdiff_t out_row_stride,
                                                     ptrdiff_t out_frame_stride) {
    // one block = 1024 pixels of one row, 4 per thread
    const long long chunks = (cols + 1023) / 1024;
    const long long total = (long long)n * rows * chunks;
    for (long long b = blockIdx.x; b < total; b += gridDim.x) {
        const long long fr = b / (rows * chunks), rem = b % (rows * chunks);
        const int y = (int)(rem / chunks), x0 = (int)(rem % chunks) * 1024 + threadIdx.x * 4;
        const uint8_t* src = gray + fr * frame_stride + (ptrdiff_t)y * row_stride;
        uint8_t* dst = out + fr * out_frame_stride + (ptrdiff_t)y * out_row_stride;
        if (x0 + 4 <= cols && (((uintptr_t)(src + x0)) & 3) == 0 && (((uintptr_t)(dst + 3 * x0)) & 3) == 0) {
            const uint32_t g = *reinterpret_cast<const uint32_t*>(src + x0);
            const uint32_t g0 = g & 0xff, g1 = (g >> 8) & 0xff, g2 = (g >> 16) & 0xff, g3 = g >> 24;
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + 3 * x0);
            d[0] = g0 | (g0 << 8) | (g0 << 16) | (g1 << 24);
            d[1] = g1 | (g1 << 8) | (g2 << 16) | (g2 << 24);
            d[2] = g2 | (g3 << 8) | (g3 << 16) | (g3 << 24);
        } else {
            for (int x = x0; x < x0 + 4 && x < cols; x++) {
                const uint8_t g = src[x];
                dst[3 * x] = g;
                dst[3 * x + 1] = g;
                dst[3 * x + 2] = g;
            }
        }
    }
}

struct RasterArgs {
    const ctag_frame_result* res;
    const int32_t* offsets;
    const ctag_pose_rec* poses;
    int capacity;
    int n;
    int rows, cols;
    uint8_t* out;
    ptrdiff_t out_row_stride, out_frame_stride;
    DrawModel model;
    DrawCam cam;
    int axis_length;
};

__global__ __launch_bounds__(kWave) void k_draw_raster(RasterArgs A) {
    const int f = blockIdx.x;
    const int lane = threadIdx.x;
    if (f >= A.n) return;
    __shared__ int px[kDrawPts], py[kDrawPts], pok[kDrawPts];
    __shared__ int hw5[6], hw8[9];
    if (lane == 0) {
        circle_half_widths(5, hw5);
        circle_half_widths(8, hw8);
    }
    __syncthreads();
    const ctag_frame_result* R = A.res + f;
    const int status = R->status, n_markers = R->n_markers;
    if (status != CTAG_OK || n_markers < 0 || n_markers > CTAG_MAX_MARKERS) return;
    long long lo = A.offsets[f], hi = A.offsets[f + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > A.capacity ? A.capacity : hi;
    const Target t{A.out + (ptrdiff_t)f * A.out_frame_stride, A.out_row_stride, A.cols, A.rows};
    const float L = (float)A.axis_length;
    for (long long k = lo; k < hi; k++) {
        const ctag_pose_rec* P = A.poses + k;
        if (P->status != CTAG_POSE_OK || P->frame != f) continue;
        const int m = P->marker, mi = P->model_index;
        if (m < 0 || m >= n_markers || mi < 0 || mi >= A.model.n_models) continue;
        const ctag_marker_rec M = R->markers[m];
        const int nf = M.n_features, first = M.first_feature;
        if (nf < 0 || nf > CTAG_MAX_CODE_POS || nf > M.n_pos || first < 0 || first + nf > CTAG_MAX_FEATURES) continue;
        bool bad = false;
        for (int j = 0; j < nf; j++) {
            const int pos = R->features[first + j].pos;
            bad |= pos < 0 || pos >= A.model.model_size;
        }
        if (bad) continue;  // the reference reads outside the model there (CTAG_POSE_BAD_POS)
        double Rm[9];
        rodrigues(P->rvec, Rm);
        const int npts = nf * 8 + 4;
        const float* base = A.model.base + 3 * (size_t)mi;
        const float* axis = A.model.axis + 3 * (size_t)mi;
        for (int q = lane; q < npts; q += kWave) {
            float X, Y, Z;
            if (q < nf * 8) {
                const int pos = R->features[first + q / 8].pos;
                const float* c = A.model.corners + (((size_t)mi * A.model.model_size + pos) * 8 + q % 8) * 3;
                X = c[0], Y = c[1], Z = c[2];
            } else {
                // base, base + axis*L, base + (0.0372, 0.0372, 0.9986)*L, base + (0.9980, -0.0520, -0.0353)*L in float
                const int e = q - nf * 8;
                float ex = 0.f, ey = 0.f, ez = 0.f;
                if (e == 1) ex = axis[0] * L, ey = axis[1] * L, ez = axis[2] * L;
                if (e == 2) ex = 0.0372f * L, ey = 0.0372f * L, ez = 0.9986f * L;
                if (e == 3) ex = 0.9980f * L, ey = -0.0520f * L, ez = -0.0353f * L;
                X = e ? base[0] + ex : base[0];
                Y = e ? base[1] + ey : base[1];
                Z = e ? base[2] + ez : base[2];
            }
            float u, v;
            const bool ok = project_point(Rm, P->tvec, A.cam, X, Y, Z, &u, &v);
            px[q] = ok ? round_sat((double)u) : 0;
            py[q] = ok ? round_sat((double)v) : 0;
            pok[q] = ok;
        }
        __syncthreads();
        // circle(imgMark, imagePoints[i], 5, Scalar(255, 234, 32), -1) for i < size - 5
        disks(t, px, py, pok, 0, npts - 5, 5, hw5, Col{255, 234, 32}, lane);
        const int b = npts - 4;
        const Col axc[3] = {{255, 0, 0}, {0, 255, 0}, {0, 0, 255}};
        if (pok[b]) {
            for (int a = 0; a < 3; a++)
                if (pok[b + 1 + a]) arrowed_line(t, px[b], py[b], px[b + 1 + a], py[b + 1 + a], axc[a], lane);
            disks(t, px, py, pok, b, 1, 8, hw8, Col{247, 235, 235}, lane);
        }
        __syncthreads();  // the LDS points are rewritten by the next record
    }
}

struct DrawState {
    DevBuf<uint8_t> d_gray, d_out;
    DevBuf<ctag_frame_result> d_res;
    DevBuf<int32_t> d_offsets;
    DevBuf<ctag_pose_rec> d_poses;
};

void draw_state_free(void* p) { delete static_cast<DrawState*>(p); }

DrawState* draw_state(ctag_handle* h) {
    void** slot = handle_state_slot(h, kDrawState, draw_state_free);
    if (!*slot) *slot = new (std::nothrow) DrawState();
    return static_cast<DrawState*>(*slot);
}

constexpr int kMaxSide = 1 << 15;
constexpr int kMaxAxisLength = 1 << 16;

bool sizes_ok(int rows, int cols, ptrdiff_t row_stride, ptrdiff_t out_row_stride, int axis_length) {
    return rows >= 1 && cols >= 1 && rows <= kMaxSide && cols <= kMaxSide && row_stride >= cols && out_row_stride >= 3 * (ptrdiff_t)cols &&
           axis_length >= 0 && axis_length <= kMaxAxisLength;
}

int enqueue(ctag_handle* h, const uint8_t* frames, int n, int rows, int cols, ptrdiff_t row_stride, ptrdiff_t frame_stride,
            const ctag_frame_result* res, const int32_t* offsets, const ctag_pose_rec* poses, int capacity, ctag_model* model,
            const ctag_camera* camera, int axis_length, uint8_t* out, ptrdiff_t out_row_stride, ptrdiff_t out_frame_stride) {
    const int dev = handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    if (model_to_device(model, dev) != CTAG_OK) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    if (n == 0) return CTAG_OK;
    hipLaunchKernelGGL(k_draw_expand, dim3(4096), dim3(256), 0, s, frames, n, rows, cols, row_stride, frame_stride, out, out_row_stride,
                       out_frame_stride);
    RasterArgs A;
    A.res = res;
    A.offsets = offsets;
    A.poses = poses;
    A.capacity = capacity;
    A.n = n;
    A.rows = rows;
    A.cols = cols;
    A.out = out;
    A.out_row_stride = out_row_stride;
    A.out_frame_stride = out_frame_stride;
    A.model = DrawModel{model->n_models, model->model_size, model->d_corners.p, model->d_base, model->d_axis};
    A.cam.fx = (double)camera->K[0];
    A.cam.fy = (double)camera->K[4];
    A.cam.cx = (double)camera->K[2];
    A.cam.cy = (double)camera->K[5];
    for (int i = 0; i < 12; i++) A.cam.k[i] = i < camera->n_dist ? (double)camera->dist[i] : 0.0;
    A.axis_length = axis_length;
    hipLaunchKernelGGL(k_draw_raster, dim3(n), dim3(kWave), 0, s, A);
    return hipGetLastError() == hipSuccess ? CTAG_OK : CTAG_ERR_HIP;
}

}  // namespace
}  // namespace ctag

extern "C" {

int ctag_draw_axis_batch_device(ctag_handle* h, const uint8_t* frames_dev, int n_frames, int rows, int cols, ptrdiff_t row_stride,
                                ptrdiff_t frame_stride, const ctag_frame_result* results_dev, const int32_t* offsets_dev,
                                const ctag_pose_rec* poses_dev, int capacity, const ctag_model* model, const ctag_camera* camera,
                                int axis_length, uint8_t* out_dev, ptrdiff_t out_row_stride, ptrdiff_t out_frame_stride) {
    if (!h || !model || n_frames < 0 || capacity < 0) return CTAG_ERR_ARG;
    if (!ctag::sizes_ok(rows, cols, row_stride, out_row_stride, axis_length)) return CTAG_ERR_ARG;
    if (n_frames > 0) {
        if (!frames_dev || !results_dev || !offsets_dev || !out_dev || (capacity > 0 && !poses_dev)) return CTAG_ERR_ARG;
        if (n_frames > 1 && (frame_stride < row_stride * (rows - 1) + cols || out_frame_stride < out_row_stride * (rows - 1) + 3 * (ptrdiff_t)cols))
            return CTAG_ERR_ARG;
    }
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    {   // records of frames that wait for the any-frame pass (CTAG_PENDING) are completed before they are read
        const int fr = ctag::handle_finish_pending(h);
        if (fr != CTAG_OK) return fr;
    }
    return ctag::enqueue(h, frames_dev, n_frames, rows, cols, row_stride, frame_stride, results_dev, offsets_dev, poses_dev, capacity,
                         const_cast<ctag_model*>(model), camera, axis_length, out_dev, out_row_stride, out_frame_stride);
}

int ctag_draw_axis(ctag_handle* h, const uint8_t* gray, int rows, int cols, ptrdiff_t row_stride, const ctag_frame_result* result,
                   const ctag_pose_rec* poses, int n_poses, const ctag_model* model, const ctag_camera* camera, int axis_length, uint8_t* out,
                   ptrdiff_t out_row_stride) {
    if (!h || !gray || !result || !model || !out || n_poses < 0 || n_poses > (1 << 20) || (n_poses > 0 && !poses)) return CTAG_ERR_ARG;
    if (!ctag::sizes_ok(rows, cols, row_stride, out_row_stride, axis_length)) return CTAG_ERR_ARG;
    if (!ctag::camera_ok(camera)) return CTAG_ERR_UNSUPPORTED;
    const int dev = ctag::handle_device(h);
    if (hipSetDevice(dev) != hipSuccess) return CTAG_ERR_HIP;
    ctag::DrawState* st = ctag::draw_state(h);
    if (!st) return CTAG_ERR_HIP;
    const size_t gb = (size_t)rows * cols, ob = gb * 3;
    if (st->d_gray.grow(gb) != hipSuccess || st->d_out.grow(ob) != hipSuccess) return CTAG_ERR_HIP;
    if (st->d_res.grow(1) != hipSuccess || st->d_offsets.grow(2) != hipSuccess) return CTAG_ERR_HIP;
    if (n_poses > 0 && st->d_poses.grow((size_t)n_poses) != hipSuccess) return CTAG_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(ctag_stream(h));
    const int32_t off[2] = {0, n_poses};
    if (hipMemcpy2DAsync(st->d_gray.p, cols, gray, row_stride, cols, rows, hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpyAsync(st->d_res.p, result, sizeof(ctag_frame_result), hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    if (hipMemcpyAsync(st->d_offsets.p, off, sizeof(off), hipMemcpyHostToDevice, s) != hipSuccess) return CTAG_ERR_HIP;
    if (n_poses > 0 && hipMemcpyAsync(st->d_poses.p, poses, sizeof(ctag_pose_rec) * (size_t)n_poses, hipMemcpyHostToDevice, s) != hipSuccess)
        return CTAG_ERR_HIP;
    int rc = ctag::enqueue(h, st->d_gray.p, 1, rows, cols, cols, (ptrdiff_t)gb, st->d_res.p, st->d_offsets.p, st->d_poses.p, n_poses,
                           const_cast<ctag_model*>(model), camera, axis_length, st->d_out.p, 3 * (ptrdiff_t)cols, (ptrdiff_t)ob);
    if (rc != CTAG_OK) return rc;
    if (hipMemcpy2DAsync(out, out_row_stride, st->d_out.p, 3 * (size_t)cols, 3 * (size_t)cols, rows, hipMemcpyDeviceToHost, s) != hipSuccess)
        return CTAG_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return CTAG_ERR_HIP;
    return CTAG_OK;
}

}  // extern "C"
