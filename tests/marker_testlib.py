"""An independent Python statement of the stages behind edgeExtraction that work on quads, features and markers:
a5 `featureRecovery` + `featureOrganization` (reference `corner_detector.cpp:465-559`, `:571-598`), a6 `cornerObtain` (`:561-569`),
a8 `markerOrganization` (`:976-1052`), a9 `featureExtraction` (`:1054-1209`) and a10 `markerDecoder` + `match_dictionary`
(`:1211-1324`), with the flow of `CylinderTag::detect` (`CylinderTag.cpp:87-128`) between them.

It is written from the reference text, `header/corner_detector.h` (member types and constants) and SURVEY App. A (A.7: the 2 x 2
`determinant` / `solve`, A.8: `fastAtan2`) and App. B only; `oracle/ctag_oracle.cpp` and `k_feature.hip`, which it is compared with,
were not read while it was written.  The record layouts are those of `include/ctag_types.h`.

Each stage is a function of the previous stage's output:
  recover_features(quads) -> features0        obtain_corners(features0) -> features1
  organize_markers(features2, params) -> premarkers        decode_markers(premarkers, state, feature_size) -> result

Two modes:
  "ref"  the reference's types: float32 wherever it stores or computes a `float` (`using namespace std` gives `atan2`, `sqrt`,
         `abs` of floats their float overloads; `x * 180 / CV_PI` is a float product divided in double), double where it
         computes in double.  A float operation is written r(a op b) on doubles that hold float32 values: for + - * / sqrt the
         second rounding from 53 to 24 bits is innocuous.  atan2f comes from MATH (see use_shared_math);
  "f64"  every real quantity in float64 with numpy / libm functions; fastAtan2 keeps its polynomial (it defines the function).

Every thresholded comparison leaves a margin in the stage's Trace: |value - threshold| over the magnitude of the terms.  Ties
under `std::sort` (:1035-1047) are unspecified: the statement sorts stably and reports margin 0.  Undefined behaviour follows SURVEY
App. B (B3, B4, B5, B6, B9, B13, B15, B16, B17), cited in place.
"""
import math

import numpy as np

import edge_testlib as et
from ctag_testlib import FEATURE_DT, MARKER_DT, MAX_FEATURES, MAX_MARKERS, RESULT_DT

F32 = np.float32
CV_PI = 3.1415926535897932384626433832795
MAX_QUADS, MAX_CODE_POS = 1000, 20             # isVisited[1000], code[20] (header/corner_detector.h:124,152)
FLAG_QUAD_OVERFLOW, FLAG_FEATURE_OVERFLOW, FLAG_CODE_OVERFLOW = 1, 2, 4
OK, NO_CORNER, NO_FEATURE, ERR_LIMIT = 0, 1, 2, -3

FEATURE_DT64 = np.dtype([(n, "<f8" if FEATURE_DT[n].base == np.dtype("<f4") else "<i4", FEATURE_DT[n].shape) for n in FEATURE_DT.names])
RESULT_DT64 = np.dtype([("status", "<i4"), ("n_markers", "<i4"), ("n_features", "<i4"), ("flags", "<u4"),
                        ("markers", MARKER_DT, (MAX_MARKERS,)), ("features", FEATURE_DT64, (MAX_FEATURES,))])

DEFAULT_PARAMS = dict(threshold_angle=5.0, threshold_vertical=0.5,          # header/corner_detector.h:122,144
                      ID_cr_correspond=(1.47, 1.54, 1.61, 1.68),            # :135
                      cr_covariance_left=(0.1, 0.035, 0.035, 0.035),        # :136
                      cr_covariance_right=(0.035, 0.035, 0.035, 0.1))       # :137


class _NumpyMath:
    @staticmethod
    def atan2f(y, x):
        return np.arctan2(np.asarray(y, np.float32), np.asarray(x, np.float32))

    @staticmethod
    def cosf(a):
        return np.cos(np.asarray(a, np.float32))

    @staticmethod
    def sinf(a):
        return np.sin(np.asarray(a, np.float32))


class SharedMath(et.SharedMath):
    """edge_testlib's SharedMath (the project's float exp) with the float atan2 / cos / sin the project ships for both of its
    implementations, reached through the oracle library's math probe.  They are definitions of libm functions,
    not readings of a stage."""

    def _call(self, op, a, b=None):
        a = np.asarray(a, np.float32)
        b64 = None if b is None else np.asarray(b, np.float32).astype(np.float64).ravel()
        return self.oracle.math(op, a.astype(np.float64).ravel(), b64).astype(np.float32).reshape(a.shape)

    def atan2f(self, y, x):
        y, x = np.broadcast_arrays(np.asarray(y, np.float32), np.asarray(x, np.float32))
        return self._call(5, y, x)

    def cosf(self, a):
        return self._call(7, a)

    def sinf(self, a):
        return self._call(6, a)


MATH = _NumpyMath()


def use_shared_math(oracle):
    """Route "ref" mode's float transcendentals, here and in edge_testlib, through the project's shared math: one object for both."""
    global MATH
    MATH = et.MATH = SharedMath(oracle)


class Trace:
    """What one stage call met: the smallest margin (per item where the stage has items), and counters of the branches taken."""

    def __init__(self):
        self.margin, self.site = math.inf, ""
        self.item_margin = {}      # item index -> smallest margin of the comparisons that decided that item
        self.count = {}
        self.resolution = {}       # a7: feature -> how far float32 line directions can move one of its corners (refine_testlib)
        self.slot_feature = []     # a8: the input feature behind each feature slot of the premarkers record
        self.outcome = {}          # a10: premarker -> (isGood, ID, inverse, pos) or "short" / "overflow"

    def note(self, site, value, threshold, scale, item=None):
        m = abs(float(value) - float(threshold)) / max(float(scale), 1e-30)
        if m < self.margin:
            self.margin, self.site = m, site
        for it in (() if item is None else item if isinstance(item, tuple) else (item,)):  # a comparison between two items counts for both
            if m < self.item_margin.get(it, math.inf):
                self.item_margin[it] = m

    def hit(self, tag, n=1):
        self.count[tag] = self.count.get(tag, 0) + n


class _Ar:
    """The float arithmetic of one mode."""

    def __init__(self, mode):
        assert mode in ("ref", "f64")
        self.f64 = mode == "f64"
        self.dt = np.float64 if self.f64 else np.float32

    def r(self, v):
        return float(v) if self.f64 else float(F32(v))

    def atan2_deg(self, y, x):
        """`atan2(y, x) * 180 / CV_PI` of float arguments (arrays of self.dt): atan2f, a float product, a double quotient."""
        if self.f64:
            return np.arctan2(y, x) * 180 / CV_PI
        return (MATH.atan2f(y, x) * F32(180)).astype(np.float64) / CV_PI

    def dist(self, ax, ay, bx, by):
        """distance_2points (:1252-1254), all float."""
        r = self.r
        dx, dy = r(ax - bx), r(ay - by)
        return r(math.sqrt(r(r(dx * dx) + r(dy * dy))))

    def fast_atan2(self, y, x):
        """cv::fastAtan2, degrees in [0, 360)."""
        r = self.r
        scale = r(180 / CV_PI)  # (float)(180 / CV_PI); the coefficients are float products
        p1, p3, p5, p7 = (r(r(c) * scale) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
        ax, ay = abs(x), abs(y)
        eps = r(2.220446049250313e-16)
        if ax >= ay:
            c = r(ay / r(ax + eps))
        else:
            c = r(ax / r(ay + eps))
        c2 = r(c * c)
        a = r(r(r(r(r(r(r(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
        if ay > ax:
            a = r(90 - a)
        if x < 0:
            a = r(180 - a)
        if y < 0:
            a = r(360 - a)
        return a

    def solve2(self, a00, a01, a10, a11, b0, b1):
        """determinant(A) != 0 -> solve(A, B) of 2 x 2 CV_32F: double products, multiplied by 1 / det, stored as float.
        None when the determinant is exactly 0."""
        det = a00 * a11 - a01 * a10
        if det == 0:
            return None
        d = 1.0 / det
        return self.r((b0 * a11 - b1 * a01) * d), self.r((b1 * a00 - b0 * a10) * d)


# ------------------------------------------------------------------------------------------------ a5

def _gate(ar, fa, ca, t):
    """:490 and its three sisters on arrays: |d| < t || ||d| - 180| < t || ||d| - 360| < t, all float.  Returns (pass, margin)."""
    dt = ar.dt
    d = np.abs(fa - ca)
    v = np.stack([d, np.abs(d - dt(180)), np.abs(d - dt(360))])
    return (v < dt(t)).any(0), (np.abs(v.astype(np.float64) - t) / 360.0).min(0)


def recover_features(quads, mode, params=None, trace=None):
    """a5: (nq, 8) quads in half-size coordinates -> (nf, 19) features (16 corner coordinates, centre, feature_angle), and
    the (nf, 4) integers quad i, quad j, pos_quad1, pos_quad2 of each."""
    P = dict(DEFAULT_PARAMS, **(params or {}))
    ar, tr = _Ar(mode), trace if trace is not None else Trace()
    r, dt = ar.r, ar.dt
    T = ar.r(P["threshold_angle"])
    q = np.asarray(quads, dt).reshape(-1, 4, 2)
    n = len(q)
    feats, pairs = [], []
    if n == 0 or n > MAX_QUADS:  # B13: nothing to pair; B6: isVisited[1000]
        return np.zeros((0, 19), dt), np.zeros((0, 4), np.int32)
    x, y = q[:, :, 0], q[:, :, 1]
    cx = (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) / dt(4)  # :474
    cy = (((y[:, 0] + y[:, 1]) + y[:, 2]) + y[:, 3]) / dt(4)
    nx_, ny_ = np.roll(x, -1, 1), np.roll(y, -1, 1)
    cd = np.sqrt((x - nx_) * (x - nx_) + (y - ny_) * (y - ny_))  # :477, float
    deg = lambda a, b: ar.atan2_deg(y[:, a] - y[:, b], x[:, a] - x[:, b])  # noqa: E731
    d01, d32, d12, d03, d23 = deg(0, 1), deg(3, 2), deg(1, 2), deg(0, 3), deg(2, 3)
    ca1 = ((d01 + d32) / 2).astype(dt)  # :479-480: double sums stored in vector<float>
    ca2 = ((d12 + d03) / 2).astype(dt)
    e01, e12, e03, e23 = (a.astype(dt) for a in (d01, d12, d03, d23))  # the float member edge_angle1/2
    fa = ar.atan2_deg(cy[:, None] - cy[None, :], cx[:, None] - cx[None, :]).astype(dt)  # :488, the float member feature_angle
    g1a, m1a = _gate(ar, fa, ca1[:, None], T)
    g1b, m1b = _gate(ar, fa, ca2[:, None], T)
    g2a, m2a = _gate(ar, fa, ca1[None, :], T)
    g2b, m2b = _gate(ar, fa, ca2[None, :], T)
    gm = np.minimum(np.minimum(m1a, m1b), np.minimum(m2a, m2b))
    both = (g1a | g1b) & (g2a | g2b)
    visited = np.zeros(n, bool)

    def side(k, first, second, tr):
        """The dist_long, dist_short and edge_angle the two blocks leave for quad k: the second block overrides the first."""
        out = None
        if first:  # :491-501
            dl, ds = r(r(cd[k, 0] + cd[k, 2]) / 2), min(float(cd[k, 1]), float(cd[k, 3]))
            out = dl, ds, float(e03[k]) if cd[k, 1] < cd[k, 3] else float(e12[k])
            tr.note("a5.side13", cd[k, 1], cd[k, 3], cd[k, 1] + cd[k, 3], k)
        if second:  # :504-514
            ds, dl = min(float(cd[k, 0]), float(cd[k, 2])), r(r(cd[k, 1] + cd[k, 3]) / 2)
            out = dl, ds, float(e01[k]) if cd[k, 0] > cd[k, 2] else float(e23[k])
            tr.note("a5.side02", cd[k, 0], cd[k, 2], cd[k, 0] + cd[k, 2], k)
        return out

    def judge(i, j, tr):
        """The six clauses of :543-548 for a pair that passed the angle gates."""
        d1l, d1s, ea1 = side(i, g1a[i, j], g1b[i, j], tr)
        d2l, d2s, ea2 = side(j, g2a[i, j], g2b[i, j], tr)
        fl = ar.dist(cx[i], cy[i], cx[j], cy[j])  # :542
        de = abs(r(ea1 - ea2))
        T10 = r(T * 10)
        ev = [de, abs(r(de - 180)), abs(r(de - 360))]
        sl, ss = r(d1l + d2l), r(d1s + d2s)
        half = r(sl / 2)
        clauses = [d1l > d1s or d2l > d2s,                                   # :543
                   any(v < T10 for v in ev),                                # :544
                   abs(r(d1s - d2s)) < min(d1s, d2s) * 0.33,                # :545 (double)
                   sl > ss,                                                 # :546
                   sl < r(15 * ss),                                         # :547
                   r(fl - half) < 0.3 * r(fl + half)]                       # :548 (double)
        both_ = (i, j)
        tr.note("a5.long_short_1", d1l, d1s, d1l + d1s, both_)
        tr.note("a5.long_short_2", d2l, d2s, d2l + d2s, both_)
        tr.note("a5.edge_angle", min(abs(v - T10) for v in ev), 0, 360, both_)
        tr.note("a5.short_ratio", abs(r(d1s - d2s)), min(d1s, d2s) * 0.33, d1s + d2s, both_)
        tr.note("a5.long_gt_short", sl, ss, sl + ss, both_)
        tr.note("a5.long_lt_15", sl, r(15 * ss), sl + 15 * ss, both_)
        tr.note("a5.length", r(fl - half), 0.3 * r(fl + half), fl + half, both_)
        return clauses

    for i in range(n - 1):
        if visited[i]:
            continue
        for j in range(i + 1, n):
            if visited[j]:
                continue
            tr.note("a5.gate", gm[i, j], 0.0, 1.0, (i, j))
            if not both[i, j]:
                continue
            clauses = judge(i, j, tr)
            if sum(clauses) == 5:
                tr.hit("a5.only_clause_%d_fails" % clauses.index(False))
            if not all(clauses):
                tr.hit("a5.tagged_pair_rejected")
                continue
            visited[i] = visited[j] = True
            # the first match wins (:553): a later quad that is still free and would pass every clause with i is never asked
            if any(both[i, k] and not visited[k] and all(judge(i, k, Trace())) for k in range(j + 1, n)):
                tr.hit("a5.first_match_wins")
            f, p1, p2 = _organize_feature(ar, tr, q[i], q[j], (cx[i], cy[i]), (cx[j], cy[j]), float(fa[i, j]), (i, j))
            feats.append(f)
            pairs.append((i, j, p1, p2))
            break  # :553
    return np.array(feats, dt).reshape(-1, 19), np.array(pairs, np.int32).reshape(-1, 4)


def _organize_feature(ar, tr, q1, q2, c1, c2, fa, item=None):
    """featureOrganization (:571-598): rotate both quads so that corners 0, 1 and 4, 5 are the far long edges."""
    r = ar.r
    a1 = ar.atan2_deg(c1[1] - q1[:, 1], c1[0] - q1[:, 0]).astype(ar.dt)  # :577-578, float arrays
    a2 = ar.atan2_deg(c2[1] - q2[:, 1], c2[0] - q2[:, 0]).astype(ar.dt)

    def fold(a):  # min(360 - |a - fa|, |a - fa|), float
        d = abs(r(float(a) - fa))
        return min(r(360 - d), d)

    s1 = [r(fold(a1[(i + 2) % 4]) + fold(a1[(i + 3) % 4])) for i in range(4)]
    s2 = [r(fold(a2[(i + 2) % 4]) + fold(a2[(i + 3) % 4])) for i in range(4)]
    amin, amax, p1, p2 = 360.0, 0.0, -1, -1
    for i in range(4):  # :580-589: strict comparisons, the first extreme wins
        if s1[i] < amin:
            amin, p1 = s1[i], i
        if s2[i] > amax:
            amax, p2 = s2[i], i
    assert p1 >= 0 and p2 >= 0  # (-1 would index before the quad: sums of exactly 360 / 0 on all four rotations)
    tr.note("a5.rotation1", sorted(s1)[1], sorted(s1)[0], 360, item)
    tr.note("a5.rotation2", sorted(s2)[-2], sorted(s2)[-1], 360, item)
    c = np.concatenate([np.roll(q1, -p1, 0), np.roll(q2, -p2, 0)])  # :590-595
    fx = r(r(r(r(c[0, 0] + c[1, 0]) + c[4, 0]) + c[5, 0]) / 4)  # :596
    fy = r(r(r(r(c[0, 1] + c[1, 1]) + c[4, 1]) + c[5, 1]) / 4)
    return list(c.reshape(-1)) + [fx, fy, fa], p1, p2


# ------------------------------------------------------------------------------------------------ a6

def obtain_corners(features0, mode):
    """a6 (:561-569): corners to full-size coordinates, (c - 0.5) * 2 + 0.5 in float, and the centre from corners 0, 1, 4, 5."""
    dt = _Ar(mode).dt
    f = np.array(features0, dt).reshape(-1, 19)
    c = (f[:, :16] - dt(0.5)) * dt(2) + dt(0.5)
    f[:, :16] = c
    for k in (0, 1):  # Point2f sums left to right, then / 4
        f[:, 16 + k] = (((c[:, 0 + k] + c[:, 2 + k]) + c[:, 8 + k]) + c[:, 10 + k]) / dt(4)
    return f


# ------------------------------------------------------------------------------------------------ a8 + a9

def _empty_result(mode, status=OK, flags=0):
    res = np.zeros(1, RESULT_DT64 if mode == "f64" else RESULT_DT)[0]
    res["status"], res["flags"] = status, flags  # (unused marker and feature slots stay zero)
    return res


def organize_markers(features2, mode, params=None, trace=None, feature_size=0):
    """a8 + a9: (nf, 19) features -> the markers before decoding as a ctag_frame_result record (marker_id -1, pos -1, n_pos 0).
    Fewer features than `feature_size` is the early return of CylinderTag.cpp:93-96."""
    P = dict(DEFAULT_PARAMS, **(params or {}))
    ar, tr = _Ar(mode), trace if trace is not None else Trace()
    r = ar.r
    f = np.asarray(features2, ar.dt).reshape(-1, 19).astype(np.float64)
    n = len(f)
    if n < feature_size or n == 0:
        return _empty_result(mode, NO_FEATURE)
    if n > MAX_FEATURES:  # B6: father[100]
        return _empty_result(mode, ERR_LIMIT, FLAG_FEATURE_OVERFLOW)
    if n >= 65:
        tr.hit("a8.features_65")
    T, TV = r(P["threshold_angle"]), r(P["threshold_vertical"])
    C = f[:, :16].reshape(n, 8, 2)
    cen, ang = f[:, 16:18], f[:, 18]
    father = list(range(n))

    def find(k):  # union_find (:1256-1258), with its path compression
        if father[k] != k:
            father[k] = find(father[k])
        return father[k]

    for i in range(n - 1):
        for j in range(i + 1, n):
            vcx, vcy = r(cen[i, 0] - cen[j, 0]), r(cen[i, 1] - cen[j, 1])  # :982
            vlx, vly = r(C[i, 0, 0] - C[i, 5, 0]), r(C[i, 0, 1] - C[i, 5, 1])  # :983
            num = r(r(vcx * vlx) + r(vcy * vly))
            den2 = r(r(r(vcx * vcx) + r(vcy * vcy)) * r(r(vlx * vlx) + r(vly * vly)))
            cang = r(num / r(math.sqrt(den2))) if den2 > 0 else math.nan  # :984, float
            da = abs(r(ang[i] - ang[j]))
            dc, dl = ar.dist(cen[i, 0], cen[i, 1], cen[j, 0], cen[j, 1]), ar.dist(C[i, 0, 0], C[i, 0, 1], C[i, 5, 0], C[i, 5, 1])
            both_ = (i, j)
            tr.note("a8.angle_2T", da, r(T * 2), 360, both_)
            tr.note("a8.angle_180", abs(r(180 - da)), T, 360, both_)
            tr.note("a8.distance", dc, 0.3 * dl, dc + dl, both_)
            if not math.isnan(cang):
                tr.note("a8.vertical", abs(cang), TV, 1.0, both_)
            near, anti = da < r(T * 2), abs(r(180 - da)) < T  # :985: threshold_angle * 2 on one side of the ||, threshold_angle on the other
            rest = dc < 0.3 * dl and abs(cang) < TV
            if rest and anti and not near:
                tr.hit("a8.joined_by_180_clause_only")
            if rest and not anti and not near and abs(r(180 - da)) < r(T * 2):
                tr.hit("a8.180_clause_between_T_and_2T")
            if (near or anti) and rest:
                fi, fj = find(i), find(j)
                if fi != fj:
                    father[fj] = fi
    # :993-1019, literally: father[0] is taken as it stands, the others are resolved to their roots
    database, members = [father[0]], [[0]]
    if father[0] != find(0):
        tr.hit("a8.father_chain")
    for i in range(1, n):
        now = father[i]
        while now != father[now]:
            now = find(now)
        father[i] = now
    for i in range(1, n):
        if father[i] in database:
            members[database.index(father[i])].append(i)
        else:
            database.append(father[i])
            members.append([i])
    res = _empty_result(mode)
    ids = [0, 0]  # B3: ID_left / ID_right persist from feature to feature; 0 at the entry of detect()
    k = 0
    for mi, mem in enumerate(members):
        el, ma = [], 0.0
        for j in mem:
            c = C[j]
            el.append(r(ar.dist(c[0, 0], c[0, 1], c[1, 0], c[1, 1]) + r(ar.dist(c[4, 0], c[4, 1], c[5, 0], c[5, 1]) / 2)))  # :1027, B5
            a = ar.fast_atan2(r(c[0, 1] - c[5, 1]), r(c[0, 0] - c[5, 0]))  # :1028
            tr.note("a8.angle_now_180", a, 180, 360, tuple(mem))
            if a > 180:
                a -= 180
            ma = r(ma + a)  # the float member marker_angle += double
        ma = r(ma / r(len(mem)))  # :1032
        tr.note("a8.direction_45", abs(ma), 45, 180, tuple(mem))
        tr.note("a8.direction_135", abs(ma), 135, 180, tuple(mem))
        direction = 0 if (abs(ma) < 45 or abs(ma) > 135) else 1  # :1034
        key = [-cen[j, 1] for j in mem] if direction == 0 else [cen[j, 0] for j in mem]  # :1036 a.y > b.y, :1044 a.x < b.x
        order = sorted(range(len(mem)), key=lambda t: key[t])  # stable
        if len(set(key)) < len(key):
            tr.note("a8.sort_tie", 0, 0, 1, tuple(mem))  # std::sort leaves the order of equal keys unspecified
        tr.hit("a8.direction_%d_%s" % (direction, "low" if ma < 45 else "mid" if ma <= 135 else "high"))
        res["markers"][mi] = (-1, k, len(mem), 0)
        for t in order:
            rec = res["features"][k]
            tr.slot_feature.append(mem[t])
            _extract_feature(ar, tr, P, C[mem[t]].copy(), direction, ids, rec, mem[t], first_of_marker=(t == order[0]), first=(k == 0))
            rec["center"], rec["edge_length"], rec["pos"] = cen[mem[t]], el[t], -1
            k += 1
    res["n_markers"], res["n_features"] = len(members), n
    return res


def _extract_feature(ar, tr, P, c, direction, ids, rec, item, first_of_marker, first):
    """a9, one feature of featureExtraction (:1056-1208).  marker_dst and marker_src are the same object (:1040, :1048), so the
    swap of :1058-1063 is seen by everything after it."""
    r, d = ar.r, ar.dist
    if not direction:
        tr.note("a9.swap", c[0, 0], c[4, 0], abs(c[0, 0]) + abs(c[4, 0]), item)
        if c[0, 0] > c[4, 0]:
            c = np.concatenate([c[4:], c[:4]])
            tr.hit("a9.swapped")
    L = lambda a, b: d(c[a, 0], c[a, 1], c[b, 0], c[b, 1])  # noqa: E731
    l1 = [L(0, 3), L(3, 6), L(6, 5), L(0, 5)]  # :1066-1073
    l2 = [L(1, 2), L(2, 7), L(7, 4), L(1, 4)]
    cr = lambda l: r(r(r(l[0] + l[1]) * r(l[2] + l[1])) / r(l[1] * l[3]))  # noqa: E731  :1075-1076
    crl, crr = cr(l1), cr(l2)

    def line(a, b, p):  # a Point3f line: x = a.y - b.y, y = b.x - a.x, z = -x * p.x - y * p.y
        lx, ly = r(c[a, 1] - c[b, 1]), r(c[b, 0] - c[a, 0])
        return lx, ly, r(r(-lx * c[p, 0]) - r(ly * c[p, 1]))

    line1, line2 = line(5, 4, 5), line(0, 1, 0)                # :1080-1085
    cross1, cross2 = line(0, 4, 0), line(5, 1, 5)              # :1087-1092
    left, right = line(5, 0, 5), line(1, 4, 1)                 # :1094-1099

    def meet(a, b, what):  # B9: a point left unset by a zero determinant is (0, 0)
        s = ar.solve2(a[0], a[1], b[0], b[1], -a[2], -b[2])
        if s is None:
            tr.hit("a9.zero_determinant_" + what)
        return s if s is not None else (0.0, 0.0)

    vanish, middle = meet(line1, line2, "vanish"), meet(cross1, cross2, "middle")
    mlx, mly = r(middle[1] - vanish[1]), r(vanish[0] - middle[0])  # :1128-1130
    mline = (mlx, mly, r(r(-mlx * middle[0]) - r(mly * middle[1])))
    ml = meet(mline, left, "left")
    meet(mline, right, "right")  # middle_right: computed (:1144-1154) and never used (B4)
    D = lambda k: d(ml[0], ml[1], c[k, 0], c[k, 1])  # noqa: E731
    tables = [[ar.r(v) for v in P[k]] for k in ("ID_cr_correspond", "cr_covariance_left", "cr_covariance_right")]
    for s, (crv, ks) in enumerate(((crl, (0, 3, 5, 6)), (crr, (1, 2, 4, 7)))):  # :1157-1189; B4: the right side measures from middle_left too
        d1, d2, d3, d4 = (D(k) for k in ks)
        a, b = r(d2 * d3), r(d1 * d4)
        is_long = a < b
        tr.note("a9.long_%d" % s, a, b, a + b, item)
        found = False
        for j in range(4):
            idc, cl, crr_ = tables[0][j], tables[1][j], tables[2][j]
            tr.note("a9.interval_low_%d" % s, r(idc - crv), cl, idc, item)
            tr.note("a9.interval_high_%d" % s, r(crv - idc), crr_, idc, item)
            tr.note("a9.interval_side_%d" % s, idc, crv, idc, item)
            if (idc >= crv and r(idc - crv) < cl) or (idc < crv and r(crv - idc) < crr_):
                ids[s] = 7 - j if is_long else j
                found = True
        if not found:  # B3: the member keeps the value an earlier feature left
            tr.hit("a9.carry_first_of_frame" if first else "a9.carry_first_of_marker" if first_of_marker else "a9.carry_inside_marker")
    gap_bad = abs(r(l1[1] - l2[1])) > 0.05 * r(l1[1] + l2[1])  # :1194, float against double
    tr.note("a9.gap_lengths", abs(r(l1[1] - l2[1])), 0.05 * r(l1[1] + l2[1]), l1[1] + l2[1], item)
    rec["corners"] = c.reshape(-1)
    rec["cr_left"], rec["cr_right"] = crl, crr
    if gap_bad:
        rec["id"], rec["id_left"], rec["id_right"] = -2, -1, -1
        tr.hit("a9.id_minus_2")
    else:
        rec["id"], rec["id_left"], rec["id_right"] = ids[0] * 8 + ids[1], ids[0], ids[1]


# ------------------------------------------------------------------------------------------------ a10

def _cdiv(a, b):
    """C integer division and remainder: the quotient truncates toward zero, the remainder has the dividend's sign."""
    q = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)
    return q, a - q * b


def match_dictionary(code, state, length, legal_bits, tr=None):
    """:1269-1324.  Returns (isGood, ID, inverse, pos)."""
    tr = tr if tr is not None else Trace()
    rows, cols = state.shape
    flat = state.reshape(-1)

    def at(i, col):  # state.at<int>(i, col); the C remainder of :1299 can leave the column negative
        if col < 0:  # reached by a code longer than the dictionary is wide: SURVEY B15, a negative column never matches
            tr.hit("a10.negative_column")
            return None
        return int(flat[i * cols + col])
    best, second, where, direc = -1, -1, None, 0
    for sign in (1, -1):
        for i in range(rows):
            for j in range(cols):
                cov = 0
                for k in range(length + 1):
                    if sign == 1:
                        cov += at(i, (j + k) % cols) == code[k]  # :1281
                    else:
                        q, rem = _cdiv(code[k], 8)
                        cov += at(i, _cdiv(j - k + cols, cols)[1]) == (7 - q) + (7 - rem) * 8  # :1299
                if cov > best:
                    best, where, direc = cov, (i, j), sign
                elif cov > second:  # only when the maximum did not move (:1290, :1308)
                    second = cov
    need = min(0.8 * legal_bits, legal_bits - 1.0)
    if best >= need and best == second:
        tr.hit("a10.rejected_by_coverage_tie")  # enough coverage, and a second place with as much
    if best >= need and best > second:  # :1313
        if best == need:
            tr.hit("a10.accepted_at_exact_coverage")
        pos = [_cdiv(where[1] + direc * i + cols, cols)[1] for i in range(length + 1) if code[i] != -1]  # :1317-1321
        return True, where[0], direc == -1, pos
    return False, -1, False, []


def decode_markers(premarkers, state, feature_size, mode, trace=None):
    """a10 (:1211-1250): the markers of a premarkers record that the dictionary accepts, as a result record."""
    ar, tr = _Ar(mode), trace if trace is not None else Trace()
    r = ar.r
    state = np.asarray(state, np.int32)
    res = _empty_result(mode, int(premarkers["status"]), int(premarkers["flags"]))
    if premarkers["status"] != OK:
        return res
    nm = nf = 0
    for mi in range(int(premarkers["n_markers"])):
        m = premarkers["markers"][mi]
        n = int(m["n_features"])
        if n < feature_size:  # :1215
            tr.hit("a10.short_marker")
            tr.outcome[mi] = "short"
            continue
        F = premarkers["features"][int(m["first_feature"]):int(m["first_feature"]) + n]
        code = [-1] * MAX_CODE_POS
        pos, overflow = 0, False
        code[0] = int(F["id"][0])
        for j in range(1, n):
            dist = ar.dist(F["center"][j][0], F["center"][j][1], F["center"][j - 1][0], F["center"][j - 1][1])
            q = r(dist / r(r(r(float(F["edge_length"][j]) + float(F["edge_length"][j - 1])) * 3) / 4))  # :1224, float
            gap = int(math.floor(abs(q) + 0.5) * (1 if q >= 0 else -1))  # roundf: halves away from zero
            tr.note("a10.gap_round", abs(q) - math.floor(abs(q)), 0.5, max(abs(q), 1.0), item=mi)
            tr.hit("a10.gap_%s" % (gap if gap < 3 else "3+"))
            pos += gap
            if pos >= MAX_CODE_POS:  # B6: code[20]; the marker is dropped and the frame flagged
                overflow = True
                break
            code[pos] = int(F["id"][j])
        if overflow:
            res["flags"] |= FLAG_CODE_OVERFLOW
            tr.hit("a10.code_overflow")
            tr.outcome[mi] = "overflow"
            continue
        legal = sum(c > -1 for c in code)
        if any(c == -2 for c in code[:pos + 1]):
            tr.hit("a10.minus_2_in_code")
        good, ident, inverse, where = match_dictionary(code, state, pos, legal, tr)
        tr.outcome[mi] = (good, ident, inverse, tuple(where))
        if not good:
            tr.hit("a10.rejected")
            continue
        tr.hit("a10.accepted_inverse" if inverse else "a10.accepted")
        filled = [i for i in range(pos + 1) if code[i] != -1]
        if len(filled) > 1 and max(np.diff(filled)) > 1:
            tr.hit("a10.accepted_with_gap_%d" % min(max(np.diff(filled)), 3))
        res["markers"][nm] = (ident, nf, n, len(where))
        out = res["features"][nf:nf + n]
        for name in FEATURE_DT.names:
            if name != "pos":
                out[name] = F[name]
        if inverse:  # :1239-1246
            cc = np.array(F["corners"]).reshape(n, 2, 8)
            out["corners"] = cc[:, ::-1].reshape(n, 16)
        out["pos"] = -1
        out["pos"][:len(where)] = where
        nm, nf = nm + 1, nf + n
    res["n_markers"], res["n_features"] = nm, nf
    return res


# ------------------------------------------------------------------------------------------------ comparing records

INT_FIELDS = ("pos", "id", "id_left", "id_right")
REAL_FIELDS = ("corners", "center", "edge_length", "cr_left", "cr_right")


def record_integers(res):
    """Every integer of a record, as one comparable tuple."""
    nm, nf = int(res["n_markers"]), int(res["n_features"])
    return (int(res["status"]), nm, nf, int(res["flags"]), res["markers"][:nm].tolist(),
            [res["features"][k][:nf].tolist() for k in INT_FIELDS])


def record_reals(res):
    """(n_features, 21): 16 corner coordinates, the centre, edge_length, then the two cross ratios."""
    nf = int(res["n_features"])
    return np.concatenate([np.asarray(res["features"][k][:nf], np.float64).reshape(nf, w) for k, w in zip(REAL_FIELDS, (16, 2, 1, 1, 1))], 1)
