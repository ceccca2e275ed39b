/* ctag_testkit.h -- C ABI of libctag_testkit.so: TEST AND BENCH SCAFFOLDING, not part of the product.
 *
 * Nothing here replaces an interface of the reference (/root/reference/header/CylinderTag.h:15-30 is covered by
 * include/ctag.h alone); a host that links libctag_hip.so never needs this library.  It holds what the parity tests,
 * bench.py and the developer tools need around the product:
 *   - parity probes: the intermediates of a frame of the last chunk (stages a1..a8 of SURVEY.md 8(a)),
 *   - the shared deterministic math (cylindertag_amd/csrc/ctag_math.h) evaluated on the device,
 *   - one wave primitive of cylindertag_amd/csrc/ctag_wave.h at a time, under caller-given lane masks,
 *   - the synthetic frame generators,
 *   - the unpack half of ctag_gather_end on a caller-built gathered buffer (the multi-rank device path on one GPU).
 * libctag_testkit.so links against libctag_hip.so and reaches into a handle only through the private accessors of
 * cylindertag_amd/csrc/ctag_internal.h.
 */
#ifndef CTAG_TESTKIT_H
#define CTAG_TESTKIT_H
#include <stddef.h>
#include <stdint.h>

#include "ctag.h"
#include "ctag_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- parity probes: intermediates of frame `frame` of the last chunk -------------------------------------- */
#define CTAG_DBG_HALF 1       /* uint8  [hrows*hcols]   half-resolution image (a1) */
#define CTAG_DBG_LABELS 2     /* int32  [hrows*hcols]   0 = background, else 1 + frame-local root id (a2,a3) */
#define CTAG_DBG_CANDIDATES 3 /* int32  [ncand*8]       area, x_min, y_min, x_max, y_max, has_quad, n_boundary, root */
#define CTAG_DBG_CAND_QUADS 4 /* float  [ncand*8] */
#define CTAG_DBG_FEATURES0 5  /* float  [nfeat*19]      after featureRecovery (half-res) */
#define CTAG_DBG_FEATURES1 6  /* float  [nfeat*19]      after cornerObtain */
#define CTAG_DBG_FEATURES2 7  /* float  [nfeat*19]      after edgeRefine */
#define CTAG_DBG_PREMARKERS 8 /* ctag_frame_result      markers before decoding (needs CTAG_OPT_KEEP_PREMARKERS) */
#define CTAG_DBG_GRAY 9       /* uint8  [rows*cols]     gray image the BGR entry points computed (ctag_detect_batch_bgr8...) */
#define CTAG_DBG_MASK 11      /* uint8  [hrows*hcols]   0 / 1: the adaptive-threshold mask of the fused sweep (k_decimate_mask); -1 when the last chunk took the two-kernel form */
#define CTAG_DBG_LINES 10     /* int32  [nlines]        point count of every edge cluster handed to the Welsch fit (a4) */
#define CTAG_DBG_LINE_POINTS 12 /* int32 [sum n][2]       x, y of those clusters' points, cluster after cluster in the order of CTAG_DBG_LINES */
#define CTAG_DBG_LINE_FITS 13   /* float [nlines][4]      vx, vy, x0, y0 the Welsch fit gave every one of them */
#define CTAG_DBG_PACKS 14       /* int32 [5 + np1 + np2 + nc + nel + nc]  the packed boundary kernels' work lists of a frame of a batch: nc candidates, np1 packs of the first
                                 * kernel, oversize components, np2 packs of the second kernel, nel components in those; then the np1 and the np2 pack words
                                 * (first entry of the order | count << 24), the first kernel's order (nc candidate indices, oversize last), the second
                                 * kernel's order (nel indices) and every candidate's traced boundary length */
#define CTAG_DBG_PACKS1 15      /* int32 [4 + np + nel + nc]  the work lists the first packed boundary kernel walks behind a silhouette scan (k_prepack), of a frame of a batch: nc candidates,
                                 * built (1, or 0: the last chunk's branch of the boundary stage built no such lists -- the four header words are all there is), np packs, nel
                                 * components in them; then the np pack words (first entry of the order | count << 24), the order (nel candidate indices) and, per
                                 * candidate, the number of distinct silhouette pixels the packs were built from (-1: in no pack) */
/* returns the number of ELEMENTS available (copies min(available, capacity) elements), < 0 on error */
long ctag_debug_fetch(ctag_handle* h, int frame, int what, void* dst, size_t capacity_elems);

/* evaluates the shared deterministic math on the device; op codes as oracle/ctag_oracle.h:ctago_math_probe.
 * Host arrays in/out. */
int ctag_math_probe(ctag_handle* h, int op, int n, const double* a, const double* b, double* out);

/* ---- one primitive of cylindertag_amd/csrc/ctag_wave.h by itself ---------------------------------------------------------------------------
 * n_waves waves of 64 lanes; lane l of wave w is element 64 w + l of a, ia, out and iout (host arrays) and bit l of active[w].  Every lane's out / iout
 * first get the sentinels; the lanes whose bit is set then call the primitive inside a branch, so the other lanes are off where it runs and keep the
 * sentinels.  block_threads is 64 or 256 (four waves a block).  Operands and results:
 *   lane moves, scan and sums on int          low word of ia -> iout, zero-extended (SHR1_F32: the float's bits)
 *   lane moves and sums on long long          ia -> iout
 *   SHR1_F64, SUM_F64                         a -> out
 *   SG_BEST* (d = (float)a, index = ia), MAX_F64 (d = a, index = ia)   -> out (the best d), iout (its index); NEAREST: the smallest d, ties to the lowest
 *                                             index; FARTHEST: the largest d, ties to the highest index (the two orders of k_quad.hip)
 *   ALL                                       predicate ia != 0 -> iout 0 / 1
 *   PK_MIN_U16 / PK_MAX_U16                   the low and the high word of ia -> iout
 * CTAG_ERR_ARG where the mask breaks the primitive's contract (ctag_wave.h), so that no result is an undefined value: the whole-wave forms (SG_SUM64*,
 * SG_BEST64*, SUM_F64, MAX_F64, INCL_SCAN) take all-ones masks only, the 8-lane forms (SG_SUM8*, SG_BEST8*) masks whose sub-groups are on or off as a
 * whole.  Runs on the handle's device and stream and waits. */
#define CTAG_WAVE_FROM_PREV 0
#define CTAG_WAVE_FROM_NEXT 1
#define CTAG_WAVE_SHR1_I32 2
#define CTAG_WAVE_SHR2_I32 3
#define CTAG_WAVE_SHR4_I32 4
#define CTAG_WAVE_SHR1_F32 5
#define CTAG_WAVE_SHR1_F64 6
#define CTAG_WAVE_XOR1_I32 7
#define CTAG_WAVE_XOR2_I32 8
#define CTAG_WAVE_HALF_MIRROR_I32 9
#define CTAG_WAVE_ROW_MIRROR_I32 10
#define CTAG_WAVE_XOR1_I64 11
#define CTAG_WAVE_XOR2_I64 12
#define CTAG_WAVE_HALF_MIRROR_I64 13
#define CTAG_WAVE_ROW_MIRROR_I64 14
#define CTAG_WAVE_INCL_SCAN 15
#define CTAG_WAVE_SG_SUM8_I32 16
#define CTAG_WAVE_SG_SUM64_I32 17
#define CTAG_WAVE_SG_SUM8_I64 18
#define CTAG_WAVE_SG_SUM64_I64 19
#define CTAG_WAVE_SG_BEST8_NEAREST 20
#define CTAG_WAVE_SG_BEST8_FARTHEST 21
#define CTAG_WAVE_SG_BEST64_NEAREST 22
#define CTAG_WAVE_SG_BEST64_FARTHEST 23
#define CTAG_WAVE_SUM_F64 24
#define CTAG_WAVE_MAX_F64 25
#define CTAG_WAVE_ALL 26
#define CTAG_WAVE_PK_MIN_U16 27
#define CTAG_WAVE_PK_MAX_U16 28
#define CTAG_WAVE_OPS 29
#define CTAG_WAVE_SENTINEL_F64 (-12345.6789)
#define CTAG_WAVE_SENTINEL_I64 (-0x5a5a5a5a5a5a5a5aLL)
int ctag_testkit_wave_probe(ctag_handle* h, int op, int block_threads, int n_waves, const uint64_t* active, const double* a, const int64_t* ia, double* out,
                            int64_t* iout);

/* exp32_nonpos_k0 and exp32_k_is_zero (cylindertag_amd/csrc/ctag_math.h) against exp32_nonpos on the HOST, over the floats of bit patterns first_bits,
 * first_bits + step, ... up to last_bits (all of them <= 0 and not NaN, else CTAG_ERR_ARG; among negative floats a larger pattern lies further from zero).
 * counts[0] = values visited, counts[1] = those with exp32_k_is_zero, counts[2] = those where exp32_k_is_zero(x) != (rintf(x * log2e) == 0) with the product
 * exp32_nonpos rounds, counts[3] = those with exp32_k_is_zero whose exp32_nonpos_k0 and exp32_nonpos differ in bits; *first_bad (may be null) = the bit
 * pattern of the first value counted in [2] or [3].  Host only. */
int ctag_testkit_exp32_k0_sweep(uint32_t first_bits, uint32_t last_bits, uint32_t step, uint64_t* counts, uint32_t* first_bad);

/* ---- the multi-rank unpack on one GPU -----------------------------------------------------------------------
 * Runs exactly what ctag_gather_end runs after the payload all-gather (include/ctag_gather.h): the segment table of a
 * `world`-rank job over n_total frames (shard r = the ctag_shard_range of rank r, placed at r * width in the
 * gathered buffer) and the unpack kernels, on the handle's gather stream; waits for completion.  `gathered_dev` is what
 * the all-gather would have delivered: world packed shards, each padded to `width` bytes. */
int ctag_testkit_unpack_gathered(ctag_handle* h, const void* gathered_dev, int n_total, int world, uint64_t width,
                                 ctag_frame_result* out_dev);

/* Occupies the handle's stream (ctag_stream) with a kernel that spins for about `milliseconds` (<= 10 000): what a late peer looks
 * like to the gather's bounded waits (include/ctag_gather.h: ctag_gather_set_timeout) -- work enqueued behind it, the gather stream
 * included, does not complete until it ends.  Returns at once. */
int ctag_testkit_stall_stream(ctag_handle* h, int milliseconds);

/* ---- synthetic frames -------------------------------------------------------------
 * Frame f is a pure function of (seed + f): gray background with a ramp and noise plus `markers` planted
 * CylinderTag strips of the handle's dictionary.  The same code renders on the device and on the host. */
typedef struct ctag_synth_truth {
    int32_t n_markers;
    int32_t dict_row[8];
    float strip_len[8];      /* L, full-res pixels */
    float corners[8][8];     /* image positions of the strip's 4 outer corners */
} ctag_synth_truth;
int ctag_synth_frames_device(ctag_handle* h, uint8_t* frames_dev, int first_frame, int n, int rows, int cols,
                             ptrdiff_t row_stride, ptrdiff_t frame_stride, uint64_t seed, int markers_per_frame);
int ctag_synth_frame_host(const int32_t* state, int dict_rows, int dict_cols, uint8_t* frame, int frame_index, int rows,
                          int cols, ptrdiff_t row_stride, uint64_t seed, int markers_per_frame, ctag_synth_truth* truth);
/* planted markers of synthetic frame `frame_index` without rendering it */
int ctag_synth_layout_truth(const int32_t* state, int dict_rows, int dict_cols, int frame_index, int rows, int cols, uint64_t seed,
                            int markers_per_frame, ctag_synth_truth* truth);

/* ---- synthetic 3-D scenes (BASELINE config 5: detect() + estimatePose with known answers) ---------------------
 * The same strips printed on cylinders (strip height 60 mm, a radius fixed per dictionary row) in front of a pinhole
 * camera (fx, fy, cx, cy; no distortion), every marker with a planted rigid pose; the image is ray-cast.
 * ctag_synth3d_model gives the objects' 3-D corner lists -- the `.model` of CylinderTag.cpp:168-188 for them:
 * corners[row][feature*8 + k][3] in mm, corner order as detect() emits it -- ready for ctag_model_create with
 * marker ids 0..dict_rows-1. */
typedef struct ctag_synth3d_truth {
    int32_t n_markers;
    int32_t dict_row[8];
    double R[8][9];    /* object -> camera rotation, row-major */
    double t[8][3];    /* mm */
    double radius[8];  /* mm */
} ctag_synth3d_truth;
int ctag_synth3d_frames_device(ctag_handle* h, uint8_t* frames_dev, int first_frame, int n, int rows, int cols, ptrdiff_t row_stride,
                               ptrdiff_t frame_stride, uint64_t seed, int markers_per_frame, double fx, double fy, double cx, double cy);
int ctag_synth3d_frame_host(const int32_t* state, int dict_rows, int dict_cols, uint8_t* frame, int frame_index, int rows, int cols,
                            ptrdiff_t row_stride, uint64_t seed, int markers_per_frame, double fx, double fy, double cx, double cy,
                            ctag_synth3d_truth* truth);
int ctag_synth3d_model(const int32_t* state, int dict_rows, int dict_cols, float* corners);

/* ---- edge search of the dense pose-refinement study (tests/dense_testlib.py search_edges, docs/history.md) -------
 * For one pose (rvec, tvec; Rodrigues, double) and n_seg straight 3-D segments a -> b, each given with the opposite long side
 * oa -> ob of its black quad (segments: host doubles [n_seg][12] = a, b, oa, ob), samples_per_edge samples per segment at
 * parameters (i + 0.5) / S.  Each sample is projected with K and the 14 distortion terms (cv::projectPoints, no tilt); the unit
 * normal of the projected segment there (central difference at +-1/64 of the segment) is turned away from the opposite side's
 * projection, i.e. from the dark quad to the bright paper; the u8 frame (host, pixel centres at integers) is read bilinearly
 * at offsets -r, -r + 0.5, ..., r along it; the first maximum of the central difference (I[k+1] - I[k-1]) / 2 is refined by a
 * three-point parabola.  A sample is dropped when a tap leaves [0, cols-1] x [0, rows-1] or is not finite, the maximum lies at
 * either end of the difference profile, or it is below min_contrast.
 * out: host doubles [n_seg * S][5] in segment-major order: projected point x, y, normal x, y, found offset (NaN if dropped);
 * keep: host int32 [n_seg * S].  Limits: rows, cols in [2, 32768], row_stride >= cols, n_seg in [1, 4096], S in [1, 64],
 * search_px a multiple of 0.25 in [0.5, 8], min_contrast >= 0 -- otherwise CTAG_ERR_ARG.  Runs on the handle's device and
 * waits. */
int ctag_testkit_dense_edge_probe(ctag_handle* h, const uint8_t* gray, int rows, int cols, ptrdiff_t row_stride, const double* segments,
                                  int n_seg, const double* K, const double* dist, const double* rvec, const double* tvec,
                                  int samples_per_edge, double search_px, double min_contrast, double* out, int32_t* keep);

/* ---- the Welsch line fits alone (k_line_sort + k_welsch, k_welsch_lat; cylindertag_amd/csrc/k_quad.hip: launch_line_fits) ---------
 * Fits caller-built edge clusters with the very launcher the detection chain ends its quad stage with.  Works on the workspace of the
 * handle's last chunk: run a detect call of at least n_frames (blank) frames of the size whose workspace is wanted first.  Frame f has
 * edges_per_frame[f] clusters; points_per_edge lists their point counts and xy their points (host int32 [sum n][2], 0..65535), all
 * frames back to back in input order.  The probe writes line_count, line_desc and cl_pool (clusters back to back from the start of a
 * frame's pool, or -- tail_at_pool_end -- so that the frame's last point is the pool's last element, where the read one point past a
 * cluster's last meets the pad of the allocation), runs the launcher on the handle's stream, waits, and copies line_fit back:
 * lines = host float [sum edges][4] in input order.  latency: 0 = k_welsch alone, 1 = k_welsch_lat + the pick in k_welsch (the form
 * of calls of a few frames).  welsch_gx / welsch_gs: k_welsch's blocks per frame for the long / short edges, 0 = the plan's defaults.
 * CTAG_ERR_ARG where an input does not fit: n_frames above the last chunk's frames, latency with more than 4 frames, an edge of fewer
 * than 2 points, more edges than the workspace's line_cap or more points than its cl_cap, a coordinate outside 16 bits. */
int ctag_testkit_welsch_fit(ctag_handle* h, int n_frames, const int32_t* edges_per_frame, const int32_t* points_per_edge, const int32_t* xy,
                            int latency, int welsch_gx, int welsch_gs, int tail_at_pool_end, float* lines);

/* The sizes at which those kernels change form, in the order of testkit.WELSCH_LIMITS (kWShort, kWCap, ...); host only.  Writes min(capacity, count)
 * int32 values, returns their count. */
int ctag_testkit_welsch_limits(int32_t* out, int capacity);

/* ---- edgeRefine's ordered sums alone (k_edge_refine_sums; cylindertag_amd/csrc/k_feature.hip: launch_edge_refine_sums) -----------------------
 * The sums kernel of a batch's edge refinement on caller-made inputs, launched with the plan's grid.  Works on the workspace of the handle's
 * last chunk: run a detect call of at least n_frames frames, more than four, with the corner refinement on first.  Frame f has nfeat[f] features
 * (0..CTAG_MAX_FEATURES) and the status status[f] (the kernel works on CTAG_OK frames only); corners = host float [sum nfeat][16], a feature's 8
 * corners (x, y) as K7 leaves them, quad 0 then quad 1; n0 = host double [sum 2 nfeat][4][128], per quad, edge and sample the search kernel's result
 * (NaN: no edge point), all frames back to back.  The probe writes nfeat, status, feat1 and the quads' n0 blocks, launches the kernel on the
 * handle's stream, waits, and copies the first 49 doubles of every quad's block back: sums = host double [sum 2 nfeat][49], [0, 48) the sums at
 * edge * 12 + weighting * 6 + {Mx, My, Mxx, Mxy, Myy, N}, [48] 1.0 where the quad has them.  What the kernel does not write comes back as
 * the n0 that was there.  CTAG_ERR_ARG where an input does not fit: no such workspace, n_frames above the last chunk's frames or so few that the
 * plan runs edgeRefine as one kernel, a feature count out of range. */
int ctag_testkit_refine_sums(ctag_handle* h, int n_frames, const int32_t* nfeat, const int32_t* status, const float* corners, const double* n0,
                             double* sums);

/* ---- the reduced system of the model reconstruction (cylindertag_amd/csrc/k_model_fit.hip; include/ctag_pose.h, model reconstruction) ---------
 * k_mfit_record, k_mfit_assemble and k_mfit_solve at a caller-given state instead of inside the fit's loop.  results: n_frames HOST detection
 * records; poses: n_poses HOST pose records over them, as ctag_pose_batch_device orders them -- the CTAG_POSE_OK ones are the observation records
 * (rule 1) and their rvec / tvec the state; model: the corner lists; lambda: the damping (any finite value: a negative one makes the system
 * indefinite).  For model `model_index`, with P = model_size * 8 corners: S [3P][3P] and g [3P] as assembled over ALL its corners (rule 4),
 * held [P] (rule 2, from min_obs), delta [3P] = the solution of (S + lambda diag S) delta = -g with the held corners as identity rows (0 there),
 * *bad_pivot = 1 when a pivot was not positive (delta is 0 then).  pass_records > 0: the workspace holds that many records a pass (rule 7);
 * 0: the call's own size.  Host arrays out.  Runs on the handle's device and waits. */
int ctag_testkit_model_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_pose_rec* poses, int n_poses,
                                  const ctag_model* model, const ctag_camera* camera, int model_index, double lambda, int min_obs, int pass_records,
                                  double* S, double* g, double* delta, int32_t* held, int32_t* bad_pivot);
/* k_mfit_record's grid and the records a pass holds by default (host only): out[0], out[1]; returns 2 */
int ctag_testkit_model_fit_limits(int32_t* out, int capacity);

/* ---- the reduced system of the rig assembly (cylindertag_amd/csrc/k_rig_fit.hip; include/ctag_pose.h, rig assembly) ---------------------------
 * k_rfit_record, k_fit_assemble<96> and k_fit_solve<96> at a caller-given state instead of inside the assembly's loop.  results: n_frames HOST
 * detection records; rig_poses: the n_frames x n_rigs HOST records ctag_rig_pose_batch_device gives over them on `model` with `rigs` -- the
 * CTAG_POSE_OK ones with n_members >= 2 are the observation records (rule 4) and their rvec / tvec the state; model: the corner lists, already
 * in the rig's frame; lambda: the damping (any finite value: a negative one makes the system indefinite).  For rig `rig`, whose M models (2 ..
 * CTAG_RIG_FIT_MAX_MODELS, ascending model index) own the unknowns 6k .. 6k+5 (rotation, translation: rule 5) and whose first model is the
 * anchor, with N = 6 M: *n_unknowns = N, S [N][N] and g [N] as assembled over ALL its models, delta [N] = the solution of
 * (S + lambda diag S) delta = -g with the anchor's rows as identity rows (0 there), *bad_pivot = 1 when a pivot was not positive (delta is 0
 * then).  The arrays hold 96 x 96, 96 and 96 doubles.  pass_records > 0: the workspace holds that many records a pass (rule 6); 0: the
 * call's own size.  Host arrays out.  Runs on the handle's device and waits. */
int ctag_testkit_rig_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* rig_poses,
                                const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* camera, int rig, double lambda, int pass_records,
                                double* S, double* g, double* delta, int32_t* n_unknowns, int32_t* bad_pivot);
/* k_rfit_record's grid and the records a pass holds by default (host only): out[0], out[1]; returns 2 */
int ctag_testkit_rig_fit_limits(int32_t* out, int capacity);

/* ---- the reduced system of the camera set fit (cylindertag_amd/csrc/k_cam_fit.hip; include/ctag_pose.h, camera set fit) -------------------
 * k_cfit_record, k_fit_assemble<48> and k_fit_solve<48> at a caller-given state instead of inside the fit's loop.  results: n_cameras x n_frames
 * HOST detection records, camera-major (n_cameras is the set's); mv_poses: the n_frames x n_rigs HOST records
 * ctag_mv_rig_pose_batch_device gives over them under `cams` -- the CTAG_POSE_OK ones with n_cameras >= 2 are the observation records
 * (rule 3) and their rvec / tvec the state; lambda: the damping (any finite value: a negative one makes the system indefinite).  Camera c of
 * the set owns the unknowns 6c .. 6c+5 (rotation, translation: rule 4), camera `anchor` is dropped; with N = 6 n_cameras: *n_unknowns = N,
 * S [N][N] and g [N] as assembled over ALL cameras, delta [N] = the solution of (S + lambda diag S) delta = -g with the anchor's rows as
 * identity rows (0 there), *bad_pivot = 1 when a pivot was not positive (delta is 0 then).  The arrays hold 48 x 48, 48 and 48 doubles.
 * pass_records > 0: the workspace holds that many records a pass (rule 5); 0: the call's own size.  Runs on the handle's device and waits. */
int ctag_testkit_camera_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_mv_pose_rec* mv_poses,
                                   const ctag_model* model, const ctag_rigs* rigs, const ctag_camera_set* cams, int anchor, double lambda,
                                   int pass_records, double* S, double* g, double* delta, int32_t* n_unknowns, int32_t* bad_pivot);
/* k_cfit_record's grid and the records a pass holds by default (host only): out[0], out[1]; returns 2 */
int ctag_testkit_camera_fit_limits(int32_t* out, int capacity);

/* ---- the intrinsics fit's kernels at a caller-given state (cylindertag_amd/csrc/k_intr_fit.hip; include/ctag_pose.h, intrinsics fit) -----------
 * results: n_frames HOST detection records; poses: n_frames x n_rigs HOST rig pose records -- the CTAG_POSE_OK ones are the observation
 * records and their rvec / tvec the state.
 * ctag_testkit_intrinsics_fit_system: k_ifit_record, k_ifit_assemble and k_ifit_solve at (camera, poses): S [16 x 16], g [16] over all sixteen
 * parameters (with tie_focal the fx row and column carry the tied fy), delta [16] of (S + lambda diag S) delta = -g over the free rows
 * (0 elsewhere; any finite lambda: a negative one makes the system indefinite), *n_free and whether a pivot was not positive.  free_mask and
 * tie_focal as ctag_intrinsics_fit_opts has them; pass_records > 0 sets how many records one pass of the workspace holds.
 * ctag_testkit_intrinsics_fit_poses: k_ifit_pose (rule 4) alone from the records' poses under `camera`: out gets the n_frames x n_rigs
 * records with rvec, tvec and cost of the observation records replaced, *usable = every observation record could be evaluated.  Both wait. */
int ctag_testkit_intrinsics_fit_system(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* poses,
                                       const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* camera, uint32_t free_mask, int tie_focal,
                                       double lambda, int pass_records, double* S, double* g, double* delta, int32_t* n_free, int32_t* bad_pivot);
int ctag_testkit_intrinsics_fit_poses(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_rig_pose_rec* poses,
                                      const ctag_model* model, const ctag_rigs* rigs, const ctag_camera* camera, ctag_rig_pose_rec* out, int32_t* usable);
/* the record and pose kernels' grid and the records a pass holds by default (host only): out[0], out[1]; returns 2 */
int ctag_testkit_intrinsics_fit_limits(int32_t* out, int capacity);

/* ---- the kernel forms the library picks for a chunk (plan_chunk, cylindertag_amd/csrc/ctag_api.hip) ------------------
 * For `nframes` frames of rows x cols (gray, or BGR for channels == 3) at `frames` (only its alignment is looked at) with the given
 * strides, the handle options CTAG_OPT_FUSED_SWEEP (-1: not set), CTAG_OPT_WAVE_POINTS, CTAG_OPT_BGR_DIRECT, CTAG_OPT_EXPAND_EXACT,
 * default ctag_params and no developer aids in the environment.  Host only.  Writes min(capacity, count) int32 fields in the order
 * of testkit.PLAN_FIELDS; returns their count. */
int ctag_testkit_plan(int rows, int cols, int adaptive_thresh, int nframes, int channels, int corner_subpix, const void* frames,
                      ptrdiff_t frame_stride, ptrdiff_t row_stride, int fuse_mode, int wave_points, int bgr_direct, int expand_exact,
                      int32_t* out, int capacity);

#ifdef __cplusplus
}
#endif
#endif
