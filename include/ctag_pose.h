/* ctag_pose.h -- C ABI of the pose back end on the MI355X: what the reference does in
 *     CylinderTag::loadModel    /root/reference/CylinderTag.cpp:161-190   (.model text file)
 *     CylinderTag::loadCamera   /root/reference/CylinderTag.cpp:192-196   (OpenCV FileStorage YAML: cameraMatrix, distCoeffs)
 *     CylinderTag::estimatePose /root/reference/CylinderTag.cpp:198-209
 *     PoseEstimator::PnPSolver  /root/reference/pose_estimation.cpp:50-98  (correspondences, solvePnP EPNP)
 *     PoseEstimator::PoseBA     /root/reference/pose_estimation.cpp:100-127 (undistortPoints + Ceres LM on the
 *                                                                            reprojection error of :5-48)
 * for every decoded marker of a batch of frames, on the device, straight from the detection result records
 * (ctag_frame_result in HBM) -- one wavefront per marker.
 *
 * Third-party arithmetic restated here (un-vendored in the reference, absent from this image):
 * OpenCV 4.5.3 solvePnP(SOLVEPNP_EPNP) / undistortPoints / Rodrigues and Ceres 2.0 trust-region
 * Levenberg-Marquardt (Release.props:6,11).  Floating point: the parity bar against the CPU oracle is stated in
 * tests/test_pose_gpu.py.
 *
 * The overlay of CylinderTag::drawAxis (CylinderTag.cpp:211-246) renders from those records where they lie (k_draw.hip).
 *
 * Plain pointers and sizes only.  Every function returns a CTAG_* status and never throws.
 */
#ifndef CTAG_POSE_H
#define CTAG_POSE_H
#include <stddef.h>
#include <stdint.h>

#include "ctag.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTAG_POSE_MAX_POINTS 160 /* CTAG_MAX_CODE_POS features x 8 corners */

/* status of one marker's pose */
#define CTAG_POSE_OK 0
#define CTAG_POSE_NO_MODEL 1     /* reference: pose.markerID = -1 (pose_estimation.cpp:63-66), erased by estimatePose */
#define CTAG_POSE_TOO_FEW 2      /* < 4 correspondences: cv::solvePnP throws in the reference */
#define CTAG_POSE_BAD_POS 3      /* featurePos outside the model (out-of-bounds read in the reference) */
#define CTAG_POSE_DEGENERATE 4   /* non-finite EPnP result */

/* CamInfo (header/pose_estimation.h:12-14): cameraMatrix 3x3 and distCoeffs, both 'dt: f' in cameraParams.yml */
typedef struct ctag_camera {
    float K[9];      /* row-major cameraMatrix */
    float dist[14];  /* k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (tau_x tau_y must be 0) */
    int32_t n_dist;  /* 0, 4, 5, 8, 12 or 14 */
} ctag_camera;

/* vector<ModelInfo> (header/pose_estimation.h:16-20) flattened */
typedef struct ctag_model_view {
    int32_t n_models;         /* model_num   (CylinderTag.cpp:169) */
    int32_t model_size;       /* model_size: features per marker; corners has model_size*8 points per model */
    const int32_t* marker_id; /* [n_models]  ModelInfo::MarkerID */
    const float* base;        /* [n_models*3] */
    const float* axis;        /* [n_models*3] */
    const float* corners;     /* [n_models*model_size*8*3] */
} ctag_model_view;

typedef struct ctag_pose_rec {
    int32_t status;      /* CTAG_POSE_* */
    int32_t model_index; /* PoseInfo::markerID: the INDEX into the model list (pose_estimation.cpp:59,69), -1 if none */
    int32_t frame;       /* frame index in the batch */
    int32_t marker;      /* marker index inside the frame's ctag_frame_result */
    int32_t n_points;    /* correspondences used */
    int32_t iterations;  /* LM iterations taken (successful + unsuccessful) */
    double rvec[3];      /* PoseInfo::rvec after PoseBA */
    double tvec[3];      /* PoseInfo::tvec after PoseBA */
    double rvec0[3];     /* solvePnP(EPNP) result the refinement started from */
    double tvec0[3];
    double cost0;        /* 0.5 * sum of squared reprojection residuals at the EPnP pose */
    double cost;         /* ... at the final pose */
} ctag_pose_rec;         /* 136 bytes */

typedef struct ctag_model ctag_model; /* host + device copy of a model list */

/* ---- loaders (no OpenCV FileStorage) ------------------------------------------------------------- */
/* Parses a .model text file exactly as CylinderTag::loadModel does (CylinderTag.cpp:161-190). */
int ctag_model_load(const char* path, ctag_model** out);
/* Same from arrays (copied). */
int ctag_model_create(const ctag_model_view* view, ctag_model** out);
void ctag_model_free(ctag_model* m);
int ctag_model_get_view(const ctag_model* m, ctag_model_view* view); /* host pointers, owned by the model */
/* Parses the `cameraMatrix` and `distCoeffs` !!opencv-matrix nodes of an OpenCV YAML 1.0 file
 * (CylinderTag.cpp:192-196 reads them with cv::FileStorage). */
int ctag_camera_load(const char* path, ctag_camera* out);

/* ---- pose ---------------------------------------------------------------------------------------- */
/* Poses of all markers of n_frames detection results resident in DEVICE memory (as ctag_detect_batch_device
 * leaves them).  offsets_dev[f] .. offsets_dev[f+1] index the pose records of frame f in poses_dev (one record
 * per marker of a CTAG_OK frame, in marker order, CTAG_POSE_NO_MODEL records included so that record k of a frame
 * is marker k).  offsets_dev holds n_frames+1 int32, poses_dev `capacity` records (n_frames*CTAG_MAX_MARKERS is
 * always enough).  Enqueued on the handle's stream; returns without waiting.  If the batch has more markers than
 * `capacity` the surplus is not computed and offsets_dev[n_frames] still holds the needed count. */
int ctag_pose_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                           const ctag_camera* camera, int32_t* offsets_dev, ctag_pose_rec* poses_dev, int capacity);

/* One frame, host result in, host poses out: what CylinderTag::estimatePose does before its erase
 * (CylinderTag.cpp:198-204).  out holds result->n_markers records (0 for a frame whose status is not CTAG_OK). */
int ctag_estimate_pose(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_camera* camera,
                       ctag_pose_rec* out);

/* device time of the last ctag_pose_batch_device call (needs CTAG_OPT_TIMING), milliseconds */
float ctag_pose_last_ms(ctag_handle* h);

/* ---- rig pose: one pose per rigid object that carries several markers (k_rig_pose.hip) -------------------------------------
 * A rig set maps each model index to a rig: rig_of_model[n_models], -1 = in no rig, 0 .. n_rigs-1 = that rig.  The markers of
 * one rig have their model corners in one common frame.  The record of frame f and rig g:
 *   1. res[f].status != CTAG_OK: status CTAG_POSE_NOT_SEEN, every other field 0 except rig and frame.
 *   2. Markers k = 0 .. min(n_markers, CTAG_MAX_MARKERS)-1 are visited in order.  Model index mi = the first model with the
 *      marker's marker_id (as ctag_pose_batch_device looks it up).  The marker is skipped when there is no model or
 *      rig_of_model[mi] != g.  Otherwise it is excluded, and counted in n_excluded, when
 *        - an earlier marker of the frame has the same model index (a duplicate: the first marker with a model index claims it,
 *          whether or not that marker became a member), or
 *        - the per-marker correspondence builder rejects it (what gives CTAG_POSE_BAD_POS in ctag_pose_rec), or
 *        - its points would take the rig's total past CTAG_RIG_MAX_POINTS.
 *      Any other marker is a member: bit k of member_mask is set and its correspondences are appended in the builder's own
 *      order (PnPSolver's rule: the end-feature skip, corners 0 1 4 5 [2 3 6 7]).
 *   3. No member: CTAG_POSE_NOT_SEEN.  n < 4 points: CTAG_POSE_TOO_FEW.  Otherwise EPnP then PoseBA over the n concatenated
 *      points, with the arithmetic of ctag_pose_batch_device; a non-finite EPnP result gives CTAG_POSE_DEGENERATE.  Pose fields
 *      (rvec .. cost, iterations) are 0 unless the status is CTAG_POSE_OK.
 *   4. Detection records can never exceed CTAG_RIG_MAX_POINTS (features are disjoint across markers); only hand-built or
 *      corrupted records can.
 * Identity: a rig holding one model, seen once in a frame, has the n_points, iterations, rvec, tvec, rvec0, tvec0, cost0 and
 * cost bytes of that marker's ctag_pose_rec. */
#define CTAG_POSE_NOT_SEEN 5       /* rig pose: the frame is not CTAG_OK, or no marker of the rig is a member */
#define CTAG_RIG_MAX_POINTS 800    /* CTAG_MAX_FEATURES x 8 corners */

typedef struct ctag_rig_pose_rec {
    int32_t status;          /* CTAG_POSE_OK, _TOO_FEW, _DEGENERATE or _NOT_SEEN */
    int32_t rig;             /* rig index g */
    int32_t frame;           /* frame index f in the batch */
    int32_t n_members;       /* markers whose points were used */
    int32_t n_excluded;      /* markers of the rig left out (duplicate, rejected by the builder, over CTAG_RIG_MAX_POINTS) */
    int32_t n_points;        /* correspondences used */
    int32_t iterations;      /* LM iterations taken */
    int32_t reserved;        /* 0 */
    uint32_t member_mask[4]; /* bit k (word k/32, bit k%32): marker k of the frame is a member */
    double rvec[3];          /* pose of the rig's common frame after PoseBA */
    double tvec[3];
    double rvec0[3];         /* EPnP result the refinement started from */
    double tvec0[3];
    double cost0;            /* 0.5 * sum of squared reprojection residuals at the EPnP pose */
    double cost;             /* ... at the final pose */
} ctag_rig_pose_rec;         /* 160 bytes */

typedef struct ctag_rigs ctag_rigs; /* host + device copy of a rig set */

/* Host only.  Copies rig_of_model[model's n_models]; CTAG_ERR_ARG for null pointers, n_rigs < 1 or an entry outside
 * [-1, n_rigs).  The device copy is made on the handle's device at the first pose call.  A pose call with a model whose
 * n_models differs from the one given here returns CTAG_ERR_ARG. */
int ctag_rigs_create(const ctag_model* model, const int32_t* rig_of_model, int n_rigs, ctag_rigs** out);
void ctag_rigs_free(ctag_rigs* rigs);

/* Rig poses of n_frames detection results resident in DEVICE memory: writes exactly n_frames x n_rigs records to out_dev,
 * record f*n_rigs + g for frame f and rig g, and no byte outside them.  Enqueued on the handle's stream; returns without
 * waiting. */
int ctag_rig_pose_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                               const ctag_rigs* rigs, const ctag_camera* camera, ctag_rig_pose_rec* out_dev);

/* One frame, host result in, n_rigs host records out.  Waits for completion. */
int ctag_estimate_rig_pose(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_rigs* rigs,
                           const ctag_camera* camera, ctag_rig_pose_rec* out);

/* ---- multi-view rig pose: one pose per rig from several calibrated cameras (k_mv_pose.hip) ------------------------------------
 * A camera set holds n cameras (1 .. CTAG_MV_MAX_CAMERAS): the intrinsics of each and its pose in one reference frame,
 * X_cam = R(rvec) X_ref + tvec (Rodrigues).  Every camera delivers one detection record per frame; frame f of every camera is
 * the same instant.  The record of frame f and rig g gives the pose of the rig's model frame in the REFERENCE frame,
 * X_ref = R(rvec) X_model + tvec:
 *   1. Membership.  Cameras are visited in order c = 0 .. n-1.  A camera whose record of the frame is not CTAG_OK contributes
 *      nothing (no error).  Inside one camera's record rule 2 of the rig section holds unchanged, duplicates judged per camera;
 *      the bound CTAG_RIG_MAX_POINTS holds for the TOTAL over all cameras (a marker that would pass it is excluded and counted).
 *      Bit k of member_mask[c] is set for member k of camera c.  Points are appended in camera order, then marker order, then the
 *      builder's own order.  No member in any camera: CTAG_POSE_NOT_SEEN.  Pose fields are 0 unless the status is CTAG_POSE_OK.
 *   2. Start camera: the camera with the most points, the lowest index on a tie.  Fewer than 4 points there: CTAG_POSE_TOO_FEW.
 *   3. Stage 1: EPnP then PoseBA over the start camera's points alone with its intrinsics, the arithmetic of
 *      ctag_rig_pose_batch_device: rvec_epnp tvec_epnp rvec_cam tvec_cam cost_cam0 cost_cam iterations_cam are the rvec0 tvec0
 *      rvec tvec cost0 cost iterations bytes of that camera's own ctag_rig_pose_rec whenever its members are the same.  A
 *      non-finite EPnP result gives CTAG_POSE_DEGENERATE.
 *   4. Into the reference frame: R_start = Rc^T R(rvec_cam), t_start = Rc^T (tvec_cam - tc), sums in index order, rvec_start by
 *      the inverse Rodrigues formula.  If the start camera's rvec and tvec are all exactly 0 the move is skipped: rvec_start,
 *      tvec_start are the bytes of rvec_cam, tvec_cam.
 *   5. Stage 2: the LM loop of PoseBA (same options, scaling and stop rules, sums in point order) over all n_points from
 *      (rvec_start, tvec_start).  Point i of camera c: Q = Rc (R X + t) + tc, residual (fx_c Q0/Q2 + cx_c - obs_u,
 *      fy_c Q1/Q2 + cy_c - obs_v), obs = the point's pixel undistorted with camera c's own coefficients, through its K, rounded
 *      to float; exact analytic Jacobian.  cost0 is 0.5 * sum r^2 at the start, cost at the end.  If every point belongs to the
 *      start camera, stage 2 is not run: rvec, tvec = rvec_start, tvec_start, iterations = 0, cost0 = cost = cost_cam.
 *   6. With every camera pose exactly 0 and equal intrinsics, Rc P + tc is P bit for bit, and stage 2 equals PoseBA over the
 *      concatenated points from (rvec_cam, tvec_cam) byte for byte.
 * A rig that is its own single model gets a multi-camera marker pose: there is no separate per-marker entry point. */
#define CTAG_MV_MAX_CAMERAS 8

typedef struct ctag_camera_pose {
    double rvec[3], tvec[3]; /* X_cam = R(rvec) X_ref + tvec */
} ctag_camera_pose;

typedef struct ctag_mv_pose_rec {
    int32_t status;              /* CTAG_POSE_OK, _TOO_FEW, _DEGENERATE or _NOT_SEEN */
    int32_t rig;                 /* rig index g */
    int32_t frame;               /* frame index f in the batch */
    int32_t n_cameras;           /* cameras with at least one member */
    int32_t start_camera;        /* rule 2; 0 when there is no member */
    int32_t n_members;           /* totals over all cameras */
    int32_t n_excluded;
    int32_t n_points;
    int32_t iterations;          /* LM iterations of stage 2 */
    int32_t iterations_cam;      /* ... of stage 1 */
    int32_t points_of_camera[CTAG_MV_MAX_CAMERAS];
    uint32_t member_mask[CTAG_MV_MAX_CAMERAS][4]; /* camera c, marker k: word k/32, bit k%32 */
    int32_t reserved[2];         /* 0 */
    double rvec_epnp[3];         /* EPnP pose in the start camera's frame */
    double tvec_epnp[3];
    double rvec_cam[3];          /* stage-1 pose in the start camera's frame */
    double tvec_cam[3];
    double cost_cam0;            /* stage-1 cost at the EPnP pose */
    double cost_cam;             /* ... at the stage-1 pose */
    double rvec_start[3];        /* stage-2 start in the reference frame */
    double tvec_start[3];
    double cost0;                /* cost over all points at the start */
    double rvec[3];              /* final pose in the reference frame */
    double tvec[3];
    double cost;                 /* ... and its cost */
} ctag_mv_pose_rec;              /* 432 bytes */

typedef struct ctag_camera_set ctag_camera_set; /* n cameras: intrinsics + pose of each in one reference frame */

/* Host only.  Copies both arrays.  CTAG_ERR_ARG for null pointers, n_cameras outside 1 .. CTAG_MV_MAX_CAMERAS or a non-finite
 * pose entry; CTAG_ERR_UNSUPPORTED for a camera the pose back end does not handle (tilt terms). */
int ctag_camera_set_create(const ctag_camera* cameras, const ctag_camera_pose* poses, int n_cameras, ctag_camera_set** out);
void ctag_camera_set_free(ctag_camera_set* s);

/* results_dev: HOST array of n_cameras DEVICE pointers, n_frames records each (read before the call returns).  Writes exactly
 * n_frames x n_rigs records to out_dev, record f*n_rigs + g, and no byte outside them.  Enqueued on the handle's stream;
 * returns without waiting.  Arguments are judged as ctag_rig_pose_batch_device judges them. */
int ctag_mv_rig_pose_batch_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_frames, const ctag_model* model,
                                  const ctag_rigs* rigs, const ctag_camera_set* cams, ctag_mv_pose_rec* out_dev);

/* One instant: n_cameras HOST records in (record c from camera c), n_rigs host records out.  Waits for completion. */
int ctag_estimate_mv_rig_pose(ctag_handle* h, const ctag_frame_result* results, const ctag_model* model, const ctag_rigs* rigs,
                              const ctag_camera_set* cams, ctag_mv_pose_rec* out);

/* ---- pose covariance: how far a pose record can be trusted (k_pose_cov.hip) ------------------------------------------------------
 * One ctag_pose_cov_rec per pose record of any of the three kinds above, computed on the device from the pose records and the
 * detection records where they lie: the 6x6 covariance of the pose under the first-order model cov = sigma^2 (J^T J)^-1 at the
 * record's final pose, and the residuals' diagnostics.  No pose record, kernel or result above is changed by it.
 *   1. A source record whose status is not CTAG_POSE_OK gives CTAG_COV_NO_POSE.  For every status but CTAG_COV_OK all other
 *      fields of the covariance record are 0.
 *   2. The points are rebuilt from the detection record(s) exactly as the pose call built them (the builder's rule and order:
 *      the end-feature skip, corners 0 1 4 5 [2 3 6 7]):
 *        per marker  marker poses[w].marker of frame poses[w].frame against model poses[w].model_index;
 *        rig         frame rig_poses[w].frame: the markers whose bit is set in member_mask, in marker order, each against the
 *                    first model with its marker_id;
 *        multi-view  frame mv_poses[w].frame: the same per camera c from member_mask[c], in camera order; each camera's pixels
 *                    are undistorted with that camera's own coefficients.
 *      CTAG_COV_BAD_RECORD when the source record does not describe its detection record(s): an index lies outside its array
 *      (frame outside the batch, marker >= the frame's marker count, model_index outside the model list, a member bit at or
 *      past the frame's marker count, a member whose marker_id has no model, a member_mask of a camera the set does not have),
 *      a frame that is read is not CTAG_OK, the builder rejects a member (CTAG_POSE_BAD_POS) or the total passes
 *      CTAG_RIG_MAX_POINTS, the rebuilt point count differs from the record's n_points or is below 4, or rvec / tvec are not
 *      finite.  Nothing outside the records' own data is ever read.  The rig set only gives n_rigs: rig_of_model is not
 *      consulted, the member_mask is the membership.
 *   3. The residual is PoseBA's, in undistorted pixels: rule 5 of the multi-view section for multi-view records, the same with
 *      one camera at the reference for the other two.  The covariance describes THAT residual: the observations are the
 *      undistorted pixels, and the Jacobian of the undistortion itself is taken as the identity (sigma_px is a noise of the
 *      undistorted pixel).
 *   4. Unknowns.  CTAG_COV_PARAM_RVEC: the record's own coordinates (rvec, tvec); the rotation derivatives are those of the
 *      Rodrigues formula, as the LM loop has them.  CTAG_COV_PARAM_TANGENT: R <- Exp(dw) R, t <- t + dt, dw a small rotation
 *      vector in the frame the pose maps INTO (the camera; the reference frame for multi-view records): dR/dw_k = [e_k]x R.
 *      The translation columns are the same in both.
 *   5. H = J^T J (6x6), D = diag(H)^-1/2, C = D H D (unit diagonal), C = L L^T by Cholesky; min_pivot is the smallest pivot of
 *      that factorisation before its square root.  CTAG_COV_SINGULAR when the cost or a diagonal entry of H is not finite, a
 *      diagonal entry of H is not positive, or a pivot is not above 1e-12 (well-posed problems of 4 to 160 points stay above
 *      1e-6; four coincident points give -2e-16).  Otherwise cov = sigma2_used * D C^-1 D, mirrored so that it is symmetric bit
 *      for bit.
 *   6. Deterministic: lane l of one wavefront owns points l, l+64, ... in order, the lanes are combined in one fixed tree.  The
 *      same source record gives the same bytes in any batch, at any place in it, in a one-frame call and on a second run. */
#define CTAG_COV_OK 0
#define CTAG_COV_NO_POSE 1     /* the source pose record's status is not CTAG_POSE_OK */
#define CTAG_COV_BAD_RECORD 2  /* the source record does not describe its detection record(s): rule 2 */
#define CTAG_COV_SINGULAR 3    /* rule 5 */

#define CTAG_COV_PARAM_TANGENT 0 /* R <- Exp(dw) R, t <- t + dt: dw in the frame the pose maps INTO (camera; reference frame for mv) */
#define CTAG_COV_PARAM_RVEC 1    /* the record's own coordinates (rvec, tvec) */

typedef struct ctag_cov_opts {
    uint32_t struct_size;  /* filled by ctag_cov_opts_default, checked */
    int32_t param;         /* CTAG_COV_PARAM_* ; default TANGENT */
    double sigma_px;       /* > 0: the pixel noise to assume; <= 0 (default 0): use sigma2_hat */
    double outlier_k;      /* > 0: count points whose residual norm exceeds outlier_k * sqrt(sigma2_used); default 3 */
} ctag_cov_opts;

typedef struct ctag_pose_cov_rec {
    int32_t status;        /* CTAG_COV_* */
    int32_t n_points;
    int32_t dof;           /* 2 * n_points - 6 */
    int32_t worst_point;   /* index, in the builder's point order, of the largest residual norm; lowest index on a tie */
    int32_t n_outliers;    /* 0 when outlier_k <= 0 */
    int32_t param;
    double cost;           /* 0.5 * sum r^2 at the record's final pose, recomputed */
    double sigma2_hat;     /* 2 * cost / dof */
    double sigma2_used;    /* sigma_px^2 if sigma_px > 0, else sigma2_hat */
    double max_residual_px;
    double min_pivot;      /* rule 5 */
    double cov[36];        /* row-major, symmetric bit for bit: sigma2_used * (J^T J)^-1; rows/cols 0-2 rotation (rad), 3-5 translation (model units) */
} ctag_pose_cov_rec;       /* 352 bytes */

void ctag_cov_opts_default(ctag_cov_opts* opts);

/* The three batch calls: enqueued on the handle's stream, return without waiting, write no byte outside their records.  Arguments
 * are judged as the matching pose call judges them; opts == NULL means the defaults; a wrong struct_size, an unknown param or a
 * sigma_px / outlier_k that is not finite gives CTAG_ERR_ARG.
 * Per marker: offsets_dev, poses_dev and capacity as ctag_pose_batch_device left them.  Covariance record w is for pose record w,
 * for every w < min(offsets_dev[n_frames], capacity); nothing beyond those records is written. */
int ctag_pose_cov_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                               const ctag_camera* camera, const int32_t* offsets_dev, const ctag_pose_rec* poses_dev, int capacity,
                               const ctag_cov_opts* opts, ctag_pose_cov_rec* out_dev);
/* Rig: rig_poses_dev as ctag_rig_pose_batch_device left it; writes exactly n_frames x n_rigs records, record w for pose record w. */
int ctag_rig_pose_cov_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                                   const ctag_rigs* rigs, const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses_dev,
                                   const ctag_cov_opts* opts, ctag_pose_cov_rec* out_dev);
/* Multi-view: results_dev is a HOST array of n_cameras DEVICE pointers (read before the call returns), mv_poses_dev as
 * ctag_mv_rig_pose_batch_device left it; writes exactly n_frames x n_rigs records. */
int ctag_mv_rig_pose_cov_batch_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_frames, const ctag_model* model,
                                      const ctag_rigs* rigs, const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses_dev,
                                      const ctag_cov_opts* opts, ctag_pose_cov_rec* out_dev);

/* One frame (one instant), host memory in and out, the records of the matching ctag_estimate_* call (their frame fields 0); they
 * wait for completion.  out holds result->n_markers records (none for a frame that is not CTAG_OK), n_rigs records for the other two. */
int ctag_estimate_pose_cov(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_camera* camera,
                           const ctag_pose_rec* poses, const ctag_cov_opts* opts, ctag_pose_cov_rec* out);
int ctag_estimate_rig_pose_cov(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_rigs* rigs,
                               const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses, const ctag_cov_opts* opts,
                               ctag_pose_cov_rec* out);
int ctag_estimate_mv_rig_pose_cov(ctag_handle* h, const ctag_frame_result* results, const ctag_model* model, const ctag_rigs* rigs,
                                  const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses, const ctag_cov_opts* opts,
                                  ctag_pose_cov_rec* out);

/* ---- robust refit: a finished pose minimised again under a loss (k_pose_robust.hip) ----------------------------------------------------
 * Every pose above minimises a plain sum of squares (pose_estimation.cpp:141 passes NULL in AddResidualBlock's loss slot), so one
 * mislocated feature pulls the pose with its full weight.  One ctag_robust_pose_rec per pose record of any of the three kinds: the
 * record's points under Ceres 2.0's stock Huber or Cauchy loss, minimised by PoseBA's loop from the record's own pose, with the
 * inlier set the loss ends with.  Like the covariance calls it takes finished records and changes nothing above it;
 * ctag_pose_rec / ctag_rig_pose_rec / ctag_mv_pose_rec with rvec, tvec replaced by the refit's go into the covariance and overlay calls.
 *   1. A source record whose status is not CTAG_POSE_OK gives CTAG_ROBUST_NO_POSE.  For every status but CTAG_ROBUST_OK all other
 *      fields of the robust record are 0.
 *   2. The points are rebuilt exactly as rule 2 of the covariance section rebuilds them: the same walk, the same order, the same
 *      causes of rejection (a mask bit at or past the frame's marker count among them), reported as CTAG_ROBUST_BAD_RECORD.  Nothing
 *      outside the records' own data is ever read.
 *   3. r_i is PoseBA's residual of point i in undistorted pixels (rule 3 there; rule 5 of the multi-view section for multi-view
 *      records, the pose stays in the reference frame); s_i = r_i . r_i.
 *   4. Scale a, fixed for the whole record.  m = the lower median of sqrt(s_i) at the source pose: the value of rank (n - 1) / 2
 *      (integer division) in ascending order, one value of the array, never an interpolation.  sigma_hat = m / 1.1774100225154747
 *      (the median of a Rayleigh variable in units of its sigma); it is always computed and reported.  a = scale_px if scale_px > 0,
 *      else max(auto_k * sigma_hat, min_scale_px).
 *   5. Loss: Ceres 2.0's stock definitions on the squared norm of a residual block, a block being one point (pose_estimation.cpp:141).
 *        CTAG_LOSS_HUBER   rho(s) = s for s <= a^2, else 2 a sqrt(s) - a^2;     rho'(s) = 1, else a / sqrt(s)
 *        CTAG_LOSS_CAUCHY  rho(s) = a^2 log(1 + s / a^2);                       rho'(s) = 1 / (1 + s / a^2)
 *      Both have rho'' <= 0, for which Ceres' corrector is exactly: scale the point's two residuals and two Jacobian rows by
 *      sqrt(rho'(s_i)).  There is no alpha branch to implement.  The cost is 0.5 sum rho(s_i); it is NOT the squared norm of the
 *      scaled residuals.
 *   6. Loop: PoseBA's (Ceres' TrustRegionMinimizer with the Levenberg-Marquardt strategy and the options of ctag_pose_batch_device:
 *      radius 1e4, the diagonal clamped to [1e-6, 1e32], Jacobi scaling 1 / (1 + column norm) from the first evaluation, a step is
 *      accepted when its cost decrease is above 1e-3 of the model's, radius / max(1/3, 1 - (2 rho - 1)^3) then, radius / 2, / 4, ...
 *      after a rejected one; it stops at a gradient of 1e-15, a step of 1e-10 |x|, a cost change of 1e-15 of the cost, a radius of
 *      1e-32) over the scaled rows with rule 5's cost, from the source record's (rvec, tvec), at most max_iterations times (0 .. 50).
 *      max_iterations = 0 evaluates only: rvec, tvec are the source's bytes, cost = cost0, cost_ls = cost_ls0, and the mask and the
 *      worst point are those of the source pose.  `iterations` counts accepted and rejected steps.  A loop that max_iterations does
 *      not end finishes in steps whose cost change lies below the rounding of a float64 cost (the residual is a difference of pixel
 *      coordinates near 1000): its iteration count is a property of the build, the final pose is not.
 *   7. Reported.  At the start cost0 (rule 5) and cost_ls0 = 0.5 sum s_i; at the end cost, cost_ls, max_residual_px = the largest
 *      sqrt(s_i) and worst_point, its index (the lowest on a tie).  Bit i (word i / 32, bit i % 32) of inlier_mask is set iff
 *      s_i <= a^2 at the end, under either loss; n_inliers is their count.  A cost0 that is not finite gives CTAG_ROBUST_DEGENERATE.
 *   8. Deterministic, as rule 6 of the covariance section: lane l owns points l, l + 64, ... in order, one fixed tree over the lanes.
 *      The same source record gives the same bytes anywhere in any batch, in a one-frame call and on a second run.
 *   9. CTAG_ERR_ARG: a wrong struct_size, an unknown loss, max_iterations outside 0 .. 50, scale_px / auto_k / min_scale_px that
 *      are not finite, scale_px <= 0 together with auto_k <= 0 or with min_scale_px <= 0.  Everything else is judged as the matching
 *      pose call judges it.
 * What to expect (tools/robust_study.py; planted poses, 0.2 px noise, the 8 corners of ONE feature moved together
 * by 2 or 5 px).  The refit can be relied on from FOUR CLEAN FEATURES next to the wrong one: with five features of one marker Cauchy's
 * pose is nearer the planted one than the least-squares pose in 97-99 % of the trials and halves the median error, from six on in
 * 98-100 % with 25-40 % of it left, and for rigs of three markers from two features each.  With three clean features it wins in 78 %,
 * with two (a third of the points wrong) in 45 %: it does not help there and does not claim to -- n_inliers and inlier_mask say what was kept.
 * Huber removes less than Cauchy everywhere. */
#define CTAG_ROBUST_OK 0
#define CTAG_ROBUST_NO_POSE 1     /* the source pose record's status is not CTAG_POSE_OK */
#define CTAG_ROBUST_BAD_RECORD 2  /* the source record does not describe its detection record(s): rule 2 */
#define CTAG_ROBUST_DEGENERATE 3  /* rule 7: the cost at the source pose is not finite */

#define CTAG_LOSS_HUBER 0
#define CTAG_LOSS_CAUCHY 1

typedef struct ctag_robust_opts {
    uint32_t struct_size;   /* filled by ctag_robust_opts_default, checked */
    int32_t loss;           /* CTAG_LOSS_* ; default CAUCHY */
    int32_t max_iterations; /* 0 .. 50; default 50 */
    int32_t reserved;       /* 0 */
    double scale_px;        /* > 0: the loss's scale a; <= 0 (default 0): automatic, rule 4 */
    double auto_k;          /* default 2.5 */
    double min_scale_px;    /* default 0.05 */
} ctag_robust_opts;         /* 40 bytes */

typedef struct ctag_robust_pose_rec {
    int32_t status;          /* CTAG_ROBUST_* */
    int32_t n_points;
    int32_t n_inliers;       /* points with s_i <= a^2 at the final pose */
    int32_t iterations;      /* loop iterations taken (successful + unsuccessful) */
    int32_t loss;
    int32_t worst_point;     /* index, in the builder's point order, of the largest residual norm at the final pose; lowest on a tie */
    uint32_t inlier_mask[25];/* bit i (word i / 32, bit i % 32): point i, in the builder's order, is an inlier */
    int32_t reserved;        /* 0 */
    double scale_px;         /* a, rule 4 */
    double sigma_hat;        /* rule 4 */
    double cost_ls0;         /* 0.5 sum s_i at the source pose */
    double cost_ls;          /* ... at the final pose */
    double cost0;            /* 0.5 sum rho(s_i) at the source pose */
    double cost;             /* ... at the final pose */
    double max_residual_px;  /* at the final pose */
    double rvec[3];          /* the refitted pose, in the source record's frame */
    double tvec[3];
} ctag_robust_pose_rec;      /* 232 bytes */

void ctag_robust_opts_default(ctag_robust_opts* opts);

/* The three batch calls take the argument lists of the covariance calls with robust options in place of the covariance options:
 * enqueued on the handle's stream, return without waiting, write no byte outside their records; record w is for pose record w;
 * opts == NULL means the defaults. */
int ctag_pose_robust_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                                  const ctag_camera* camera, const int32_t* offsets_dev, const ctag_pose_rec* poses_dev, int capacity,
                                  const ctag_robust_opts* opts, ctag_robust_pose_rec* out_dev);
int ctag_rig_pose_robust_batch_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model,
                                      const ctag_rigs* rigs, const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses_dev,
                                      const ctag_robust_opts* opts, ctag_robust_pose_rec* out_dev);
int ctag_mv_rig_pose_robust_batch_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_frames, const ctag_model* model,
                                         const ctag_rigs* rigs, const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses_dev,
                                         const ctag_robust_opts* opts, ctag_robust_pose_rec* out_dev);

/* One frame (one instant), host memory in and out, as the one-frame covariance calls; they wait for completion. */
int ctag_estimate_pose_robust(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_camera* camera,
                              const ctag_pose_rec* poses, const ctag_robust_opts* opts, ctag_robust_pose_rec* out);
int ctag_estimate_rig_pose_robust(ctag_handle* h, const ctag_frame_result* result, const ctag_model* model, const ctag_rigs* rigs,
                                  const ctag_camera* camera, const ctag_rig_pose_rec* rig_poses, const ctag_robust_opts* opts,
                                  ctag_robust_pose_rec* out);
int ctag_estimate_mv_rig_pose_robust(ctag_handle* h, const ctag_frame_result* results, const ctag_model* model, const ctag_rigs* rigs,
                                     const ctag_camera_set* cams, const ctag_mv_pose_rec* mv_poses, const ctag_robust_opts* opts,
                                     ctag_robust_pose_rec* out);

/* ---- track smoothing: one trajectory per rig over the frames of a batch (k_track.hip) ---------------------------------------------------
 * Every call above treats frame f on its own.  This one takes the n_frames x n_rigs rig pose records of a batch (record w = f * n_rigs + g,
 * ctag_rig_pose_rec from one camera or ctag_mv_pose_rec in the reference frame) with their covariance records and a time per frame, and
 * returns per rig the trajectory that a constant-velocity model (white noise on acceleration) draws through them: every frame informs
 * its neighbours in proportion to its covariance, short losses are bridged, every frame gets a velocity and a covariance of the result.
 * Nothing above is changed by it.  times: a HOST array of n_frames finite, strictly increasing doubles; NULL means t_f = f * opts.dt.
 *   1. Measured.  Frame f is measured for rig g when the pose record's status is CTAG_POSE_OK, the covariance record's status is
 *      CTAG_COV_OK with param CTAG_COV_PARAM_TANGENT, and cov factors as rule 5 of the covariance section factors H: D = diag(cov)^-1/2
 *      (every diagonal entry positive and finite), C = D cov D = L L^T with every pivot above 1e-12.  W_f = cov^-1 = D C^-1 D,
 *      (Rm_f, tm_f) = (R(rvec), tvec).  Bad input, not an unmeasured frame: a CTAG_COV_OK covariance record with param
 *      CTAG_COV_PARAM_RVEC, and a pose record whose rig or frame field is not its place in the array.  Either gives the rig's stat record
 *      and every one of its frame records CTAG_TRACK_BAD_INPUT; all other fields of those frame records are 0 except rig and frame.
 *   2. Pieces.  A piece is a maximal run of frames [a, b] whose ends are measured and in which no two consecutive measured frames are
 *      more than max_gap frame indices apart.  Frames in no piece get CTAG_TRACK_NOT_TRACKED, every other field 0 except rig and frame.
 *      Pieces are independent problems; a piece may be one frame.
 *   3. Unknowns per frame of a piece: the pose (R_f, t_f), the angular velocity w_f in the frame the pose maps INTO (the frame of the
 *      covariance's dw) and the translational velocity v_f.  Update R <- Exp(dtheta) R; the other nine unknowns are additive.
 *   4. Cost of a piece = half the sum of
 *        measurement, at every measured frame: rho(e^T W_f e), e = [Log(R_f Rm_f^T); t_f - tm_f];
 *        motion, between frames f and f+1 of the piece, D = t_{f+1} - t_f: a = [Log(R_{f+1} R_f^T) - D w_f; t_{f+1} - t_f - D v_f],
 *          b = [w_{f+1} - w_f; v_{f+1} - v_f], per axis k: (12 a_k^2 / D^3 - 12 a_k b_k / D^2 + 4 b_k^2 / D) / q_k, q_k = q_rot for the
 *          three rotation axes, q_trans for the three translation axes;
 *        velocity prior, at the piece's first frame: |w_a|^2 / vel0_sigma_rot^2 + |v_a|^2 / vel0_sigma_trans^2.
 *      rho is the identity for CTAG_TRACK_LOSS_NONE; for CTAG_LOSS_HUBER / CTAG_LOSS_CAUCHY it is the robust refit's rule 5 with
 *      a = loss_scale on the squared Mahalanobis norm (one function for both: ctag_loss.h).
 *   5. Start.  A measured frame starts at its measurement.  An unmeasured frame between its nearest measured neighbours p < f < n starts at
 *      Exp(s Log(Rm_n Rm_p^T)) Rm_p and tm_p + s (tm_n - tm_p), s = (t_f - t_p) / (t_n - t_p).  w_f, v_f are the forward differences of the
 *      starts, Log(R_{f+1} R_f^T) / D and (t_{f+1} - t_f) / D; the last frame copies its predecessor's; a one-frame piece gets 0.
 *   6. Minimisation: Levenberg-Marquardt on the Gauss-Newton system of rule 4, (A + lambda diag A) delta = -g, the loss by its weight
 *      rho' alone (no second-order correction, as the robust refit).  One lambda per piece from lambda0; a trial is accepted iff the
 *      cost decreases, lambda <- max(lambda / 3, 1e-9) on accept and 4 lambda on reject; a piece stops when an accepted round lowers the
 *      cost by less than 1e-12 of it, when lambda exceeds 1e6, or after max_iterations rounds (the fits' round control, ctag_lm.h,
 *      decided on the device: the call does not wait).  A round whose factorisation meets a pivot that is not positive is a reject.
 *      max_iterations = 1 with lambda0 = 0 is one undamped Gauss-Newton step from the start of rule 5.
 *   7. Result: ctag_track_rec, row f * n_rigs + g.  cov is the pose's 6x6 marginal block of the inverse of the undamped Gauss-Newton
 *      matrix at the returned state, in the parametrisation of the input covariance, symmetric bit for bit; vel_sigma the square roots
 *      of the diagonal of the velocity marginal (w then v); mahalanobis2 = e^T W_f e and weight = rho' at the returned state (0 and 1
 *      where the frame is unmeasured).  Every frame of a solved piece, measured or bridged, is CTAG_TRACK_OK; every frame of a piece
 *      whose final factorisation met a pivot that is not positive or whose cost is not finite is CTAG_TRACK_SINGULAR (its pose fields
 *      are the last accepted state, cov and vel_sigma 0).  ctag_track_stat, one per rig: cost0 and cost are summed over the pieces in
 *      piece order.
 *   8. Deterministic.  A piece's bytes do not depend on the rig index it belongs to, on where it lies in the batch, on what the other
 *      rigs hold, or on the run.  Every entry of every block has one owner lane and a fixed order of summation; the cost of a piece is
 *      lane l's frames l, l + 64, ... of the piece in order, then wave_sum_f64's tree.  No floating-point atomics.
 *   9. The system of a piece is block-tridiagonal along time, 12 unknowns a frame.  It is cut every segment_frames frames counted from
 *      the piece's first frame (local frames 0, L, 2L, ... are separators); one wavefront per segment eliminates the frames between two
 *      separators, one wavefront per piece solves the separators' chain, the segments substitute back side by side, and the marginals come
 *      from the same factors (selected inverse along the separators, interiors conditioned on their two separators).  The result does
 *      not depend on L beyond rounding.  segment_frames = 0 is the library's choice, 64.
 *  10. CTAG_ERR_ARG: a null argument (times excepted), n_frames < 1, a wrong struct_size, an unknown loss, dt / q_rot / q_trans /
 *      vel0_sigma_rot / vel0_sigma_trans / loss_scale that are not positive and finite, lambda0 that is negative or not finite,
 *      max_iterations < 1, max_gap < 1, segment_frames outside {0, 8, 16, 32, 64}, times that are not finite and strictly increasing,
 *      n_frames x n_rigs above CTAG_TRACK_MAX_ITEMS.  Device memory of one call: 8400 bytes per (frame, rig) item, 0.55 GB at the bound. */
#define CTAG_TRACK_OK 0
#define CTAG_TRACK_NOT_TRACKED 1  /* the frame lies in no piece: rule 2 */
#define CTAG_TRACK_BAD_INPUT 2    /* rule 1: the whole rig */
#define CTAG_TRACK_SINGULAR 3     /* rule 7: the whole piece */

#define CTAG_TRACK_LOSS_NONE 2    /* beside CTAG_LOSS_HUBER 0 and CTAG_LOSS_CAUCHY 1 */
#define CTAG_TRACK_MAX_ITEMS 65536 /* n_frames x n_rigs of one call */

#define CTAG_TRACK_FLAG_MEASURED 1u     /* rule 1 */
#define CTAG_TRACK_FLAG_DOWNWEIGHTED 2u /* the loss's weight at the returned state is below 1 (CTAG_HE_FLAG_DOWNWEIGHTED is defined otherwise) */

typedef struct ctag_track_opts {
    uint32_t struct_size;    /* filled by ctag_track_opts_default, checked */
    int32_t loss;            /* CTAG_TRACK_LOSS_NONE (default), CTAG_LOSS_HUBER or CTAG_LOSS_CAUCHY */
    int32_t max_iterations;  /* >= 1; default 10 */
    int32_t max_gap;         /* >= 1; default 5 */
    int32_t segment_frames;  /* 0 (default: the library's choice), 8, 16, 32 or 64 */
    int32_t reserved;        /* 0 */
    double dt;               /* seconds between frames when times == NULL; default 1 / 30 */
    double q_rot;            /* power spectral density of the angular acceleration, rad^2 / s^3; default 0.1: a hand-held object (tools/track_study.py) */
    double q_trans;          /* ... of the translational acceleration, model units^2 / s^3; default 3000: the same, for a model in mm */
    double vel0_sigma_rot;   /* rad / s; default 10 */
    double vel0_sigma_trans; /* model units / s; default 1000 */
    double loss_scale;       /* a of the loss, in units of the Mahalanobis norm; default 4 */
    double lambda0;          /* >= 0; default 1e-3 */
} ctag_track_opts;           /* 80 bytes */

typedef struct ctag_track_rec {
    int32_t status;          /* CTAG_TRACK_* */
    int32_t rig;
    int32_t frame;
    uint32_t flags;          /* CTAG_TRACK_FLAG_* */
    double rvec[3];          /* the smoothed pose, Rodrigues, in the frame of the input records */
    double tvec[3];
    double w[3];             /* angular velocity, rad / s */
    double v[3];             /* translational velocity, model units / s */
    double cov[36];          /* rule 7; rows/cols 0-2 rotation, 3-5 translation */
    double vel_sigma[6];
    double mahalanobis2;
    double weight;
} ctag_track_rec;            /* 464 bytes */

typedef struct ctag_track_stat {   /* one per rig */
    int32_t status;          /* CTAG_TRACK_OK or CTAG_TRACK_BAD_INPUT */
    int32_t n_measured;
    int32_t n_pieces;
    int32_t n_tracked;       /* frames in a piece */
    int32_t longest_piece;   /* frames */
    int32_t rounds;          /* sum over the pieces of the rounds taken (accepted + rejected) */
    double cost0;            /* cost at the start of rule 5, summed over the pieces in piece order */
    double cost;             /* ... at the returned state */
} ctag_track_stat;           /* 40 bytes */

void ctag_track_opts_default(ctag_track_opts* opts);
/* Device records in, device records out: rig_poses_dev / cov_dev as ctag_rig_pose_batch_device and ctag_rig_pose_cov_batch_device left
 * them.  Writes exactly n_frames x n_rigs track records to out_dev and n_rigs stat records to stat_dev and no byte outside them.
 * Enqueued on the handle's stream; returns without waiting for its own work or for anything else on the stream, with one exception: the
 * workspace is the handle's, so an earlier smoothing call of this handle that is still in flight is waited for first.  The rig set only gives n_rigs.  opts == NULL means the defaults. */
int ctag_rig_track_smooth_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                 int n_frames, const double* times, const ctag_track_opts* opts, ctag_track_rec* out_dev, ctag_track_stat* stat_dev);
int ctag_mv_rig_track_smooth_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                    int n_frames, const double* times, const ctag_track_opts* opts, ctag_track_rec* out_dev, ctag_track_stat* stat_dev);
/* The same with HOST arrays in and out; they wait for completion. */
int ctag_rig_track_smooth(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                          const double* times, const ctag_track_opts* opts, ctag_track_rec* out, ctag_track_stat* stat);
int ctag_mv_rig_track_smooth(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                             const double* times, const ctag_track_opts* opts, ctag_track_rec* out, ctag_track_stat* stat);
/* device time of the last smoothing call's kernels (needs CTAG_OPT_TIMING), milliseconds: gather + pieces + start, the rounds, the
 * marginals and the records, the whole call */
int ctag_track_last_ms(ctag_handle* h, float* out4);

/* ---- track filtering: the smoother's causal counterpart, one frame at a time (k_track_filter.hip) -----------------------------------------
 * The smoother needs every frame of a batch; a live caller has the frames up to now.  A ctag_track_filter holds per rig the state of an
 * extended Kalman filter on (R, t, w, v) under the smoother's model (white noise on acceleration) in device memory between calls.  A
 * step call takes the n_frames x n_rigs pose and covariance records of the call (record w = f * n_rigs + g, rig and frame fields equal
 * to their place in THIS call's arrays) in order, from the state the previous call left, and writes n_frames x n_rigs ctag_track_rec;
 * n_frames = 1 is the live use.  times: a HOST array of n_frames finite, strictly increasing doubles, the first above the last time the
 * filter was given; it is copied before the call returns.  NULL means t = (frames given since creation or reset + f) * opts.dt.
 *   1. Measured and bad input are the smoother's rule 1 (the same functions).  cov_f below is the covariance record's matrix read from
 *      its upper triangle.  If any record of rig g in a call is bad input, every record of rig g of that call is CTAG_TRACK_BAD_INPUT,
 *      all other fields 0 except rig and frame, and the state of rig g is left exactly as it was.  Other rigs are unaffected.
 *   2. A track is EMPTY (at creation and after a reset) or TRACKING.  EMPTY and an unmeasured frame: CTAG_TRACK_NOT_TRACKED, every other
 *      field 0 except rig and frame.  EMPTY and a measured frame starts the track: R = Rm, t = tm, w = v = 0,
 *      P = blockdiag(cov_f, vel0_sigma_rot^2 I, vel0_sigma_trans^2 I) in the order theta, t, w, v; flags MEASURED | STARTED,
 *      mahalanobis2 0, weight 1: the smoother's first frame, a measurement plus the velocity prior.
 *   3. Predict over D = t - t_prev: E = Exp(D w), R- = E R, t- = t + D v, w and v kept.  F has the blocks theta,theta = E,
 *      theta,w = D Jl(D w) (Jl the left Jacobian of SO(3)), t,t = I, t,v = D I, w,w = v,v = I.  P- = F P F^T + Q; per axis
 *      Q = q [[D^3 / 3, D^2 / 2], [D^2 / 2, D]] between (theta, w) with q_rot and between (t, v) with q_trans: the inverse of the motion
 *      term of the smoother's rule 4.
 *   4. Update at a measured frame: phi = Log(R- Rm^T), e = [phi; t- - tm], H = [Jl^-1(phi) 0 0 0; 0 I 0 0].  S = H P- H^T + cov_f is
 *      scaled to unit diagonal and factored with pivots above 1e-12; d^2 = e^T S^-1 e.  Gate: gate > 0 and d^2 > gate^2 gives flags
 *      MEASURED | GATED, weight 0, and the state treats the frame as unmeasured (rule 5).  Otherwise omega = rho'(d^2) of the loss with
 *      a = loss_scale (ctag_loss.h; 1 without a loss), C = cov_f / omega, K = P- H^T (H P- H^T + C)^-1 (the same factorisation; S itself
 *      when omega = 1), delta = -K e, R = Exp(delta_theta) R-, the other nine unknowns additive,
 *      P = (I - K H) P- (I - K H)^T + K C K^T (Joseph form; every entry (a <= b) is computed once and mirrored: P is symmetric bit for
 *      bit).  DOWNWEIGHTED when omega < 1; mahalanobis2 = d^2, weight = omega.  A factorisation that fails, or a d^2 that is not finite,
 *      makes the frame CTAG_TRACK_SINGULAR (flags MEASURED, every other field 0 except rig and frame) and the track EMPTY.
 *   5. An unmeasured or gated frame while TRACKING: the prediction is the result and the new state, status OK, mahalanobis2 0, weight 1
 *      (unmeasured) or 0 (gated).  On the max_gap-th consecutive such frame the track goes to EMPTY and that frame is
 *      CTAG_TRACK_NOT_TRACKED (a gated one keeps its flags): measured frames at most max_gap indices apart stay one track, as in the
 *      smoother's rule 2.
 *   6. Record: rvec = Log(R), cov the pose block of P, vel_sigma the square roots of the diagonal of its velocity block.
 *   7. The predict calls give rule 3's prediction to time t (finite, above the last time given) for every rig, n_rigs records with
 *      frame 0, flags 0, weight 1, and leave the state and the filter's clock untouched.  An EMPTY track gives CTAG_TRACK_NOT_TRACKED.
 *   8. Deterministic and split-invariant.  Bad input apart, the bytes of a frame's record (the frame field excepted, which counts within
 *      the call) depend only on that rig's records and times up to that frame: not on how the frames were divided among calls, on g, on
 *      n_rigs, on the other rigs or on the run.  Every entry has one owner lane and one order of summation; no floating-point atomics.
 *   9. CTAG_ERR_ARG: a null argument (times and opts excepted), n_frames < 1, a wrong struct_size, an unknown loss, max_gap < 1, dt /
 *      q_rot / q_trans / vel0_sigma_rot / vel0_sigma_trans / loss_scale that are not positive and finite, a gate that is negative or
 *      not finite, times that are not finite and strictly increasing, a time that does not exceed the last one the filter was given
 *      (checked on the host: no device wait), n_frames x n_rigs above CTAG_TRACK_MAX_ITEMS.  A refused call changes nothing.
 *  10. Device memory: 1320 bytes per rig, owned by the filter; no per-item workspace.  One kernel launch per call, one wavefront a rig. */
#define CTAG_TRACK_FLAG_GATED 4u      /* rule 4: the measurement was refused by the gate */
#define CTAG_TRACK_FLAG_STARTED 8u    /* rule 2: the track starts at this frame */

typedef struct ctag_track_filter ctag_track_filter;

typedef struct ctag_track_filter_opts {
    uint32_t struct_size;    /* filled by ctag_track_filter_opts_default, checked */
    int32_t loss;            /* CTAG_TRACK_LOSS_NONE (default), CTAG_LOSS_HUBER or CTAG_LOSS_CAUCHY */
    int32_t max_gap;         /* >= 1; default 5 */
    int32_t reserved;        /* 0 */
    double dt;               /* seconds between frames when times == NULL; default 1 / 30 */
    double q_rot;            /* as ctag_track_opts, the same defaults */
    double q_trans;
    double vel0_sigma_rot;
    double vel0_sigma_trans;
    double loss_scale;
    double gate;             /* Mahalanobis norm above which a measurement is refused; 0 = off, the default: on hand-held motion at the default
                              * q every gate of 3 .. 8 refuses correctly decoded frames (tools/track_filter_study.py).
                              * The track noise fit below gives the q and the covariance scale of a recorded track, with which a gate is meant to be used. */
} ctag_track_filter_opts;    /* 72 bytes */

void ctag_track_filter_opts_default(ctag_track_filter_opts* opts);
/* The rig set only gives n_rigs.  opts == NULL means the defaults.  Several filters may live on one handle; each is freed before the
 * handle is destroyed.  Every track starts EMPTY. */
int ctag_track_filter_create(ctag_handle* h, const ctag_rigs* rigs, const ctag_track_filter_opts* opts, ctag_track_filter** filter);
void ctag_track_filter_free(ctag_track_filter* filter);
/* every track EMPTY again, the frame count 0 and no last time; enqueued */
int ctag_track_filter_reset(ctag_track_filter* filter);
/* Device records in, device records out, enqueued on the handle's stream behind whatever wrote the records; returns without waiting.
 * (The times of a call of more than one frame are staged in two buffers of the filter's in turn: such a call waits only if the one before
 * the previous one is still in flight.  A one-frame call never waits.) */
int ctag_rig_track_filter_device(ctag_track_filter* filter, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev, int n_frames,
                                 const double* times, ctag_track_rec* out_dev);
int ctag_mv_rig_track_filter_device(ctag_track_filter* filter, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev, int n_frames,
                                    const double* times, ctag_track_rec* out_dev);
/* The same with HOST arrays in and out; they wait for completion. */
int ctag_rig_track_filter(ctag_track_filter* filter, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                          ctag_track_rec* out);
int ctag_mv_rig_track_filter(ctag_track_filter* filter, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames, const double* times,
                             ctag_track_rec* out);
/* rule 7: n_rigs records to out_dev (enqueued) / to out (waits) */
int ctag_track_filter_predict_device(ctag_track_filter* filter, double t, ctag_track_rec* out_dev);
int ctag_track_filter_predict(ctag_track_filter* filter, double t, ctag_track_rec* out);
/* device time of the filter's last step call's kernel (needs CTAG_OPT_TIMING), milliseconds */
int ctag_track_filter_last_ms(ctag_track_filter* filter, float* out1);
/* From the next call on the filter reads every cov_f (rules 2 and 4) as s * cov_f; rule 1 still judges cov_f itself.  s must be positive and
 * finite, else CTAG_ERR_ARG and nothing changes.  The default is 1, and x * 1.0 is exact: a filter that never calls this produces the
 * bytes it always produced.  The scale is what the track noise fit below returns as cov_scale. */
int ctag_track_filter_set_cov_scale(ctag_track_filter* filter, double s);

/* ---- track noise fit: the filter's two process-noise densities and the covariance scale from a recorded track (k_track_noise.hip) ---------
 * The smoother and the filter take q_rot and q_trans from the caller and trust the covariance records' scale.  This call fits the three
 * numbers from a recorded batch by maximum likelihood on the filter's own innovations.  The batch has the filter's layout (record
 * w = f * n_rigs + g, rig and frame fields equal to their place; times a HOST array of n_frames finite, strictly increasing doubles, copied
 * before the call returns, or NULL for t = f * opts.dt).  A candidate is theta = (q_rot, q_trans, s).
 *   1. Measured and bad input are the filter's rule 1 (the same functions, on cov_f itself).  A rig with a bad record is
 *      CTAG_NOISE_BAD_INPUT: its score entries are 0 apart from the status.
 *   2. The score L_g(theta) of rig g: run the filter's rules 2-5 from an EMPTY track over all frames in order, with no loss and no gate,
 *      the call's max_gap, vel0_sigma_rot and vel0_sigma_trans, q_rot and q_trans from theta, and every cov_f replaced by s * cov_f (at
 *      the start of a track, rule 2, as well as in rule 4).  At every rule-4 update add l_f = log det S_f + d^2_f, S_f = H P- H^T + s cov_f
 *      and d^2 rule 4's; log det S_f comes from rule 4's factorisation: sum_a log S_aa + 2 sum_j log L_jj, L the Cholesky factor of the
 *      unit-diagonal matrix (ctag_math.h's log64).  The sum runs in frame order and has one owner.  Beside L: n_terms, the number of
 *      updates; sum_m2, the sum of d^2; n_singular, the frames where rule 4 gives CTAG_TRACK_SINGULAR (such a frame empties the track as
 *      in the filter and adds nothing to the sums).
 *   3. The fit minimises L over the parameters named in free_mask; the others stay at their start values opts.q_rot, opts.q_trans,
 *      opts.cov_scale.  CTAG_NOISE_PER_RIG: n_rigs independent searches on L_g and n_rigs result records.  CTAG_NOISE_POOLED: one search on
 *      the sum of L_g (and of n_terms, sum_m2, n_singular) over the rigs that are not bad input, in rig order, and one record with rig -1;
 *      CTAG_NOISE_BAD_INPUT when every rig is.
 *   4. The search is a grid search in u = log2(value / start) per free axis, decided on the device, centre u = 0 at first.  Round
 *      r = 0 .. rounds - 1 evaluates 5 points per free axis, u = u_centre + k h_r for k = -2 .. 2 with h_r = span / 2^(r+1): 1, 5, 25 or
 *      125 candidates.  Candidate c has k_j = (c / 5^j) % 5 - 2 on the j-th free axis (axes in the order q_rot, q_trans, cov_scale; the
 *      first free axis is the lowest digit), value = start * exp64(u * ln 2).
 *   5. A candidate with n_singular > 0 is disqualified.  The round's winner is the smallest L, ties to the lowest index; it is the next
 *      centre.  The previous centre is among the candidates (all k_j = 0), so L never rises from round to round.
 *   6. Status.  CTAG_NOISE_BAD_INPUT (rule 1, rule 3): the start values, rounds 0, every other number 0.  CTAG_NOISE_TOO_FEW: n_terms at the start values (round 0's centre) is below min_terms; the values returned are the start
 *      values, score = score_start, n_terms and mean_m2 those of the start values, rounds 1.  CTAG_NOISE_SINGULAR: every candidate of
 *      some round was disqualified; the values returned are that round's centre, rounds counts that round, score, n_terms and mean_m2 are 0.
 *   7. Result, a ctag_track_noise_rec, when the status is CTAG_NOISE_OK: the last round's winner's values, score = L and n_terms there,
 *      mean_m2 = sum_m2 / n_terms (about 6 when the filter is consistent), score_start = L at the start values, rounds = opts.rounds.
 *      flags: CTAG_NOISE_FLAG_EDGE << axis when the last round's winner lies at k = -2 or 2 on that axis.  log2_sigma[axis]: from the last
 *      round's grid, c = ((L+ - 2 L0) + L-) / h^2 along the axis through the winner, sigma = sqrt(2 / c) in octaves; 0 where the axis is
 *      fixed, the winner is at an edge, a neighbour was disqualified or c <= 0.
 *   8. Trace (optional, NULL allowed): rounds records per search, ctag_track_noise_round, row search * rounds + r: the winner's u and
 *      value, its L and its index; a round that was not evaluated, or had no winner, has winner -1 and every other field 0.
 *   9. Deterministic: the bytes of a per-rig record depend only on that rig's records, the times and the options (not on g apart from
 *      the rig field, on n_rigs or on the other rigs); the pooled search of a one-rig batch gives the per-rig bytes apart from rig.
 *  10. CTAG_ERR_ARG: the filter's rule-9 cases (null argument, times and opts and trace excepted; n_frames < 1; struct_size; max_gap < 1;
 *      dt, q_rot, q_trans, cov_scale, vel0_sigma_rot, vel0_sigma_trans not positive and finite; times not finite and strictly increasing;
 *      n_frames x n_rigs above CTAG_TRACK_MAX_ITEMS), an unknown mode, a free_mask outside 0 .. 7, rounds outside 1 .. 16, min_terms < 1,
 *      a span that is not positive and finite, n_cand outside 1 .. CTAG_NOISE_MAX_SCORE_CAND or a candidate value that is not positive
 *      and finite in a score call.  A free_mask of 0 is legal: one candidate, and the record carries the scores of the start values.
 *  11. One wavefront per (candidate, rig) item: k_track_noise walks the frames as the filter does and keeps four sums; one small launch
 *      per round (k_track_noise_select) makes the pooled sums and the argmin and writes the next candidates.  Nothing waits on the host.
 * Using the result.  The filter: q_rot and q_trans into ctag_track_filter_opts, cov_scale through ctag_track_filter_set_cov_scale; then a
 * gate is usable.  The smoother has no scale of its own and needs none: its poses depend only on q / s, so a caller
 * passes q_rot / s and q_trans / s in ctag_track_opts and multiplies the returned cov by s and vel_sigma by sqrt(s). */
#define CTAG_NOISE_OK 0
#define CTAG_NOISE_BAD_INPUT 1
#define CTAG_NOISE_TOO_FEW 2
#define CTAG_NOISE_SINGULAR 3

#define CTAG_NOISE_PER_RIG 0
#define CTAG_NOISE_POOLED 1

#define CTAG_NOISE_FREE_Q_ROT 1
#define CTAG_NOISE_FREE_Q_TRANS 2
#define CTAG_NOISE_FREE_COV_SCALE 4

#define CTAG_NOISE_FLAG_EDGE 1u          /* << axis: 0 q_rot, 1 q_trans, 2 cov_scale */
#define CTAG_NOISE_MAX_SCORE_CAND 64     /* candidates of one score call */

typedef struct ctag_track_noise_opts {
    uint32_t struct_size;    /* filled by ctag_track_noise_opts_default, checked */
    int32_t mode;            /* CTAG_NOISE_PER_RIG (default) or CTAG_NOISE_POOLED */
    int32_t free_mask;       /* CTAG_NOISE_FREE_*, 0 .. 7; default 7 */
    int32_t rounds;          /* 1 .. 16; default 10 */
    int32_t max_gap;         /* >= 1; default 5 */
    int32_t min_terms;       /* >= 1; default 8 */
    double dt;               /* seconds between frames when times == NULL; default 1 / 30 */
    double q_rot;            /* the start values; defaults 0.1, 3000 and 1 */
    double q_trans;
    double cov_scale;
    double vel0_sigma_rot;   /* as ctag_track_filter_opts, the same defaults */
    double vel0_sigma_trans;
    double span;             /* octaves; round 0 reaches from -span / 2 to span / 2 around the start; default 16 */
} ctag_track_noise_opts;     /* 80 bytes */

typedef struct ctag_track_noise_rec {
    int32_t status;          /* CTAG_NOISE_* */
    int32_t rig;             /* -1 for the pooled search */
    int32_t n_terms;
    int32_t n_free;
    int32_t rounds;          /* rounds evaluated */
    uint32_t flags;          /* CTAG_NOISE_FLAG_EDGE << axis */
    double q_rot;
    double q_trans;
    double cov_scale;
    double log2_sigma[3];    /* rule 7 */
    double score;
    double score_start;
    double mean_m2;
} ctag_track_noise_rec;      /* 96 bytes */

typedef struct ctag_track_noise_round {   /* rule 8 */
    double u[3];
    double value[3];
    double L;
    int32_t winner;
    int32_t reserved;        /* 0 */
} ctag_track_noise_round;    /* 64 bytes */

typedef struct ctag_track_noise_score {   /* rule 2: entry cand * n_rigs + g of a score call */
    double L;
    double sum_m2;
    int32_t n_terms;
    int32_t n_singular;
    int32_t status;          /* CTAG_NOISE_OK or CTAG_NOISE_BAD_INPUT */
    int32_t reserved;        /* 0 */
} ctag_track_noise_score;    /* 32 bytes */

void ctag_track_noise_opts_default(ctag_track_noise_opts* opts);
/* Device records in; n_rigs (per rig) or 1 (pooled) device result records to out_dev and, when trace_dev is not NULL, rounds trace records per
 * search, and no byte outside them.  Every round is enqueued on the handle's stream; the call returns without waiting for its own work
 * or for anything else on the stream, with one exception: the workspace is the handle's and grow-only, so an earlier noise call of this
 * handle that is still in flight is waited for first.  The rig set only gives n_rigs.  opts == NULL means the defaults. */
int ctag_rig_track_noise_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                    int n_frames, const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out_dev,
                                    ctag_track_noise_round* trace_dev);
int ctag_mv_rig_track_noise_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                       int n_frames, const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out_dev,
                                       ctag_track_noise_round* trace_dev);
/* The same with HOST arrays in and out; they wait for completion. */
int ctag_rig_track_noise_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                             const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out, ctag_track_noise_round* trace);
int ctag_mv_rig_track_noise_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                                const double* times, const ctag_track_noise_opts* opts, ctag_track_noise_rec* out, ctag_track_noise_round* trace);
/* Rule 2 alone, at n_cand caller-given candidates: cand is a HOST array of n_cand x 3 doubles (q_rot, q_trans, s), copied before the call
 * returns; n_cand x n_rigs entries to out_dev (entry cand * n_rigs + g).  Of opts only max_gap, dt and the vel0 sigmas are used (the others
 * are still checked).  The tool for plotting a likelihood surface; enqueued like the fit. */
int ctag_rig_track_noise_score_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                      int n_frames, const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand,
                                      ctag_track_noise_score* out_dev);
int ctag_mv_rig_track_noise_score_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                         int n_frames, const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand,
                                         ctag_track_noise_score* out_dev);
int ctag_rig_track_noise_score(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                               const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand, ctag_track_noise_score* out);
int ctag_mv_rig_track_noise_score(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                                  const double* times, const ctag_track_noise_opts* opts, const double* cand, int n_cand, ctag_track_noise_score* out);
/* device time of the last noise call's kernels, fit or score (needs CTAG_OPT_TIMING), milliseconds */
int ctag_track_noise_last_ms(ctag_handle* h, float* out1);

/* ---- hand-eye calibration: the two fixed transforms between the camera's poses and a robot's link poses (k_hand_eye.hip) -----------------
 * Every pose above lives in the camera's (or the reference) frame.  A robot, stage or tracked arm reports a link pose per frame; this call
 * takes the n_frames x n_rigs rig pose records of a batch (record w = f * n_rigs + g, either record kind, as the smoother takes them) with
 * their covariance records and one link pose per frame, and returns per rig the two fixed transforms P and Q of
 *      A_f ~ P o C_f o Q,        X_cam = R_P (R_C (R_Q X_rig + t_Q) + t_C) + t_P,
 * A_f the measured pose (camera or reference frame <- rig) and C_f the link pose as the mode says.  links: a HOST array of n_frames
 * ctag_link_pose, link_f = base <- gripper.
 *      CTAG_HAND_EYE_CAMERA_ON_LINK (eye in hand): C_f = link_f^-1, P = camera <- gripper, Q = base <- rig;
 *      CTAG_HAND_EYE_RIG_ON_LINK (eye to hand):    C_f = link_f,    P = camera <- base,    Q = gripper <- rig.
 * One kernel path serves both: the mode only decides whether the links are inverted when they are taken in.  Every rig g is one
 * independent problem; all problems of a call share the link poses.  This is OpenCV's calibrateHandEye / calibrateRobotWorldHandEye
 * with every frame weighted by its own covariance, and the answer comes with a covariance of its own.  Nothing above is changed by it.
 *   1. Used frames.  Frame f is used for rig g when it is measured exactly as rule 1 of the smoother says (pose CTAG_POSE_OK, covariance
 *      CTAG_COV_OK with param CTAG_COV_PARAM_TANGENT, unit-diagonal scaling, every pivot above 1e-12; W_f = cov^-1) and all six entries
 *      of its link pose are finite.  A link pose with a non-finite entry makes the frame unused for every rig: that is how a caller
 *      drops a frame.  Bad input is what it is for the smoother (a CTAG_COV_OK covariance with param CTAG_COV_PARAM_RVEC, a rig or
 *      frame field that is not the record's place): CTAG_HE_BAD_INPUT for that rig only.
 *   2. Unknowns: (a, b, c, d), 12 tangent coordinates.  R_P <- Exp(a) R_P, t_P <- t_P + b, R_Q <- Exp(c) R_Q, t_Q <- t_Q + d.
 *   3. Cost = half the sum over the used frames of rho(e^T W_f e), e = [Log(R_pred Rm_f^T); t_pred - tm_f].  rho is the identity for
 *      CTAG_TRACK_LOSS_NONE and ctag_loss.h's Huber or Cauchy with a = loss_scale otherwise: the function and the use of the smoother's
 *      rule 4.  The link poses are taken as exact.
 *   4. Jacobian, exact.  Rotation rows: Jl^-1(phi) for a, Jl^-1(phi) R_P R_C for c, phi = the rotation residual.  Translation rows:
 *      -[R_P (R_C t_Q + t_C)]x for a, I for b, R_P R_C for d.
 *   5. Start, on the device, from the used frames in frame order, k0 the first used frame.  S = sum_k alpha_k beta_k^T with
 *      alpha_k = Log(Rm_k Rm_k0^T), beta_k = Log(R_C,k R_C,k0^T); pairs in which |alpha| or |beta| exceeds 3 rad are left out of S (Log's
 *      branch next to a half turn is not stable under noise) but stay in the cost.  R_P is the rotation nearest S (svd3, the determinant
 *      fixed, as rule 2 of the camera-set fit); R_Q the rotation nearest sum_f R_C,f^T R_P^T Rm_f; (t_Q, t_P) solve the 6x6 normal
 *      equations of [R_P R_C,f | I] [t_Q; t_P] = tm_f - R_P t_C,f by Cholesky.
 *   6. Minimisation: Levenberg-Marquardt, (A + lambda diag A) delta = -g, the loss by its weight alone.  One lambda per problem from
 *      lambda0; the round control is the fits' (ctag_lm.h: rel_tol 1e-12, lambda_max 1e6, max_iterations), decided on the device, so
 *      the call does not wait.  A round whose factorisation meets a pivot that is not positive is a reject.  Problems that have
 *      stopped skip their rounds.  max_iterations = 1 with lambda0 = 0 is one undamped Gauss-Newton step from the start of rule 5.
 *   7. Status per problem: CTAG_HE_OK; CTAG_HE_TOO_FEW, fewer than 3 used frames; CTAG_HE_BAD_INPUT (rule 1); CTAG_HE_SINGULAR when
 *      the start's 6x6 meets a pivot that is not positive, when the cost is not finite, or when the undamped Gauss-Newton matrix at
 *      the returned state, scaled to unit diagonal, has a Cholesky pivot that is not above 1e-12: link rotations that are all about
 *      one axis, and pure translations.  On singular P and Q are the last accepted state (0 when the start itself failed) and cov is 0.
 *   8. Result: ctag_hand_eye_rec, one per rig.  dof = 6 n_used - 12; sigma2_hat = 2 cost / dof (0 when dof <= 0); min_pivot the smallest
 *      pivot of the scaled matrix; cov the inverse of the undamped Gauss-Newton matrix at the returned state in rule 2's coordinates
 *      and order, symmetric bit for bit, NOT scaled by sigma2_hat: the input covariances already carry the noise.  A problem that is
 *      CTAG_HE_TOO_FEW or CTAG_HE_BAD_INPUT has every field 0 except status and rig (and n_used for TOO_FEW).  ctag_hand_eye_frame_rec,
 *      optional, row f * n_rigs + g: for a used frame of a problem that has a state (CTAG_HE_OK, or singular at the returned state)
 *      the problem's status, CTAG_HE_FLAG_USED, the residual e, mahalanobis2 = e^T W_f e and weight = rho' at the returned state, and
 *      CTAG_HE_FLAG_DOWNWEIGHTED when a loss is set and mahalanobis2 exceeds loss_scale^2: there Huber's weight falls below 1 and
 *      Cauchy's, which is below 1 at every frame, below 1/2.  n_downweighted counts those frames.  Every other frame record is 0 except rig and frame.
 *   9. Deterministic.  Every sum over frames is taken in chunks of 64 consecutive frame indices, lane = frame mod 64, unused frames
 *      adding exact zeros, by wave_sum_f64's tree; the chunks are added in ascending order by one owner.  No floating-point atomics.
 *      A problem's bytes do not depend on its rig slot, on the other rigs, on the grid or on the run.
 *  10. CTAG_ERR_ARG: a null argument (frames_dev / frames excepted), n_frames < 1, a wrong struct_size, an unknown mode or loss,
 *      loss_scale that is not positive and finite, lambda0 that is negative or not finite, max_iterations < 1, n_frames x n_rigs above
 *      CTAG_HAND_EYE_MAX_ITEMS.  Device memory of one call: 452 bytes per (frame, rig) item, 144 per frame, 744 per chunk of 64 frames
 *      of a rig and 432 per rig; at most 1772 bytes per item (one-frame rigs), 0.12 GB at the bound. */
#define CTAG_HE_OK 0
#define CTAG_HE_TOO_FEW 1     /* rule 7 */
#define CTAG_HE_BAD_INPUT 2   /* rule 1 */
#define CTAG_HE_SINGULAR 3    /* rule 7 */

#define CTAG_HAND_EYE_CAMERA_ON_LINK 0   /* eye-in-hand: link = base<-gripper; the library uses C_f = link_f^-1 */
#define CTAG_HAND_EYE_RIG_ON_LINK 1      /* eye-to-hand: link = base<-gripper; C_f = link_f */
#define CTAG_HAND_EYE_MAX_ITEMS 65536    /* n_frames x n_rigs of one call */

#define CTAG_HE_FLAG_USED 1u          /* rule 1 */
#define CTAG_HE_FLAG_DOWNWEIGHTED 2u  /* a loss is set and the frame lies beyond its scale at the returned state: rule 8; NOT the smoother's "weight below 1" */

typedef struct ctag_link_pose { double rvec[3], tvec[3]; } ctag_link_pose;   /* 48 bytes: X_out = R(rvec) X_in + tvec */

typedef struct ctag_hand_eye_opts {
    uint32_t struct_size;    /* filled by ctag_hand_eye_opts_default, checked */
    int32_t mode;            /* CTAG_HAND_EYE_CAMERA_ON_LINK (default) or CTAG_HAND_EYE_RIG_ON_LINK */
    int32_t loss;            /* CTAG_TRACK_LOSS_NONE (default), CTAG_LOSS_HUBER or CTAG_LOSS_CAUCHY */
    int32_t max_iterations;  /* >= 1; default 20 */
    double loss_scale;       /* a of the loss, in units of the Mahalanobis norm; default 4 */
    double lambda0;          /* >= 0; default 1e-3 */
} ctag_hand_eye_opts;        /* 32 bytes */

typedef struct ctag_hand_eye_rec {   /* one per rig */
    int32_t status;          /* CTAG_HE_* */
    int32_t rig;
    int32_t n_used;
    int32_t n_downweighted;
    int32_t rounds;          /* accepted + rejected */
    int32_t dof;             /* 6 n_used - 12 */
    ctag_link_pose P, Q;     /* the mode's table above */
    double cost0;            /* at the start of rule 5 */
    double cost;             /* at the returned state */
    double lambda;
    double sigma2_hat;
    double min_pivot;
    double cov[144];         /* rule 8; rows/cols a, b, c, d */
} ctag_hand_eye_rec;         /* 1312 bytes */

typedef struct ctag_hand_eye_frame_rec {
    int32_t status;          /* the problem's, where the frame is used */
    int32_t rig;
    int32_t frame;
    uint32_t flags;          /* CTAG_HE_FLAG_* */
    double e[6];             /* rule 3's residual at the returned state: rotation, translation */
    double mahalanobis2;
    double weight;
} ctag_hand_eye_frame_rec;   /* 80 bytes */

void ctag_hand_eye_opts_default(ctag_hand_eye_opts* opts);
/* Device records in, device records out.  Writes exactly n_rigs result records to out_dev and, unless frames_dev is NULL,
 * n_frames x n_rigs frame records to frames_dev, and no byte outside them.  Enqueued on the handle's stream; returns without waiting for
 * its own work or for anything else on the stream, with one exception: the workspace is the handle's, so an earlier hand-eye call of
 * this handle that is still in flight is waited for first.  links is copied before the call returns.  The rig set only gives n_rigs.
 * opts == NULL means the defaults. */
int ctag_rig_hand_eye_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                 int n_frames, const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out_dev,
                                 ctag_hand_eye_frame_rec* frames_dev);
int ctag_mv_rig_hand_eye_fit_device(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses_dev, const ctag_pose_cov_rec* cov_dev,
                                    int n_frames, const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out_dev,
                                    ctag_hand_eye_frame_rec* frames_dev);
/* The same with HOST arrays in and out (frames may be NULL); they wait for completion. */
int ctag_rig_hand_eye_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_rig_pose_rec* rig_poses, const ctag_pose_cov_rec* cov, int n_frames,
                          const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out, ctag_hand_eye_frame_rec* frames);
int ctag_mv_rig_hand_eye_fit(ctag_handle* h, const ctag_rigs* rigs, const ctag_mv_pose_rec* mv_poses, const ctag_pose_cov_rec* cov, int n_frames,
                             const ctag_link_pose* links, const ctag_hand_eye_opts* opts, ctag_hand_eye_rec* out, ctag_hand_eye_frame_rec* frames);
/* device time of the last hand-eye call's kernels (needs CTAG_OPT_TIMING), milliseconds: gather + start, the rounds, the covariance and
 * the records, the whole call */
int ctag_hand_eye_last_ms(ctag_handle* h, float* out4);

/* ---- model reconstruction: the corner lists themselves, from detections of the objects (k_model_fit.hip) ---------------------------
 * Every pose call above takes a ctag_model; this call makes one.  From the detection records of a few dozen to a few thousand
 * frames and a rough seed model (an ideal cylinder of nominal radius, cylindertag_amd/models.py, or an older model) it returns the
 * model that minimises the reprojection error over all of them.  The problem over corners AND per-record poses separates: given the
 * model every record's pose is the solve ctag_pose_batch_device already does, so only the corners are optimised, by
 * Levenberg-Marquardt on the cost with the poses eliminated (the Schur complement on the 6x6 pose blocks).  Models are
 * independent problems (a pose record belongs to one model): each has its own lambda, accept / reject and stop, inside the same
 * launches.
 *   1. Observations.  Every marker of every CTAG_OK frame whose pose record under the SEED (ctag_pose_batch_device) has status
 *      CTAG_POSE_OK, in record order; its correspondences are the builder's (the end-feature skip, corners 0 1 4 5 [2 3 6 7]), its
 *      image points undistorted as PoseBA does.  The set is fixed for the whole call.  Two markers with the same model in one
 *      frame are two records.  A record in which two features claim the same model position (hand-built records only) is left out.
 *   2. Held corners.  A corner of a model observed by fewer than min_obs records is held: it keeps the seed's value and leaves the
 *      system; in the pose of a record that does see it, it still takes part with the seed's value.  A model with no fitted corner is
 *      returned unchanged with status CTAG_POSE_NOT_SEEN.
 *   3. Working model.  float32, as ctag_model stores it and every consumer reads it.  A trial step is computed in double, mapped
 *      by the gauge of rule 5 and rounded to float; the cost compared and reported is the cost of exactly those floats:
 *      stats.cost is the sum, in record order, of the cost fields ctag_pose_batch_device gives the observation records on the
 *      returned model, byte for byte.
 *   4. A round for model m.  All observation records are re-solved by the pose arithmetic (EPnP start included) on the trial
 *      model; cost[m] = the sum of their cost in record order (a record that is no longer CTAG_POSE_OK makes the trial a reject).
 *      The trial is accepted iff cost[m] decreases; on accept lambda <- max(lambda / 3, 1e-9), on reject lambda <- 4 lambda.  Reduced
 *      normal equations at the accepted state, residual r and Jacobians Jp (pose: rvec, tvec, as CTAG_COV_PARAM_RVEC has them) and Jx
 *      (the point) per point i of a record:  U = sum Jp_i^T Jp_i,  U = L L^T,  Z_i = L^-1 (Jp_i^T Jx_i),  y = L^-1 sum Jp_i^T r_i;
 *      S = sum over records [ diag(Jx_i^T Jx_i) - Z^T Z ],  g = sum over records [ Jx_i^T r_i - Z_i^T y ]  on the fitted corners.
 *      The step solves (S + lambda diag S) delta = -g by Cholesky; a pivot that is not positive counts as a reject.  Model m stops
 *      when an accepted round lowers the cost by less than rel_tol * cost, when lambda exceeds lambda_max, or after max_rounds.
 *   5. Gauge.  One camera cannot see the model's similarity (rotation, translation, scale: 7 degrees of freedom).  The fitted
 *      corners of every trial are mapped by the similarity (Umeyama) that best carries them onto the seed's same corners, on the
 *      host in double.  base, axis and marker_id are the seed's.
 *   6. Metric scale.  strip_height > 0: each fitted model is finally scaled about the centroid of its fitted corners so that the
 *      mean length of the strip's straight vertical edges -- corner pairs (0,5) and (1,4) of every feature whose four ends were
 *      fitted -- is strip_height; base moves with the scaling.  stats.cost is then the cost of the scaled model (rule 3).
 *   7. Determinism.  Every sum has a fixed order: record order across records, wave_sum_f64's tree inside one.  Two calls on the
 *      same input return the same bytes, and the result does not depend on how many records one pass of the workspace holds.
 *   8. CTAG_ERR_ARG: a null argument, n_frames < 1, max_rounds < 0, min_obs < 1, lambda0 / lambda_max / rel_tol that are not
 *      positive and finite, a strip_height that is not finite, a seed whose model_size is not the handle's dictionary's column
 *      count or is above 20 (CTAG_POSE_MAX_POINTS corners); CTAG_ERR_UNSUPPORTED: a camera the pose back end does not handle.
 * Device memory of one call: the pose records, 216 bytes (27 doubles: Z 18, Jx^T Jx 6, g 3) per model corner per observation
 * record of a pass -- 34 560 bytes a record at 160 corners, at most 2048 records a pass -- and 2 x (24 model_size)^2 doubles per
 * model for S and the damped system (3.7 MB at 160 corners). */
typedef struct ctag_model_fit_opts {
    int32_t max_rounds;   /* default 30 */
    int32_t min_obs;      /* default 2 */
    double lambda0;       /* default 1e-3 */
    double lambda_max;    /* default 1e6 */
    double rel_tol;       /* default 2.416e-7: 4 x the relative cost change float32 rounding of the model alone causes (6.04e-8) */
    double strip_height;  /* default 0: no metric scaling */
} ctag_model_fit_opts;

typedef struct ctag_model_fit_stat {
    int32_t status;           /* CTAG_POSE_OK or CTAG_POSE_NOT_SEEN */
    int32_t n_records;        /* observation records of this model */
    int32_t n_points_fitted;  /* corners in the system */
    int32_t n_points_held;    /* corners held at the seed */
    int32_t rounds;           /* rounds taken (accepted + rejected) */
    int32_t reserved;         /* 0 */
    double cost0;             /* cost at the seed */
    double cost;              /* cost of the returned model */
    double lambda;            /* lambda when the model stopped */
    double rms_px;            /* sqrt(2 cost / points of the observation records) */
} ctag_model_fit_stat;        /* 56 bytes */

void ctag_model_fit_opts_default(ctag_model_fit_opts* opts);
/* results_dev: n_frames detection records in DEVICE memory.  *out: a new model (ctag_model_free); stats: n_models HOST records.
 * opts == NULL means the defaults.  Waits for completion: the outer loop decides on the host. */
int ctag_model_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* seed,
                          const ctag_camera* camera, const ctag_model_fit_opts* opts, ctag_model** out, ctag_model_fit_stat* stats);
/* The same from HOST records: uploads them, then ctag_model_fit_device. */
int ctag_model_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* seed, const ctag_camera* camera,
                   const ctag_model_fit_opts* opts, ctag_model** out, ctag_model_fit_stat* stats);
/* Writes the .model text format of CylinderTag.cpp:168-188; floats with 9 significant digits, so that ctag_model_load returns the
 * same float bits.  Host only. */
int ctag_model_save(const ctag_model* m, const char* path);
/* device time of the last fit call's kernels by kind (needs CTAG_OPT_TIMING), milliseconds: pose, record, assemble, solve */
int ctag_model_fit_last_ms(ctag_handle* h, float* out4);

/* ---- rig assembly: the models of one rig into one common frame, from detections (k_rig_fit.hip) ------------------------------------
 * ctag_model_fit returns every model in its own frame (rule 5 there pins it to its seed); the rig and multi-view calls need the
 * models of a rig in ONE frame.  From the detection records of frames that show two or more markers of a rig together this call
 * computes the rigid transform that carries each member model into the rig's frame -- the frame of one of its models, the anchor --
 * and returns the assembled model.  The problem over member transforms AND per-frame rig poses separates: given the transforms a
 * frame's rig pose is the solve ctag_rig_pose_batch_device already does, so only the transforms are optimised, by
 * Levenberg-Marquardt on the cost with the rig poses eliminated (the Schur complement on the 6x6 pose blocks).  Rigs are
 * independent problems: each has its own lambda, accept / reject and stop, inside the same launches.
 *   1. Per-marker poses.  The poses of ctag_pose_batch_device under `in` are computed once, before the first round.  A frame that is not CTAG_OK and a record that is not CTAG_POSE_OK
 *      contribute nothing.  Of two markers of a frame with one model index only the first counts (the rig section's duplicate rule:
 *      the first marker with a model index claims it, whether or not its pose counts).
 *   2. Initial assembly, per rig, on the host in double from those pose records (R_m, t_m of model m in a frame).  n(a,b) = the
 *      number of frames in which models a and b of the rig both have a counted pose.  Anchor = the lowest model index of the rig
 *      with any n(a,.) >= min_frames.  A tree grows from it: repeatedly the unplaced model b with the largest n(a,b) to a placed
 *      model a is added with parent a (ties: the lowest b, then the lowest a) until no such count reaches min_frames.  The edge
 *      transform X_a = E X_b has as rotation the rotation nearest (SVD, determinant fixed) to the sum, in frame order, of
 *      R_a^T R_b and as translation the mean, in frame order, of R_a^T (t_b - t_a);  T_b = T_a o E.  model_stats' parent and
 *      n_frames_with_parent report the tree.  Unplaced models -- never seen often enough with the rig, in no rig -- keep their
 *      corners and get status CTAG_POSE_NOT_SEEN; a rig with no anchor gets status CTAG_POSE_NOT_SEEN.
 *   3. Working model.  float32, as every consumer reads it.  A state applies the transforms X_rig = R X_in + t to `in`'s float
 *      corners in double and rounds to float; base moves as a point, axis rotates only.  The anchor's transform is exactly the
 *      identity and is skipped: its corners, base and axis are `in`'s bytes, as are an unplaced model's.  marker_id and model_size
 *      are `in`'s.
 *   4. Observation set.  The (frame, rig) items whose ctag_rig_pose_rec on the initial assembly is CTAG_POSE_OK with n_members >= 2,
 *      where unplaced models are left out of their rig for the whole call (an internal rig_of_model copy has them at -1, so all
 *      members are placed).  The set is fixed for the call.  The cost of a state = the sum, in (frame, rig) order, of the cost
 *      field ctag_rig_pose_batch_device gives those items on that float model; stats.cost is that sum on the returned model byte
 *      for byte, cost_init the sum on the initial assembly.
 *   5. A round is Levenberg-Marquardt on the 6 (n_placed - 1) unknowns of a rig.  Update T_m <- Exp(d_m) T_m with d = (w, v) in
 *      the rig frame: R <- Exp(w) R, t <- Exp(w) t + v (Exp the Rodrigues formula).  Per point i of member m with rig-frame corner Y:
 *      Jm_i = (dr/dY) [-[Y]x | I] and Jp_i as CTAG_COV_PARAM_RVEC has it.  Per record: U = sum Jp^T Jp = L L^T, y = L^-1 sum Jp^T r,
 *      Z_m = L^-1 sum_{i in m} Jp^T Jm;  S_mm += sum Jm^T Jm - Z_m^T Z_m,  S_mn -= Z_m^T Z_n,  g_m += sum Jm^T r - Z_m^T y;  the
 *      anchor's rows are dropped.  The step solves (S + lambda diag S) d = -g by Cholesky; a pivot that is not positive is a reject.
 *      The trial is accepted iff the cost of rule 4 decreases; lambda <- max(lambda / 3, 1e-9) on accept, 4 lambda on reject.  A
 *      trial in which an observation record stops being CTAG_POSE_OK is a reject.  A rig stops when an accepted round lowers the
 *      cost by less than rel_tol * cost, when lambda exceeds lambda_max, or after max_rounds; max_rounds = 0 returns the initial
 *      assembly.
 *   6. Determinism.  Every sum has a fixed order: record order across records, wave_sum_f64's tree inside one.  Two calls return
 *      the same bytes, and the result does not depend on the pass size of the workspace or on the grid.
 *   7. CTAG_ERR_ARG: a null argument, n_frames < 1, max_rounds < 0, min_frames < 1, lambda0 / lambda_max / rel_tol that are not
 *      positive and finite, an `in` whose model_size is not the handle's dictionary's column count or is above 20, a `rigs` made
 *      for another n_models, a rig of more than CTAG_RIG_FIT_MAX_MODELS models; CTAG_ERR_UNSUPPORTED: a camera the pose back end
 *      does not handle.
 * Device memory of one call: the pose records of both kinds, 63 doubles (Z 36, Jm^T Jm 21, g 6) per member slot -- 8064 bytes per
 * observation record of a pass, at most 512 records a pass -- and 96 x 96 doubles per rig for S. */
#define CTAG_RIG_FIT_MAX_MODELS 16   /* member models of one rig the assembly takes */
typedef struct ctag_rig_fit_opts {
    int32_t max_rounds;   /* default 30 */
    int32_t min_frames;   /* default 2 */
    double lambda0;       /* default 1e-3 */
    double lambda_max;    /* default 1e6 */
    double rel_tol;       /* default 2.479e-5: 4 x the relative cost change float32 rounding of the model alone causes (6.198e-6) */
} ctag_rig_fit_opts;

typedef struct ctag_rig_fit_stat {        /* one per rig */
    int32_t status;       /* CTAG_POSE_OK or CTAG_POSE_NOT_SEEN */
    int32_t anchor;       /* model index, -1 without one */
    int32_t n_placed;     /* models in the rig's frame, the anchor included */
    int32_t n_unplaced;   /* models of the rig left out (rule 2) */
    int32_t n_records;    /* observation records (rule 4) */
    int32_t n_points;     /* correspondences of those records */
    int32_t rounds;       /* rounds taken (accepted + rejected) */
    int32_t reserved;     /* 0 */
    double cost_init;     /* cost of the initial assembly */
    double cost;          /* cost of the returned model */
    double lambda;        /* lambda when the rig stopped */
    double rms_px;        /* sqrt(2 cost / n_points) */
} ctag_rig_fit_stat;      /* 64 bytes */

typedef struct ctag_rig_fit_model_stat {  /* one per model */
    int32_t status;       /* CTAG_POSE_OK (placed) or CTAG_POSE_NOT_SEEN */
    int32_t rig;          /* the rig set's entry for the model */
    int32_t parent;       /* rule 2's tree; -1 for an anchor and an unplaced model */
    int32_t n_frames_with_parent;
    int32_t n_records;    /* observation records the model is a member of */
    int32_t reserved;     /* 0 */
    double rvec[3], tvec[3];  /* X_rig = R(rvec) X_in + tvec; exactly 0 for an anchor and for models that did not move */
} ctag_rig_fit_model_stat;    /* 72 bytes */

void ctag_rig_fit_opts_default(ctag_rig_fit_opts* opts);
/* results_dev: n_frames detection records in DEVICE memory.  *out: a new model (ctag_model_free); rig_stats: n_rigs HOST records,
 * model_stats: n_models HOST records.  opts == NULL means the defaults.  Waits for completion: the outer loop decides on the host.
 * The rig calls take the result together with a rig set in which model_stats' CTAG_POSE_NOT_SEEN models are -1. */
int ctag_rig_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* in, const ctag_rigs* rigs,
                        const ctag_camera* camera, const ctag_rig_fit_opts* opts, ctag_model** out, ctag_rig_fit_stat* rig_stats,
                        ctag_rig_fit_model_stat* model_stats);
/* The same from HOST records: uploads them, then ctag_rig_fit_device. */
int ctag_rig_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* in, const ctag_rigs* rigs,
                 const ctag_camera* camera, const ctag_rig_fit_opts* opts, ctag_model** out, ctag_rig_fit_stat* rig_stats,
                 ctag_rig_fit_model_stat* model_stats);
/* device time of the last assembly's kernels by kind (needs CTAG_OPT_TIMING), milliseconds: marker pose, rig pose, record + assemble, solve */
int ctag_rig_fit_last_ms(ctag_handle* h, float* out4);

/* ---- camera set fit: the poses of the cameras of a set, from detections they share (k_cam_fit.hip) -----------------------------------
 * The multi-view call takes a ctag_camera_set; this call makes one.  Two to CTAG_MV_MAX_CAMERAS cameras with known intrinsics watch
 * one working volume; frame f of every camera is the same instant, and a rig of the rig set is carried through the volume.  The call
 * returns every camera's pose in the frame of one of them, the anchor.  The problem over camera poses AND the rig's pose at every
 * instant separates: given the camera poses an instant's rig pose is the solve ctag_mv_rig_pose_batch_device already does, so only the
 * camera poses are optimised, by Levenberg-Marquardt on the cost with the rig poses eliminated (the Schur complement on the 6x6 pose
 * blocks).  Intrinsics are an input and stay as given.  One problem per call.
 *   1. Per-camera rig poses.  ctag_rig_pose_batch_device runs once per camera, on that camera's records with its intrinsics, before
 *      the first round.  The record of (instant f, rig g) -- an item -- counts for the start in camera c when it is CTAG_POSE_OK with
 *      n_points >= min_points (a lone 4-corner marker ends in its mirrored minimum nine times in ten: DESIGN.md section 16).
 *   2. Initial assembly, on the host in double, from those records (R_c, t_c of the item in camera c).  n(a,b) = the number of items
 *      counted in both cameras a and b.  Anchor = the lowest camera index with any n(a,.) >= min_items.  A tree grows from it:
 *      repeatedly the unplaced camera b with the largest n(a,b) to a placed camera a is added with parent a (ties: the lowest b, then
 *      the lowest a) until no such count reaches min_items.  The edge X_b = E X_a has as rotation Rbar, the rotation nearest (SVD,
 *      determinant fixed) to the sum, in item order, of R_b R_a^T, and as translation the mean, in item order, of t_b - Rbar t_a;
 *      T_b = E o T_a.  The reference frame is the anchor camera's: its pose is exactly zero in the output and is never updated.
 *      Cameras the tree does not reach are unplaced: they leave the call (the multi-view solves of rules 3-4 run on the placed
 *      cameras only) and get status CTAG_POSE_NOT_SEEN and a zero pose; cam_stats carry the caller's camera indices.  Without an
 *      anchor the call's status is CTAG_POSE_NOT_SEEN and every camera is unplaced.
 *   3. Observation set.  The items whose ctag_mv_pose_rec on the initial set is CTAG_POSE_OK with n_cameras >= 2.  The set is fixed
 *      for the call.  The cost of a state = the sum, in item order, of the cost fields ctag_mv_rig_pose_batch_device gives those items
 *      under that state's camera set; stat.cost is that sum on the returned set byte for byte (the set made by
 *      ctag_camera_set_create from the placed cameras' intrinsics and cam_stats' poses, in camera order), cost_init the sum on the
 *      initial set.
 *   4. A round is Levenberg-Marquardt on the 6 (n_placed - 1) unknowns.  Update of camera c by d = (w, v) in its own frame:
 *      Rc <- Exp(w) Rc, tc <- Exp(w) tc + v (Exp the Rodrigues formula; the state is (rvec, tvec), rvec by the inverse formula).  Per
 *      point of camera c with Q = Rc (R X + t) + tc: Jc = (dr/dQ) [-[Q]x | I], Jp the point's derivative in the rig pose's
 *      (rvec, tvec) as stage 2 of the multi-view section forms it.  Per record: U = sum Jp^T Jp = L L^T, y = L^-1 sum Jp^T r,
 *      Z_c = L^-1 sum_{i in c} Jp^T Jc;  S_cc += sum Jc^T Jc - Z_c^T Z_c,  S_cd -= Z_c^T Z_d,  g_c += sum Jc^T r - Z_c^T y;  the
 *      anchor's rows are dropped.  The step solves (S + lambda diag S) d = -g by Cholesky; a pivot that is not positive is a reject.
 *      The trial is accepted iff the cost of rule 3 decreases; lambda <- max(lambda / 3, 1e-9) on accept, 4 lambda on reject.  A
 *      trial in which an observation record stops being CTAG_POSE_OK is a reject.  The call stops when an accepted round lowers the
 *      cost by less than rel_tol * cost, when lambda exceeds lambda_max, or after max_rounds; max_rounds = 0 returns the initial set.
 *   5. Determinism.  Every sum has a fixed order: record order across records, wave_sum_f64's tree inside one (lane l of one
 *      wavefront owns points l, l + 64, ... of the record).  Two calls return the same bytes, and the result does not depend on the
 *      pass size of the workspace or on the grid.
 *   6. CTAG_ERR_ARG: a null argument (a null entry of results_dev included), n_frames < 1, n_cameras outside
 *      2 .. CTAG_MV_MAX_CAMERAS, max_rounds < 0, min_items < 1, min_points < 1, lambda0 / lambda_max / rel_tol that are not positive
 *      and finite, a model whose model_size is not the handle's dictionary's column count or is above 20, a `rigs` made for another
 *      n_models; CTAG_ERR_UNSUPPORTED: a camera the pose back end does not handle.
 * Device memory of one call: the rig-pose records of one camera and the multi-view records, 63 doubles (Z 36, Jc^T Jc 21, g 6) per
 * camera slot -- 4032 bytes per observation record of a pass, at most 512 records a pass -- and 48 x 48 doubles for S. */
typedef struct ctag_camera_fit_opts {
    int32_t max_rounds;   /* default 30 */
    int32_t min_items;    /* default 2: (instant, rig) items a camera pair must share to become a tree edge */
    int32_t min_points;   /* default 8: a per-camera rig record counts for the start only from this many points */
    int32_t reserved;     /* 0 */
    double lambda0;       /* default 1e-3 */
    double lambda_max;    /* default 1e6 */
    double rel_tol;       /* default 6.14e-13: 4 x the relative cost change a one-ulp change of a camera pose causes through the inner solves (1.535e-13) */
} ctag_camera_fit_opts;   /* 40 bytes */

typedef struct ctag_camera_fit_stat {     /* one per call */
    int32_t status;       /* CTAG_POSE_OK or CTAG_POSE_NOT_SEEN (no anchor) */
    int32_t anchor;       /* camera index, -1 without one */
    int32_t n_placed;     /* cameras with a pose, the anchor included */
    int32_t n_unplaced;   /* cameras left out (rule 2) */
    int32_t n_records;    /* observation records (rule 3) */
    int32_t n_points;     /* correspondences of those records */
    int32_t rounds;       /* rounds taken (accepted + rejected) */
    int32_t reserved;     /* 0 */
    double cost_init;     /* cost of the initial set */
    double cost;          /* cost of the returned set */
    double lambda;        /* lambda when the call stopped */
    double rms_px;        /* sqrt(2 cost / n_points) */
} ctag_camera_fit_stat;   /* 64 bytes */

typedef struct ctag_camera_fit_cam_stat { /* one per camera */
    int32_t status;       /* CTAG_POSE_OK (placed) or CTAG_POSE_NOT_SEEN */
    int32_t parent;       /* rule 2's tree, a camera index; -1 for the anchor and an unplaced camera */
    int32_t n_items_with_parent;
    int32_t n_records;    /* observation records in which the camera has points */
    int32_t n_points;     /* its correspondences in them */
    int32_t reserved;     /* 0 */
    ctag_camera_pose pose; /* X_cam = R(rvec) X_anchor + tvec; exactly 0 for the anchor and for an unplaced camera */
} ctag_camera_fit_cam_stat; /* 72 bytes */

void ctag_camera_fit_opts_default(ctag_camera_fit_opts* opts);
/* results_dev: HOST array of n_cameras DEVICE pointers, n_frames records each (the multi-view call's layout); cameras: n_cameras
 * intrinsics.  *out: a new camera set (ctag_camera_set_free) when every camera is placed, NULL otherwise -- the call still returns
 * CTAG_OK and the placed poses are in cam_stats; *out is NULL after every error too.  stat: one HOST record, cam_stats: n_cameras
 * HOST records.  opts == NULL means the defaults.  Waits for completion: the outer loop decides on the host. */
int ctag_camera_fit_device(ctag_handle* h, const ctag_frame_result* const* results_dev, int n_cameras, int n_frames, const ctag_model* model,
                           const ctag_rigs* rigs, const ctag_camera* cameras, const ctag_camera_fit_opts* opts, ctag_camera_set** out,
                           ctag_camera_fit_stat* stat, ctag_camera_fit_cam_stat* cam_stats);
/* The same from n_cameras x n_frames HOST records, camera-major (record c * n_frames + f): uploads them, then ctag_camera_fit_device. */
int ctag_camera_fit(ctag_handle* h, const ctag_frame_result* results, int n_cameras, int n_frames, const ctag_model* model, const ctag_rigs* rigs,
                    const ctag_camera* cameras, const ctag_camera_fit_opts* opts, ctag_camera_set** out, ctag_camera_fit_stat* stat,
                    ctag_camera_fit_cam_stat* cam_stats);
/* device time of the last fit's kernels by kind (needs CTAG_OPT_TIMING), milliseconds: per-camera rig pose, multi-view pose, record + assemble, solve */
int ctag_camera_fit_last_ms(ctag_handle* h, float* out4);
/* Reads a camera set back: *n_cameras, and the intrinsics and poses it was created from (either array may be NULL; each holds
 * CTAG_MV_MAX_CAMERAS entries at most, n_cameras are written).  Host only. */
int ctag_camera_set_get(const ctag_camera_set* s, int* n_cameras, ctag_camera* cameras, ctag_camera_pose* poses);

/* ---- intrinsics fit: the camera itself, from detections of rigs whose models are known (k_intr_fit.hip) ------------------------------
 * Every pose call takes a ctag_camera; this call makes one from a rough seed.  A rig of the rig set (a one-marker rig is the special
 * case) is shown to ONE camera in many views; models and rig layout are inputs and stay as given.  The problem over the camera AND the
 * rig's pose in every view separates: given the camera a view's pose is a 6-parameter minimisation of its own, so only the camera's
 * parameters are optimised, by Levenberg-Marquardt on the cost with the view poses eliminated (the Schur complement on the 6x6 pose
 * blocks).  Parameter i of CTAG_INTR_PARAMS: fx fy cx cy = K[0] K[4] K[2] K[5], then dist[0..11] = k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4.
 *   1. Observations.  ctag_rig_pose_batch_device runs once under the SEED camera; its records, in record order f * n_rigs + g, are the
 *      seed pass.  A record is an observation when it is CTAG_POSE_OK with n_points >= min_points.  Its members, correspondences and
 *      point order are that record's (member_mask, the builder's order), and the set is fixed for the whole call.  The image point of
 *      a correspondence is the feature's corner AS DETECTED (float pixels), never undistorted.
 *   2. Cost: the forward reprojection error, what a camera calibration minimises.  Per point with P = R X + t, x = P0/P2, y = P1/P2,
 *      r2 = x^2 + y^2: rad = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
 *        xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2) + s1 r2 + s2 r2^2,   yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y + s3 r2 + s4 r2^2,
 *        r = (fx xd + cx - u, fy yd + cy - v)                          (cv::projectPoints' model without tilt, as the overlay has it);
 *      cost of a record = 0.5 sum |r|^2, cost of a state = the record costs summed in record order.  It is NOT the sum of the pose
 *      calls' cost fields: PoseBA's residual lives in the undistorted image, which shrinks or grows with the very coefficients being
 *      fitted (a camera that maps everything towards one point would win), and its observations are rounded to float, so that cost is
 *      not smooth in the camera.  stat.pose_cost is that sum all the same, byte for byte, over the observation records of ONE
 *      ctag_rig_pose_batch_device call under the returned camera -- for comparison only.  A point with P2 <= 0, a rational
 *      denominator that is not positive, or a value that is not finite makes the state unusable.
 *   3. Working camera.  ctag_camera is float32: a trial is formed in double (camera + delta) and rounded to float, and the cost that
 *      is compared and reported is the cost of exactly those floats, read back as every pose call reads a ctag_camera.  n_dist is the
 *      seed's; coefficients at or beyond n_dist are zero and cannot be free (CTAG_ERR_ARG).  K's other entries are the seed's.  A
 *      trial whose fx or fy is not positive and finite is unusable.
 *   4. View poses.  Given the camera, a record's pose is the minimiser of rule 2's cost over its own (rvec, tvec), additive in those six
 *      numbers (CTAG_COV_PARAM_RVEC's parametrisation), found by damped Gauss-Newton from the record's accepted pose (in round 0 the
 *      seed pass's): (U + mu diag U) d = -sum Jp^T r by Cholesky; mu starts at 1e-4, mu / 3 after an accepted step (the cost fell),
 *      4 mu after a rejected one (cost not lower, unusable trial, pivot not positive); at most 40 steps; it stops after an accepted
 *      step that lowers the cost by less than 1e-15 of it, at a cost of exactly 0, and when mu passes 1e8.  There is no EPnP restart:
 *      a restart moves small records between minima from one trial to the next (case (e)).  A record whose
 *      start is unusable makes the state unusable.
 *   5. A round.  At the accepted state, per point Jp (2 x 6, in rvec, tvec) and Jc (2 x 16, analytic; with tie_focal the fx column is
 *      dr/dfx + ratio dr/dfy, ratio = seed fy / seed fx).  Per record: U = sum Jp^T Jp = L L^T, Z = L^-1 sum Jp^T Jc,
 *      y = L^-1 sum Jp^T r, S_r = sum Jc^T Jc - Z^T Z, g_r = sum Jc^T r - Z^T y; S and g are the sums over the records in record
 *      order.  The step solves (S + lambda diag S) delta = -g over the free rows by Cholesky (fixed parameters are identity rows); a
 *      pivot that is not positive is a reject.  Trial = camera + delta (rule 3; a tied fy = ratio x the new fx), then the view poses
 *      (rule 4, from the accepted poses), then the cost.  The trial is accepted iff it is usable and its cost is lower;
 *      lambda <- max(lambda / 3, 1e-9) on accept, 4 lambda on reject.  The call stops when an accepted round lowers the cost by less
 *      than rel_tol x cost, when lambda exceeds lambda_max, or after max_rounds; max_rounds = 0 returns the seed with the view poses
 *      of rule 4 under it.
 *   6. Result.  *out is the accepted camera.  poses_out (n_frames x n_rigs, may be NULL): an observation's record carries the final
 *      rvec / tvec / cost under rule 2 with rvec0 / tvec0 / cost0 (and every other field) the seed pass's; every other record is the
 *      seed pass's unchanged.  stat.cost is the sum of the observations' cost fields in record order, cost0 the same after round 0's
 *      view poses under the seed.  sigma2_hat = 2 cost / (2 n_points - 6 n_records - n_free); sigma[i] = sqrt(sigma2_hat (S^-1)_ii)
 *      from the undamped S at the returned state over the free rows, on the host in double; 0 for a fixed parameter, ratio x
 *      sigma[fx] for a tied fy; all 0 when the system at the returned state cannot be formed or factored (a record flagged there, a
 *      pivot that is not positive).  A weak data set shows in them: a single marker cannot fix a principal point.
 *      Status: CTAG_POSE_NOT_SEEN (no observation), CTAG_POSE_TOO_FEW (2 n_points - 6 n_records <= n_free), CTAG_POSE_DEGENERATE (the
 *      seed state is unusable, or the undamped S has a pivot that is not positive at the start); *out is the seed in all three, and
 *      poses_out the seed pass.
 *   7. Determinism.  Every sum has a fixed order: record order across records; inside a record the points in point order for the
 *      sums of rule 5 (one owner lane per entry), lane l's points l, l + 64, ... then wave_sum_f64's tree for rule 4.  Two calls on
 *      the same input return the same bytes, and the result does not depend on the pass size of the workspace or on the grid.
 *   8. CTAG_ERR_ARG: a null argument (poses_out excepted), n_frames < 1, max_rounds < 0, min_points < 1, lambda0 / lambda_max / rel_tol
 *      that are not positive and finite, a free_mask bit at or above CTAG_INTR_PARAMS or on a coefficient at or beyond the seed's
 *      n_dist, no free parameter, a model whose model_size is not the handle's dictionary's column count or is above 20, a `rigs`
 *      made for another n_models; CTAG_ERR_UNSUPPORTED: a seed the pose back end does not handle; CTAG_ERR_LIMIT: n_frames x
 *      CTAG_MAX_MARKERS above 2^30 or n_frames x n_rigs above 2^28, and for the host entry n_frames above 2^24.
 * Out of scope: tilt terms, several cameras in one call, fitting models or layout together with the camera (alternate with
 * ctag_model_fit / ctag_rig_fit).  Device memory of one call: two sets of rig pose records, 152 doubles per observation record of a
 * pass (at most 512 records a pass), 16 x 16 doubles for S. */
#define CTAG_INTR_PARAMS 16

typedef struct ctag_intrinsics_fit_opts {
    int32_t max_rounds;   /* default 30 */
    int32_t min_points;   /* default 8: a rig record with fewer points is no observation */
    uint32_t free_mask;   /* bit i: parameter i is fitted; 0 = fx fy cx cy and the first min(seed n_dist, 12) coefficients */
    int32_t tie_focal;    /* != 0: fy = fx * (seed fy / seed fx), one unknown; bit 1 of free_mask is ignored */
    double lambda0;       /* default 1e-3 */
    double lambda_max;    /* default 1e6 */
    double rel_tol;       /* default 7.71e-9: 4 x the relative cost change a one-ulp move of one camera field causes at a returned state (1.928e-9) */
} ctag_intrinsics_fit_opts; /* 40 bytes */

typedef struct ctag_intrinsics_fit_stat {  /* one per call */
    int32_t status;       /* CTAG_POSE_OK, _NOT_SEEN, _TOO_FEW or _DEGENERATE (rule 6) */
    int32_t n_records;    /* observation records (rule 1) */
    int32_t n_points;     /* correspondences of those records */
    int32_t n_free;       /* unknowns of the camera */
    int32_t rounds;       /* rounds taken (accepted + rejected) */
    uint32_t free_mask;   /* the mask in use: the default resolved, bit 1 cleared under tie_focal */
    double cost0;         /* cost under the seed, view poses by rule 4 */
    double cost;          /* cost of the returned camera */
    double lambda;        /* lambda when the call stopped */
    double rms_px;        /* sqrt(2 cost / n_points) */
    double sigma2_hat;    /* rule 6 */
    double pose_cost;     /* rule 2: the pose back end's own cost under the returned camera, for comparison */
    double sigma[CTAG_INTR_PARAMS]; /* rule 6, in parameter order */
} ctag_intrinsics_fit_stat; /* 200 bytes */

void ctag_intrinsics_fit_opts_default(ctag_intrinsics_fit_opts* opts);
/* results_dev: n_frames detection records in DEVICE memory.  out, stat: HOST; poses_out: n_frames x n_rigs HOST records or NULL.
 * opts == NULL means the defaults.  Waits for completion: the outer loop decides on the host. */
int ctag_intrinsics_fit_device(ctag_handle* h, const ctag_frame_result* results_dev, int n_frames, const ctag_model* model, const ctag_rigs* rigs,
                               const ctag_camera* seed, const ctag_intrinsics_fit_opts* opts, ctag_camera* out, ctag_intrinsics_fit_stat* stat,
                               ctag_rig_pose_rec* poses_out);
/* The same from HOST records: uploads them, then ctag_intrinsics_fit_device. */
int ctag_intrinsics_fit(ctag_handle* h, const ctag_frame_result* results, int n_frames, const ctag_model* model, const ctag_rigs* rigs,
                        const ctag_camera* seed, const ctag_intrinsics_fit_opts* opts, ctag_camera* out, ctag_intrinsics_fit_stat* stat,
                        ctag_rig_pose_rec* poses_out);
/* device time of the last fit's kernels by kind (needs CTAG_OPT_TIMING), milliseconds: rig pose, view pose, record + assemble, solve */
int ctag_intrinsics_fit_last_ms(ctag_handle* h, float* out4);

/* ---- overlay: CylinderTag::drawAxis (reference CylinderTag.cpp:211-246) ------------------------------------------------
 * Output: 8-bit, 3 channels, every channel = the gray value (cvtColor GRAY2RGB), then per drawn record, in record order,
 * what the reference paints with OpenCV 4.5.3 (k_draw.hip restates it):
 *   model points: corners[pos_j*8 + k] of the record's model for feature j < n_features and k < 8, then base,
 *                 base + axis*L, base + (0.0372, 0.0372, 0.9986)*L, base + (0.9980, -0.0520, -0.0353)*L (float, L = axis_length);
 *   projectPoints with rvec, tvec, K and all 14 distortion terms, rounded to float, then to int (nearest, ties to even, saturated);
 *   filled circles of radius 5 in (255,234,32) at points 0 .. size-6 (the last corner is not drawn: the reference's size()-5 bound);
 *   arrowedLine(base, end_k, thickness 10, LINE_AA, tip 0.2) in (255,0,0), (0,255,0), (0,0,255); a filled circle of radius 8
 *   in (247,235,235) at the base.  Scalar component c lands in channel c.
 * Rules the reference leaves undefined:
 *   - a record draws only when status == CTAG_POSE_OK, its frame is the frame being drawn, its marker indexes a marker of that
 *     frame's CTAG_OK result, its model_index a model, and every feature j < n_features has j < n_pos and 0 <= pos < model_size
 *     (the reference reads out of bounds otherwise; CTAG_POSE_BAD_POS), with n_features <= CTAG_MAX_CODE_POS.  Any other
 *     record draws nothing, and nothing outside the records' own data is read.
 *   - a projected point that is not finite removes the primitives that use it (its circle; an arrow whose base or end it is;
 *     all three arrows and the base circle if it is the base).
 *   - a marker without features draws its axes only (the reference's size()-5 bound wraps around there).
 *   - integer arithmetic that would overflow in OpenCV's 32-bit Point is carried out in 64 bits (points beyond +-2^30 px only).
 * axis_length must lie in [0, 65536], rows and cols in [1, 32768]. */
#define CTAG_DRAW_MAX_SIDE 32768
#define CTAG_DRAW_MAX_AXIS_LENGTH 65536

/* One frame, host memory in and out.  gray: rows x cols, row_stride bytes apart.  Record k draws marker poses[k].marker of
 * *result with model poses[k].model_index; poses[k].frame must be 0.  out: rows rows of 3*cols bytes, out_row_stride
 * (>= 3*cols) bytes apart; the bytes between 3*cols and out_row_stride are not written.  Waits for completion. */
int ctag_draw_axis(ctag_handle* h, const uint8_t* gray, int rows, int cols, ptrdiff_t row_stride, const ctag_frame_result* result,
                   const ctag_pose_rec* poses, int n_poses, const ctag_model* model, const ctag_camera* camera, int axis_length,
                   uint8_t* out, ptrdiff_t out_row_stride);

/* n_frames frames in DEVICE memory (frame f at frames_dev + f*frame_stride) with their detection results and the offsets /
 * pose records of ctag_pose_batch_device as it leaves them: frame f draws records offsets_dev[f] .. offsets_dev[f+1]-1 whose
 * frame field is f.  Records at index >= capacity are not read (ctag_pose_batch_device computes none there).  Output frame f
 * at out_dev + f*out_frame_stride, rows of 3*cols bytes out_row_stride apart; no byte outside them is written.  Enqueued
 * on the handle's stream; returns without waiting. */
int ctag_draw_axis_batch_device(ctag_handle* h, const uint8_t* frames_dev, int n_frames, int rows, int cols, ptrdiff_t row_stride,
                                ptrdiff_t frame_stride, const ctag_frame_result* results_dev, const int32_t* offsets_dev,
                                const ctag_pose_rec* poses_dev, int capacity, const ctag_model* model, const ctag_camera* camera,
                                int axis_length, uint8_t* out_dev, ptrdiff_t out_row_stride, ptrdiff_t out_frame_stride);

#ifdef __cplusplus
}
#endif
#endif
